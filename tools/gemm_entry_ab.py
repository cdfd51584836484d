"""One sha256 per output buffer of the 17 forward-type GEMM entry points (Linear / Conv1d, forward / data gradient, in the fp32,
bf16x6, fp16x3, image-operand, LDS-DMA and head-image-output forms) on fixed seeded inputs: an A/B of two builds of the library.

    TTTS_LIB=<libttts_hip.so of build A> python tools/gemm_entry_ab.py > a.txt
    TTTS_LIB=<libttts_hip.so of build B> python tools/gemm_entry_ab.py > b.txt      (a fresh process each), then diff a.txt b.txt

Small shapes: a ragged row count; for fp16x3 a width and depth that are multiples of 4 but not of 32; for the image-operand /
LDS-DMA forms a depth of 32 and of 256.  Every epilogue option is driven on its own: bias, residual, relu, dropout with a seed and a
device step word, a row shift, the relu gate of a data gradient, an `*_amax_out` array, BatchNorm partials, two amax sections.
Needs a GPU; exits non-zero when an entry refuses.  profiles/gemm_entry_ab.txt holds the digests of this tree and of its parent."""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from transformertts_amd import _lib, ops  # noqa: E402
from transformertts_amd.ops import _p, _stream  # noqa: E402

DEV = torch.device("cuda:0")
M = 333                     # three utterances of 111 rows: ragged against every tile height


def rand(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def digest(t: torch.Tensor) -> str:
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def report(entry: str, case: str, rc: int, **buffers) -> None:
    if rc != 0:
        sys.exit(f"{entry} {case}: rc {rc}: {_lib.last_error()}")
    for name, t in buffers.items():
        if t is not None:
            print(f"{entry} {case} {name} {digest(t)}")


def image_of(lib, x, rows, K):
    img, inv = torch.empty(rows * K * 2, dtype=torch.int16, device=DEV), torch.empty(rows, device=DEV)
    _lib.check(lib.ttts_act_image(_p(x), _p(img), _p(inv), rows, K, _stream()), "ttts_act_image")
    return img, inv


# form -> (weight-image mode of the forward, of the data gradient; None: the fp32 weight itself), shapes (N, K)
LINEAR = {"": (None, None, [(100, 80)]), "_x6": (0, 1, [(100, 80)]), "_h3": (4, 5, [(100, 84)]),
          "_h3i": (8, 9, [(132, 32), (132, 256)]), "_h3d": (8, 9, [(132, 32), (132, 256)])}


def linear_fwd(lib, form: str, N: int, K: int) -> None:
    entry = "linear_fwd" + form
    fn = getattr(lib, "ttts_" + entry)
    x, w, b, res = rand(M, K, seed=1), rand(N, K, seed=2, scale=K ** -0.5), rand(N, seed=3), rand(M, N, seed=4)
    mode = LINEAR[form][0]
    wp = w if mode is None else ops._planes(w, mode, N, K)
    step = torch.tensor([0x1234_5678_9ABC], dtype=torch.int64, device=DEV)
    xa = ops._amax(x)
    lead = (*image_of(lib, x, M, K),) if form == "_h3i" else (x,)
    shifts = form in ("", "_x6", "_h3")
    cases = {"bias": dict(bias=b), "plain": dict(), "residual": dict(bias=b, residual=res), "relu": dict(bias=b, act=1),
             "dropout": dict(bias=b, p=0.3, seed=1234, step=step), "dropout_relu": dict(bias=b, act=1, p=0.3, seed=77)}
    if shifts:
        cases["shift"] = dict(bias=b, shift=1, T=111)
        cases["shift_back"] = dict(bias=b, shift=-1, T=111)
    if form not in ("", "_x6"):
        cases["amax_out"] = dict(bias=b, act=1, amax=True)
    for case, o in cases.items():
        y = torch.full((M, N), float("nan"), device=DEV)
        am = torch.zeros(ops.AMAX_SLOTS, device=DEV) if o.get("amax") else None
        args = [*(_p(t) for t in lead), _p(wp), _p(o.get("bias")), _p(o.get("residual")), _p(y), M, N, K, o.get("act", 0), o.get("p", 0.0),
                o.get("seed", 0), _p(o.get("step"))]
        if shifts:
            args += [o.get("shift", 0), o.get("T", 0)]
        if form in ("_h3", "_h3d"):
            args.append(_p(xa))
        if form not in ("", "_x6"):
            args.append(_p(am))
        report(entry, f"N{N}_K{K}_{case}", fn(*args, _stream()), y=y, amax=am)


def linear_fwd_img(lib, N: int, K: int, sec: int) -> None:
    x, w, b = rand(M, K, seed=1), rand(N, K, seed=2, scale=K ** -0.5), rand(N, seed=3)
    y = torch.zeros(M, N, device=DEV)
    inv = torch.zeros(N // 64, M, device=DEV)
    am = torch.zeros(N // sec, ops.AMAX_SLOTS, device=DEV) if sec else None
    rc = lib.ttts_linear_fwd_h3d_img(_p(x), _p(ops._planes(w, 8, N, K)), _p(b), _p(y), _p(inv), M, N, K, _p(ops._amax(x)), _p(am), sec,
                                     _stream())
    report("linear_fwd_h3d_img", f"N{N}_K{K}_sec{sec}", rc, y_image=y, y_row_inv=inv, amax=am)


def linear_bwd_data(lib, form: str, N: int, K: int) -> None:
    entry = "linear_bwd_data" + form
    fn = getattr(lib, "ttts_" + entry)
    dy, w, res = rand(M, N, seed=5, scale=1e-3), rand(N, K, seed=2, scale=K ** -0.5), rand(M, K, seed=6, scale=1e-3)
    gate = torch.relu(rand(M, K, seed=7))
    mode = LINEAR[form][1]
    wp = w if mode is None else ops._planes(w, mode, K, N)
    da = ops._amax(dy)
    lead = (*image_of(lib, dy, M, N),) if form == "_h3i" else (dy,)
    cases = {"plain": dict(), "residual": dict(residual=res), "gate": dict(gate=gate, scale=1.25),
             "gate_residual": dict(residual=res, gate=gate, scale=1.25)}
    if form not in ("", "_x6"):
        cases["amax_out"] = dict(amax=True)
    for case, o in cases.items():
        dx = torch.full((M, K), float("nan"), device=DEV)
        am = torch.zeros(ops.AMAX_SLOTS, device=DEV) if o.get("amax") else None
        args = [*(_p(t) for t in lead), _p(wp), _p(o.get("residual")), _p(dx), M, N, K, _p(o.get("gate")), o.get("scale", 1.0)]
        if form in ("_h3", "_h3d"):
            args.append(_p(da))
        if form not in ("", "_x6"):
            args.append(_p(am))
        report(entry, f"N{N}_K{K}_{case}", fn(*args, _stream()), dx=dx, amax=am)


def conv(lib, form: str, B: int, T: int, cin: int, cout: int, taps: int, bn: bool = False) -> None:
    x, w, b = rand(B, T, cin, seed=1), rand(cout, cin, taps, seed=2, scale=(taps * cin) ** -0.5), rand(cout, seed=3)
    dy = rand(B, T, cout, seed=4, scale=1e-3)
    if form == "":
        w_fwd, w_bwd = torch.empty(cout * taps * cin, device=DEV), torch.empty(cin * taps * cout, device=DEV)
        _lib.check(lib.ttts_conv1d_pack_weight(_p(w), _p(w_fwd), _p(w_bwd), cout, cin, taps, _stream()), "ttts_conv1d_pack_weight")
    else:
        base = 2 if form == "_x6" else 6
        w_fwd = ops._planes(w, base, cout, taps * cin, cin, taps)
        w_bwd = ops._planes(w, base + 1, cin, taps * cout, cout, taps)
    shape = f"B{B}_T{T}_cin{cin}_cout{cout}_taps{taps}"
    y = torch.full((B, T, cout), float("nan"), device=DEV)
    dx = torch.full((B, T, cin), float("nan"), device=DEV)
    fwd, bwd = getattr(lib, "ttts_conv1d_fwd" + form), getattr(lib, "ttts_conv1d_bwd_data" + form)
    if form == "_h3":
        ws = None
        if bn:
            nblk = lib.ttts_conv1d_fwd_h3_bn_blocks(B, T, cin, cout, taps)
            if nblk <= 0:
                sys.exit(f"conv1d_fwd_h3 {shape}: no BatchNorm partials for this shape")
            ws = torch.zeros(lib.ttts_bn_workspace_bytes(B * T, cout) // 4, device=DEV)
        rc = fwd(_p(x), _p(w_fwd), _p(b), _p(y), B, T, cin, cout, taps, _p(ops._amax(x)), _p(ws), _stream())
        report("conv1d_fwd_h3", shape + ("_bn" if bn else ""), rc, y=y, bn_partials=ws)
        report("conv1d_bwd_data_h3", shape, bwd(_p(dy), _p(w_bwd), _p(dx), B, T, cin, cout, taps, _p(ops._amax(dy)), _stream()), dx=dx)
    else:
        report("conv1d_fwd" + form, shape, fwd(_p(x), _p(w_fwd), _p(b), _p(y), B, T, cin, cout, taps, _stream()), y=y)
        report("conv1d_bwd_data" + form, shape, bwd(_p(dy), _p(w_bwd), _p(dx), B, T, cin, cout, taps, _stream()), dx=dx)


def main() -> None:
    lib = _lib.load()
    print(f"# abi {lib.ttts_abi_version()}")
    for form, (_, _, shapes) in LINEAR.items():
        for N, K in shapes:
            linear_fwd(lib, form, N, K)
            linear_bwd_data(lib, form, K, N)        # (the data gradient reduces over ITS N: the same depths)
    for K in (32, 256):
        linear_fwd_img(lib, 256, K, 0)
        linear_fwd_img(lib, 256, K, 128)
    for form in ("", "_x6"):
        conv(lib, form, 3, 37, 32, 48, 5)
        conv(lib, form, 1, 1, 16, 16, 1)
    conv(lib, "_h3", 3, 37, 20, 44, 5)
    conv(lib, "_h3", 3, 50, 128, 256, 5, bn=True)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
