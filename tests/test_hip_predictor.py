"""The ragged Conv1d -> ReLU -> LayerNorm -> Dropout stage and the variance predictor built from it on the device
(csrc/predictor.hip through transformertts_amd/predictor.py) against the fp64 oracles of tests/predictor_reference.py, to the
project's kernel bound (TOL of tests/test_hip_modes.py under conftest.rel_l2).  NaN sits behind every length of x and of the
upstream gradients throughout.  The shapes are the smallest that reach every path: one row, 32-row tiles crossed, a zero-length
utterance, Cin no multiple of 32, a length one past a tile edge, lengths below the padding of nine taps, one tap, Cin > 256 (the
column loop of the data gradient) through a strided view, and a bias that switches every ReLU off.  Measured values:
parity_reports/predictor_margin.txt (as measured on one MI355X: tests/reports/predictor_margin.txt)."""
import functools
import os
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from conftest import rel_l2
from oracle.dropmask import drop_scale, keep_flat
from predictor_reference import PARAMS, poison, predictor_grads_ref, predictor_ref, stage_bwd_ref, stage_ref, valid_mask
from test_hip_dropout_parity import REPORT_DIR
from test_hip_modes import TOL
from transformertts_amd import _lib as _library
from transformertts_amd.predictor import KernelVariancePredictor, RaggedConvNorm, ragged_conv_norm  # noqa: F401 -- no feature, no tests

_library.load()                                                       # raises when the library lacks the entries of predictor.hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5

# name -> B, Pmax, Cin, Cout, taps, lens, (row stride, batch stride) of x or None
CASES = {
    "one_row": (1, 1, 4, 32, 3, (1,), None),                          # both side taps clipped
    "tile_edge_cin36": (3, 70, 36, 96, 3, (70, 12, 0), None),         # crosses 32-row tiles; a zero-length utterance
    "shipped_256": (2, 130, 256, 256, 3, (130, 65), None),            # a length one past a tile edge
    "taps9": (2, 20, 64, 64, 9, (20, 3), None),                       # a length below the padding of 4: taps that see no row
    "taps1": (2, 20, 64, 64, 1, (20, 3), None),
    "strided_cin384": (2, 70, 384, 256, 3, (66, 70), (388, 70 * 388 + 8)),   # Cin > 256: the column loop of the plain-mode dx
    "all_negative": (2, 20, 16, 64, 3, (20, 9), None),                # bias -100: r = 0, var = 0, y = beta, rstd = 1 / sqrt(eps)
}
GRADS = ("dx", "dw", "dbias", "dgamma", "dbeta")


def _report(line):
    print(line)
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(f"{REPORT_DIR}/predictor_margin.txt", "a") as f:
        f.write(line + "\n")


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _case(name):
    """fp32 inputs with NaN behind every length of x and dy, and the oracle's forward (computed once, never modified)"""
    B, Pmax, Cin, Cout, taps, lens, _ = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    x = rng.standard_normal((B, Pmax, Cin)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, taps)) / np.sqrt(Cin * taps)).astype(np.float32)
    bias = (0.3 * rng.standard_normal(Cout)).astype(np.float32)
    if name == "all_negative":
        w, bias = (0.01 * w).astype(np.float32), np.full(Cout, -100.0, np.float32)
    gamma, beta = (1 + 0.2 * rng.standard_normal(Cout)).astype(np.float32), (0.2 * rng.standard_normal(Cout)).astype(np.float32)
    dy = rng.standard_normal((B, Pmax, Cout)).astype(np.float32)
    x, dy = poison(lens, x, dy)
    fwd = stage_ref(x, lens, w, bias, gamma, beta, EPS)
    return dict(x=x, w=w, bias=bias, gamma=gamma, beta=beta, dy=dy, lens=np.array(lens, np.int64), fwd=fwd)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _device_x(name):
    B, Pmax, Cin, _, _, _, strides = CASES[name]
    x = _dev(_case(name)["x"])
    if strides is None:
        return x, Cin, Pmax * Cin
    ld_row, ld_batch = strides
    store = torch.full((B * ld_batch,), float("nan"), device=DEV)
    view = store.as_strided((B, Pmax, Cin), (ld_batch, ld_row, 1))
    view.copy_(x)
    return view, ld_row, ld_batch


def _p(t):
    return None if t is None else c_void_p(t.data_ptr())


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _fwd(name, drop_p=0.0, seed=0, x=None, lens=None, save=True):
    """the C entry itself -> dict(y, r, mean, rstd, xm), every output pre-filled with NaN"""
    from transformertts_amd import _lib
    B, Pmax, Cin, Cout, taps, _, _ = CASES[name]
    c = _case(name)
    if x is None:
        x, ld_row, ld_batch = _device_x(name)
    else:
        B, ld_row, ld_batch = x.shape[0], Cin, Pmax * Cin
    lens = _dev(c["lens"] if lens is None else lens)
    nan = float("nan")
    o = dict(y=torch.full((B, Pmax, Cout), nan, device=DEV))
    if save:
        o.update(r=torch.full((B, Pmax, Cout), nan, device=DEV), mean=torch.full((B, Pmax), nan, device=DEV),
                 rstd=torch.full((B, Pmax), nan, device=DEV), xm=torch.full((B, Pmax, Cin), nan, device=DEV))
    par = [_dev(c[k]) for k in ("w", "bias", "gamma", "beta")]
    rc = _lib.load().ttts_ragged_conv_norm_fwd(_p(x), ld_row, ld_batch, _p(lens), *[_p(t) for t in par], B, Pmax, Cin, Cout, taps, EPS,
                                               drop_p, seed, None, _p(o["y"]), _p(o.get("r")), _p(o.get("mean")), _p(o.get("rstd")),
                                               _p(o.get("xm")), _stream())
    _lib.check(rc, "ttts_ragged_conv_norm_fwd")
    torch.cuda.synchronize()
    return o


def _bwd(name, f, dy, drop_p=0.0, seed=0, accumulate=0, into=None, lens=None, want_dx=True):
    """the C entry itself on a forward's outputs -> dict(dx, dw, dbias, dgamma, dbeta)"""
    from transformertts_amd import _lib
    _, Pmax, Cin, Cout, taps, _, _ = CASES[name]
    B = dy.shape[0]
    c = _case(name)
    lib = _lib.load()
    lens = _dev(c["lens"] if lens is None else lens)
    nan = float("nan")
    g = dict(dx=torch.full((B, Pmax, Cin), nan, device=DEV) if want_dx else None, dw=torch.full((Cout, Cin, taps), nan, device=DEV),
             dbias=torch.full((Cout,), nan, device=DEV), dgamma=torch.full((Cout,), nan, device=DEV), dbeta=torch.full((Cout,), nan, device=DEV))
    if into is not None:
        for k in GRADS[1:]:
            g[k] = into[k].clone()
    nbytes = lib.ttts_ragged_conv_norm_workspace_bytes(B, Pmax, Cin, Cout, taps)
    ws = torch.full((nbytes // 4 + 4,), nan, device=DEV)
    w, gamma = _dev(c["w"]), _dev(c["gamma"])
    rc = lib.ttts_ragged_conv_norm_bwd(_p(dy), _p(f["r"]), _p(f["mean"]), _p(f["rstd"]), _p(f["xm"]), _p(lens), _p(w), _p(gamma), B, Pmax,
                                       Cin, Cout, taps, drop_p, seed, None, _p(g["dx"]), _p(g["dw"]), _p(g["dbias"]), _p(g["dgamma"]),
                                       _p(g["dbeta"]), _p(ws), nbytes, accumulate, _stream())
    _lib.check(rc, "ttts_ragged_conv_norm_bwd")
    torch.cuda.synchronize()
    return g


def _behind_are_zero(t, lens):
    return all(bool((t[b, max(int(n), 0):] == 0).all()) for b, n in enumerate(lens))


def _gate_check(name, r_kernel, fwd, lens):
    """the gate the kernel took may differ from the fp64 one only where the pre-activation is zero to within the forward's bound"""
    valid = valid_mask(lens, r_kernel.shape[1])[:, :, None].expand_as(fwd["z"])
    gate = (r_kernel.cpu() > 0) & valid
    differs = (gate != ((fwd["z"] > 0) & valid))
    zmax = fwd["z"].abs().max().item()
    worst = fwd["z"].abs()[differs].max().item() if bool(differs.any()) else 0.0
    _report(f"{name}: gate differs at {int(differs.sum())} of {int(valid.sum())} valid elements, largest |z| there {worst:.3e} (max|z| {zmax:.3e})")
    assert worst <= TOL * zmax
    assert int(differs.sum()) <= 1e-4 * int(valid.sum())
    return gate


@pytest.mark.parametrize("name", list(CASES))
def test_the_stage_forward_against_fp64(name):
    B, Pmax, Cin, Cout, taps, lens, _ = CASES[name]
    c = _case(name)
    o = _fwd(name)
    errs = {k: rel_l2(o[k], c["fwd"][k]) for k in ("y", "r", "mean", "rstd")}
    _report(f"{name} forward: " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    for k in ("y", "r", "mean", "rstd", "xm"):
        assert not bool(torch.isnan(o[k]).any()), k                   # no NaN anywhere: nothing behind a length was used
        assert _behind_are_zero(o[k], lens), k
    assert all(v < TOL for v in errs.values()), errs
    assert _same_bits(o["xm"], np.nan_to_num(c["x"]))
    if name == "all_negative":
        valid = valid_mask(lens, Pmax).to(DEV)
        assert bool((o["r"] == 0).all()) and bool((o["mean"] == 0).all())
        assert _same_bits(o["y"][valid], _dev(c["beta"]).expand(int(valid.sum()), Cout))
        assert rel_l2(o["rstd"][valid], torch.full((int(valid.sum()),), 1.0 / np.sqrt(EPS), dtype=torch.float64)) < 1e-6
    light = _fwd(name, save=False)                                    # the inference form: y alone, the same bits
    assert _same_bits(light["y"], o["y"])
    again = _fwd(name)
    assert all(_same_bits(again[k], o[k]) for k in o)


@pytest.mark.parametrize("name,scale", [(n, 1.0) for n in CASES] + [("tile_edge_cin36", 2e-7)])
def test_the_stage_backward_against_fp64(name, scale):
    B, Pmax, Cin, Cout, taps, lens, _ = CASES[name]
    c = _case(name)
    f = _fwd(name)
    gate = _gate_check(name, f["r"], c["fwd"], lens)
    dy_host = (c["dy"] * np.float32(scale)).astype(np.float32)
    ref = stage_bwd_ref(dy_host, c["fwd"], lens, c["w"], c["gamma"], gate)
    dy = _dev(dy_host)
    g = _bwd(name, f, dy)
    errs = {k: rel_l2(g[k], ref[k]) for k in GRADS}
    _report(f"{name} backward (dy x {scale:g}): " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    for k in GRADS:
        assert not bool(torch.isnan(g[k]).any()), k
    assert _behind_are_zero(g["dx"], lens)
    assert all(v < TOL for v in errs.values()), errs
    if scale != 1.0:
        return
    again = _bwd(name, f, dy)
    assert all(_same_bits(again[k], g[k]) for k in GRADS)             # the same bits on every call
    no_dx = _bwd(name, f, dy, want_dx=False)
    assert all(_same_bits(no_dx[k], g[k]) for k in GRADS[1:])
    rng = np.random.default_rng(5)
    into = {k: _dev(rng.standard_normal(tuple(g[k].shape)).astype(np.float32)) for k in GRADS[1:]}
    acc = _bwd(name, f, dy, accumulate=1, into=into)
    for k in ("dbias", "dgamma", "dbeta"):
        assert _same_bits(acc[k], into[k] + g[k]), k                  # one fp32 add onto what was there
    assert rel_l2(acc["dw"], into["dw"].double() + ref["dw"].to(DEV)) < TOL and _same_bits(acc["dx"], g["dx"])


def test_an_utterance_alone_has_the_bits_it_has_in_the_batch():
    name = "tile_edge_cin36"
    c = _case(name)
    x, _, _ = _device_x(name)
    f = _fwd(name)
    dy = _dev(c["dy"])
    g = _bwd(name, f, dy)
    f0 = _fwd(name, x=x[:1].contiguous(), lens=c["lens"][:1])
    g0 = _bwd(name, f0, dy[:1].contiguous(), lens=c["lens"][:1])
    for k in ("y", "r", "mean", "rstd"):
        assert _same_bits(f0[k], f[k][:1]), k
    assert _same_bits(g0["dx"], g["dx"][:1])


@pytest.mark.parametrize("name", ["tile_edge_cin36", "shipped_256"])
def test_dropout_is_the_oracles_mask_forward_and_backward(name):
    B, Pmax, Cin, Cout, taps, lens, _ = CASES[name]
    c = _case(name)
    p, seed = 0.5, 0x1234ABCD5678
    keep = keep_flat(seed, B * Pmax * Cout, p).reshape(B, Pmax, Cout)
    scale = np.float32(drop_scale(p))
    plain, dropped = _fwd(name), _fwd(name, drop_p=p, seed=seed)
    want = np.where(keep, plain["y"].cpu().numpy() * scale, np.float32(0)).astype(np.float32)
    assert _same_bits(dropped["y"], want)                             # the kept set and the kept values, bit for bit
    valid = valid_mask(lens, Pmax).numpy()
    nonzero = (dropped["y"].cpu().numpy() != 0)[valid]
    assert np.array_equal(nonzero, keep[valid] & (plain["y"].cpu().numpy() != 0)[valid])
    assert all(_same_bits(dropped[k], plain[k]) for k in ("r", "mean", "rstd", "xm"))
    gate = _gate_check(name + " (dropout)", dropped["r"], c["fwd"], lens)
    ref = stage_bwd_ref(c["dy"], c["fwd"], lens, c["w"], c["gamma"], gate, keep=keep, scale=float(scale))
    g = _bwd(name, dropped, _dev(c["dy"]), drop_p=p, seed=seed)
    errs = {k: rel_l2(g[k], ref[k]) for k in GRADS}
    _report(f"{name} backward under dropout 0.5: " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert all(v < TOL for v in errs.values()), errs


def test_the_autograd_function_is_the_entry_points_and_eval_ignores_dropout():
    from transformertts_amd import RaggedConvNorm, ragged_conv_norm
    name = "strided_cin384"
    B, Pmax, Cin, Cout, taps, lens, _ = CASES[name]
    c = _case(name)
    x, _, _ = _device_x(name)
    x.requires_grad_(True)
    par = [_dev(c[k]).requires_grad_(True) for k in ("w", "bias", "gamma", "beta")]
    pl = _dev(c["lens"])
    y = ragged_conv_norm(x, pl, *par, eps=EPS)
    dy = _dev(c["dy"])
    y.backward(dy)
    f = _fwd(name)
    g = _bwd(name, f, dy)
    assert _same_bits(y, f["y"]) and x.grad.shape == x.shape
    for t, k in zip([x] + par, ("dx", "dw", "dbias", "dgamma", "dbeta")):
        assert _same_bits(t.grad, g[k]), k
    with torch.no_grad():
        assert _same_bits(ragged_conv_norm(x, pl, *par, eps=EPS, drop_p=0.5, seed=77, training=False), f["y"])
        dropped = ragged_conv_norm(x, pl, *par, eps=EPS, drop_p=0.5, seed=77)
        assert _same_bits(dropped, _fwd(name, drop_p=0.5, seed=77)["y"]) and not _same_bits(dropped, f["y"])
    m = RaggedConvNorm(Cin, Cout, kernel_size=taps, dropout=0.5).to(DEV)
    with torch.no_grad():
        for t, k in zip((m.conv.weight, m.conv.bias, m.norm.weight, m.norm.bias), ("w", "bias", "gamma", "beta")):
            t.copy_(_dev(c[k]))
        assert _same_bits(m.eval()(x, pl), f["y"])
        a, b = m.train()(x, pl), m(x, pl)
        assert not _same_bits(a, b) and 0.4 < float((a[0, :66] == 0).float().mean()) < 0.6       # a fresh seed per call


# ------------------------------------------------------------------------------------------------ the predictor, the adaptor
PREDICTORS = {"cin36_hidden96": (3, 70, 36, 96, (70, 12, 0)), "shipped_256": (2, 130, 256, 256, (130, 65))}


@functools.lru_cache(maxsize=None)
def _predictor_case(name):
    B, Pmax, d, hidden, lens = PREDICTORS[name]
    from transformertts_amd.variance import VariancePredictor
    torch.manual_seed(sum(map(ord, name)))
    stock = VariancePredictor(d, hidden=hidden)
    with torch.no_grad():
        for p in stock.parameters():
            p.add_(0.1 * torch.randn_like(p))
    sd = {k: v.detach().clone() for k, v in stock.state_dict().items()}
    rng = np.random.default_rng(3)
    x, dout = poison(lens, rng.standard_normal((B, Pmax, d)).astype(np.float32), rng.standard_normal((B, Pmax)).astype(np.float32))
    out, dx, grads = predictor_grads_ref(x, lens, sd, dout, EPS)
    return dict(sd=sd, x=x, dout=dout, out=out, dx=dx, grads=grads)


@pytest.mark.parametrize("name", list(PREDICTORS))
def test_the_predictor_against_fp64_forward_and_every_gradient(name):
    from transformertts_amd import KernelVariancePredictor, VariancePredictor
    B, Pmax, d, hidden, lens = PREDICTORS[name]
    c = _predictor_case(name)
    ours, stock = KernelVariancePredictor(d, hidden=hidden).to(DEV).eval(), VariancePredictor(d, hidden=hidden).to(DEV).eval()
    ours.load_state_dict(c["sd"], strict=True)
    stock.load_state_dict(ours.state_dict(), strict=True)
    x, pl = _dev(c["x"]).requires_grad_(True), torch.tensor(lens, device=DEV)
    out = ours(x, pl)
    out.backward(_dev(c["dout"]))
    with torch.no_grad():
        out_stock = stock(x, pl)
    errs = {"out": rel_l2(out, c["out"]), "out (stock torch)": rel_l2(out_stock, c["out"]), "dx": rel_l2(x.grad, c["dx"])}
    errs.update({k: rel_l2(p.grad, c["grads"][k]) for k, p in ours.named_parameters()})
    _report(f"predictor {name}: " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert set(errs) == {"out", "out (stock torch)", "dx"} | set(PARAMS)
    assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(x.grad).any())
    assert _behind_are_zero(out, lens) and _behind_are_zero(x.grad, lens)
    assert all(v < TOL for v in errs.values()), errs
    first = {k: p.grad.clone() for k, p in ours.named_parameters()}
    dx1 = x.grad.clone()
    ours.zero_grad(set_to_none=True)
    x.grad = None
    ours(x, pl).backward(_dev(c["dout"]))
    assert _same_bits(x.grad, dx1) and all(_same_bits(p.grad, first[k]) for k, p in ours.named_parameters())


def test_a_captured_eval_call_replayed_on_another_input():
    from transformertts_amd import KernelVariancePredictor
    B, Pmax, d, hidden, lens = PREDICTORS["cin36_hidden96"]
    c = _predictor_case("cin36_hidden96")
    m = KernelVariancePredictor(d, hidden=hidden).to(DEV).eval()
    m.load_state_dict(c["sd"], strict=True)
    x0 = _dev(c["x"])
    x1 = torch.where(torch.isnan(x0), x0, x0 * 1.5 + 0.25)
    static, pl = x0.clone(), torch.tensor(lens, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():                    # (warm-up: the library is loaded, the allocator primed)
        m(static, pl)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        got = m(static, pl)
    seen = []
    for x in (x0, x1):
        static.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        with torch.no_grad():
            eager = m(x.clone(), pl)
        assert _same_bits(got, eager) and not bool(torch.isnan(got).any())
        seen.append(got.clone())
    assert not torch.equal(seen[0], seen[1])                          # the replay did follow the input


def test_the_adaptor_on_kernel_predictors_through_the_losses():
    from transformertts_amd import KernelVariancePredictor, VarianceAdaptor, VarianceLoss
    from variance_reference import poison as poison_targets, variance_loss_grad_ref
    B, Pmax, d, hidden, lens = PREDICTORS["shipped_256"]
    torch.manual_seed(11)
    a = VarianceAdaptor(d, n_bins=16, predictor=KernelVariancePredictor, max_len=64).to(DEV).eval()
    with torch.no_grad():
        for p in a.parameters():
            p.add_(0.05 * torch.randn_like(p))
    x_host, dur, pitch, energy = poison_targets(np.random.default_rng(4), B, Pmax, d, lens)
    pitch = (pitch / 100).astype(np.float32)
    x, pl = _dev(x_host).requires_grad_(True), torch.tensor(lens, device=DEV)
    out = a(x, pl, durations=_dev(dur), pitch=_dev(pitch), energy=_dev(energy))
    for k in ("log_duration", "pitch", "energy"):
        out[k].retain_grad()
    VarianceLoss((1.0, 0.5, 2.0))(out, _dev(dur), _dev(pitch), _dev(energy), pl)["total"].backward()
    names = (("log_duration", a.duration_predictor), ("pitch", a.pitch_predictor), ("energy", a.energy_predictor))
    sds = {k: {n: v.detach().cpu() for n, v in m.state_dict().items()} for k, m in names}
    ref = {k: predictor_ref(x_host, lens, sds[k], EPS) for k, _ in names}
    gout = np.array([0.0, 0.0, 0.0, 1.0])
    dref = variance_loss_grad_ref(ref["log_duration"].numpy(), dur, ref["pitch"].numpy(), pitch, ref["energy"].numpy(), energy, lens,
                                  (1.0, 0.5, 2.0), gout)
    errs, dx = {}, 0
    for (k, m), dk in zip(names, dref):
        _, dxk, grads = predictor_grads_ref(x_host, lens, sds[k], np.asarray(dk, np.float64), EPS)
        dx = dx + dxk
        errs[k] = rel_l2(out[k], ref[k])
        errs["d " + k] = rel_l2(out[k].grad, torch.from_numpy(np.asarray(dk, np.float64)))
        errs[k + " conv1.weight.grad"] = rel_l2(m.conv1.weight.grad, grads["conv1.weight"])
    errs["dx"] = rel_l2(x.grad, dx)
    _report("adaptor chain shipped_256: " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert not bool(torch.isnan(x.grad).any()) and _behind_are_zero(x.grad, lens)
    assert all(v < TOL for v in errs.values()), errs
