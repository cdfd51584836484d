"""The conv feed-forward sublayer, the FFT block and the FastSpeech-2 student on the device (csrc/predictor.hip through
transformertts_amd/fft.py) against the oracles of tests/fft_reference.py.  The sublayer is held to the project's kernel bound (TOL
of tests/test_hip_modes.py under conftest.rel_l2: its products are exact fp32 MFMA); the block and the student, whose attention
half is fp16x3, to twice the error of the stock-torch fp32 restatement from the same `state_dict` against the same fp64, and to
1e-4.  NaN sits behind every length of x and of the upstream gradients of the sublayer throughout (the block's input must be
finite: the contract of its attention half).  The shapes are the smallest that reach every path: one row, 32-row tiles crossed
with a zero-length utterance and a partial second block of hidden columns, the shipped widths (four column blocks, reduction
depth 1024), a second convolution with taps, a strided view, and a bias that switches every ReLU off.
Dropout: the kept set is checked exactly everywhere; the kept VALUES are checked bit for bit where the residual is an exact zero
(there s is the branch itself; elsewhere the fp32 add of the residual rounds once more and only the fp64 bound can hold).
Measured values: parity_reports/fft_margin.txt (as measured on one MI355X: tests/reports/fft_margin.txt)."""
import functools
import os
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from conftest import rel_l2
from fft_reference import BLOCK_PARAMS, fft_block_ref, ffn_bwd_ref, ffn_ref, poison, student_ref, valid_mask
from oracle.dropmask import drop_scale, keep_flat
from test_hip_dropout_parity import REPORT_DIR
from test_hip_modes import TOL
from transformertts_amd import _lib as _library
from transformertts_amd.fft import ConvFeedForward, FastSpeech2Student, FFTBlock, ragged_conv_ffn  # noqa: F401 -- no feature, no tests

_library.load()                                                       # raises when the library lacks the entries

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5

# name -> B, Pmax, D, Chid, k1, k2, lens, (row stride, batch stride) of x or None
CASES = {
    "one_row": (1, 1, 32, 32, 1, 1, (1,), None),
    "tiles_hidden288": (3, 70, 64, 288, 9, 1, (70, 12, 0), None),     # 32-row tiles crossed; hidden columns 256 + 32; a zero length
    "shipped": (2, 40, 256, 1024, 9, 1, (40, 33), None),              # four column blocks, reduction depth 1024
    "taps33": (2, 20, 64, 64, 3, 3, (20, 3), None),                   # a second convolution with taps
    "strided": (2, 70, 64, 288, 9, 1, (66, 70), (68, 70 * 68 + 8)),   # NaN between the rows and the utterances
    "gates_off": (2, 20, 64, 64, 3, 3, (20, 9), None),                # b1 = -100, b2 = 0: h = 0, y = LayerNorm(x'), dw1 = 0
}
PARAMS = ("w1", "b1", "w2", "b2", "gamma", "beta")
GRADS = ("dx", "dw1", "db1", "dw2", "db2", "dgamma", "dbeta")


def _report(line):
    print(line)
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(f"{REPORT_DIR}/fft_margin.txt", "a") as f:
        f.write(line + "\n")


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _case(name, sparse=False):
    """fp32 inputs with NaN behind every length of x and dy, and the oracle's forward (computed once, never modified).  sparse:
    a quarter of x's elements are exact zeros (the dropout test reads the branch's bits there)."""
    B, Pmax, D, Chid, k1, k2, lens, _ = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    x = rng.standard_normal((B, Pmax, D)).astype(np.float32)
    if sparse:
        x[rng.random((B, Pmax, D)) < 0.25] = 0.0
    w1 = (rng.standard_normal((Chid, D, k1)) / np.sqrt(D * k1)).astype(np.float32)
    b1 = (0.3 * rng.standard_normal(Chid)).astype(np.float32)
    w2 = (rng.standard_normal((D, Chid, k2)) / np.sqrt(Chid * k2)).astype(np.float32)
    b2 = (0.3 * rng.standard_normal(D)).astype(np.float32)
    if name == "gates_off":
        w1, b1, b2 = (0.01 * w1).astype(np.float32), np.full(Chid, -100.0, np.float32), np.zeros(D, np.float32)
    gamma, beta = (1 + 0.2 * rng.standard_normal(D)).astype(np.float32), (0.2 * rng.standard_normal(D)).astype(np.float32)
    dy = rng.standard_normal((B, Pmax, D)).astype(np.float32)
    x, dy = poison(lens, x, dy)
    fwd = ffn_ref(x, lens, w1, b1, w2, b2, gamma, beta, EPS)
    # the gate condition's cap must be reachable: fp64 itself has at most 1e-4 of the valid pre-activations inside the band
    valid = valid_mask(lens, Pmax)[:, :, None].expand_as(fwd["z1"])
    near = (fwd["z1"].abs() <= TOL * fwd["z1"].abs().max()) & valid
    assert int(near.sum()) <= 1e-4 * int(valid.sum()), (name, int(near.sum()))
    return dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, gamma=gamma, beta=beta, dy=dy, lens=np.array(lens, np.int64), fwd=fwd)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _device_x(name, sparse=False):
    B, Pmax, D, _, _, _, _, strides = CASES[name]
    x = _dev(_case(name, sparse)["x"])
    if strides is None:
        return x, D, Pmax * D
    ld_row, ld_batch = strides
    store = torch.full((B * ld_batch,), float("nan"), device=DEV)
    view = store.as_strided((B, Pmax, D), (ld_batch, ld_row, 1))
    view.copy_(x)
    return view, ld_row, ld_batch


def _p(t):
    return None if t is None else c_void_p(t.data_ptr())


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _fwd(name, drop_p=0.0, seed=0, x=None, lens=None, save=True, sparse=False):
    """the C entry itself -> dict(y, h, s, mean, rstd, xm), every output pre-filled with NaN"""
    from transformertts_amd import _lib
    B, Pmax, D, Chid, k1, k2, _, _ = CASES[name]
    c = _case(name, sparse)
    if x is None:
        x, ld_row, ld_batch = _device_x(name, sparse)
    else:
        B, ld_row, ld_batch = x.shape[0], D, Pmax * D
    lens = _dev(c["lens"] if lens is None else lens)
    nan = float("nan")
    o = dict(y=torch.full((B, Pmax, D), nan, device=DEV), h=torch.full((B, Pmax, Chid), nan, device=DEV))
    if save:
        o.update(s=torch.full((B, Pmax, D), nan, device=DEV), mean=torch.full((B, Pmax), nan, device=DEV),
                 rstd=torch.full((B, Pmax), nan, device=DEV), xm=torch.full((B, Pmax, D), nan, device=DEV))
    par = [_dev(c[k]) for k in PARAMS]
    rc = _lib.load().ttts_ragged_conv_ffn_fwd(_p(x), ld_row, ld_batch, _p(lens), *[_p(t) for t in par], B, Pmax, D, Chid, k1, k2, EPS,
                                              drop_p, seed, None, _p(o["h"]), _p(o["y"]), _p(o.get("s")), _p(o.get("mean")),
                                              _p(o.get("rstd")), _p(o.get("xm")), _stream())
    _lib.check(rc, "ttts_ragged_conv_ffn_fwd")
    torch.cuda.synchronize()
    return o


def _bwd(name, f, dy, drop_p=0.0, seed=0, accumulate=0, into=None, lens=None, want_dx=True, want_dw=True, sparse=False):
    """the C entry itself on a forward's outputs -> dict of GRADS"""
    from transformertts_amd import _lib
    _, Pmax, D, Chid, k1, k2, _, _ = CASES[name]
    B = dy.shape[0]
    c = _case(name, sparse)
    lib = _lib.load()
    lens = _dev(c["lens"] if lens is None else lens)
    nan = float("nan")
    shapes = dict(dx=(B, Pmax, D), dw1=(Chid, D, k1), db1=(Chid,), dw2=(D, Chid, k2), db2=(D,), dgamma=(D,), dbeta=(D,))
    g = {k: torch.full(shapes[k], nan, device=DEV) for k in GRADS}
    if not want_dx:
        g["dx"] = None
    if not want_dw:
        g.update(dw1=None, db1=None, dw2=None, db2=None)
    if into is not None:
        for k in GRADS[1:]:
            g[k] = into[k].clone()
    nbytes = lib.ttts_ragged_conv_ffn_workspace_bytes(B, Pmax, D, Chid, k1, k2)
    ws = torch.full((nbytes // 4 + 4,), nan, device=DEV)
    w1, w2, gamma = _dev(c["w1"]), _dev(c["w2"]), _dev(c["gamma"])
    rc = lib.ttts_ragged_conv_ffn_bwd(_p(dy), _p(f["s"]), _p(f["mean"]), _p(f["rstd"]), _p(f["h"]), _p(f["xm"]), _p(lens), _p(w1), _p(w2),
                                      _p(gamma), B, Pmax, D, Chid, k1, k2, drop_p, seed, None, *[_p(g[k]) for k in GRADS], _p(ws), nbytes,
                                      accumulate, _stream())
    _lib.check(rc, "ttts_ragged_conv_ffn_bwd")
    torch.cuda.synchronize()
    return g


def _behind_are_zero(t, lens):
    return all(bool((t[b, max(int(n), 0):] == 0).all()) for b, n in enumerate(lens))


def _gate_check(name, h_kernel, fwd, lens):
    """the gate the kernel took may differ from the fp64 one only where the pre-activation is zero to within the forward's bound,
    and on at most 1e-4 of the valid elements"""
    valid = valid_mask(lens, h_kernel.shape[1])[:, :, None].expand_as(fwd["z1"])
    gate = (h_kernel.cpu() > 0) & valid
    differs = (gate != ((fwd["z1"] > 0) & valid))
    zmax = fwd["z1"].abs().max().item()
    worst = fwd["z1"].abs()[differs].max().item() if bool(differs.any()) else 0.0
    _report(f"{name}: gate differs at {int(differs.sum())} of {int(valid.sum())} valid elements, largest |z1| there {worst:.3e} (max|z1| {zmax:.3e})")
    assert worst <= TOL * zmax
    assert int(differs.sum()) <= 1e-4 * int(valid.sum())
    return gate


@pytest.mark.parametrize("name", list(CASES))
def test_the_sublayer_forward_against_fp64(name):
    B, Pmax, D, Chid, k1, k2, lens, _ = CASES[name]
    c = _case(name)
    o = _fwd(name)
    errs = {k: rel_l2(o[k], c["fwd"][k]) for k in ("y", "h", "s", "mean", "rstd")}
    _report(f"{name} forward: " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    for k in ("y", "h", "s", "mean", "rstd", "xm"):
        assert not bool(torch.isnan(o[k]).any()), k                   # no NaN anywhere: nothing behind a length was used
        assert _behind_are_zero(o[k], lens), k
    assert all(v < TOL for v in errs.values()), errs
    assert _same_bits(o["xm"], np.nan_to_num(c["x"]))                 # x' bit for bit
    if name == "gates_off":
        assert bool((o["h"] == 0).all())
        xm = torch.from_numpy(np.nan_to_num(c["x"])).double()
        want = torch.nn.functional.layer_norm(xm, (D,), torch.from_numpy(c["gamma"]).double(), torch.from_numpy(c["beta"]).double(), EPS)
        want = torch.where(valid_mask(lens, Pmax)[:, :, None], want, torch.zeros((), dtype=torch.float64))
        assert rel_l2(o["y"], want) < TOL and _same_bits(o["s"], np.nan_to_num(c["x"]))
    light = _fwd(name, save=False)                                    # the inference form: y and h alone, the same bits
    assert _same_bits(light["y"], o["y"]) and _same_bits(light["h"], o["h"])
    again = _fwd(name)
    assert all(_same_bits(again[k], o[k]) for k in o)


@pytest.mark.parametrize("scale", [1.0, 2e-7])
@pytest.mark.parametrize("name", list(CASES))
def test_the_sublayer_backward_against_fp64(name, scale):
    B, Pmax, D, Chid, k1, k2, lens, _ = CASES[name]
    c = _case(name)
    f = _fwd(name)
    gate = _gate_check(name, f["h"], c["fwd"], lens)
    dy_host = (c["dy"] * np.float32(scale)).astype(np.float32)
    ref = ffn_bwd_ref(dy_host, c["fwd"], lens, c["w1"], c["w2"], c["gamma"], gate)
    dy = _dev(dy_host)
    g = _bwd(name, f, dy)
    errs = {k: rel_l2(g[k], ref[k]) for k in GRADS}
    _report(f"{name} backward (dy x {scale:g}): " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    for k in GRADS:
        assert not bool(torch.isnan(g[k]).any()), k
    assert _behind_are_zero(g["dx"], lens)
    assert all(v < TOL for v in errs.values()), errs
    if name == "gates_off":
        assert bool((g["dw1"] == 0).all()) and bool((g["db1"] == 0).all())
    if scale != 1.0:
        return
    again = _bwd(name, f, dy)
    assert all(_same_bits(again[k], g[k]) for k in GRADS)             # the same bits on every call
    no_dx = _bwd(name, f, dy, want_dx=False)
    assert all(_same_bits(no_dx[k], g[k]) for k in GRADS[1:])
    no_dw = _bwd(name, f, dy, want_dw=False)
    assert all(_same_bits(no_dw[k], g[k]) for k in ("dx", "dgamma", "dbeta"))
    rng = np.random.default_rng(5)
    into = {k: _dev(rng.standard_normal(tuple(g[k].shape)).astype(np.float32)) for k in GRADS[1:]}
    acc = _bwd(name, f, dy, accumulate=1, into=into)
    for k in ("dgamma", "dbeta"):
        assert _same_bits(acc[k], into[k] + g[k]), k                  # one fp32 add onto what was there
    for k in ("dw1", "db1", "dw2", "db2"):
        assert rel_l2(acc[k], into[k].double() + ref[k].to(DEV)) < TOL, k
    assert _same_bits(acc["dx"], g["dx"])


def test_an_utterance_alone_has_the_bits_it_has_in_the_batch():
    name = "tiles_hidden288"
    c = _case(name)
    x, _, _ = _device_x(name)
    f = _fwd(name)
    dy = _dev(c["dy"])
    g = _bwd(name, f, dy)
    f0 = _fwd(name, x=x[:1].contiguous(), lens=c["lens"][:1])
    g0 = _bwd(name, f0, dy[:1].contiguous(), lens=c["lens"][:1])
    for k in ("y", "h", "s", "mean", "rstd"):
        assert _same_bits(f0[k], f[k][:1]), k
    assert _same_bits(g0["dx"], g["dx"][:1])


@pytest.mark.parametrize("name", ["tiles_hidden288", "shipped"])
def test_dropout_is_the_oracles_mask_forward_and_backward(name):
    B, Pmax, D, Chid, k1, k2, lens, _ = CASES[name]
    c = _case(name, True)
    p, seed = 0.5, 0x1234ABCD5678
    keep = keep_flat(seed, B * Pmax * D, p).reshape(B, Pmax, D)
    scale = np.float32(drop_scale(p))
    assert scale == np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    plain, dropped = _fwd(name, sparse=True), _fwd(name, drop_p=p, seed=seed, sparse=True)
    xm = np.nan_to_num(c["x"])
    valid = np.broadcast_to(valid_mask(lens, Pmax).numpy()[:, :, None], xm.shape)
    s0, s1 = plain["s"].cpu().numpy(), dropped["s"].cpu().numpy()
    # the kept set: where the branch was dropped s is the residual itself; where it was kept it moved (wherever p = 0 moved it)
    assert np.array_equal((s1 != xm) & valid, keep & (s0 != xm) & valid)
    at0 = (xm == 0) & valid                                            # the residual is an exact zero: s is the branch, bit for bit
    assert at0.sum() > 0.2 * valid.sum()
    assert _same_bits(s1[at0], np.where(keep, s0 * scale, np.float32(0)).astype(np.float32)[at0])
    assert all(_same_bits(dropped[k], plain[k]) for k in ("h", "xm"))
    ref_f = ffn_ref(c["x"], lens, *[c[k] for k in PARAMS], EPS, keep=keep, scale=float(scale))
    errs = {k: rel_l2(dropped[k], ref_f[k]) for k in ("y", "s", "mean", "rstd")}
    gate = _gate_check(name + " (dropout)", dropped["h"], ref_f, lens)
    ref = ffn_bwd_ref(c["dy"], ref_f, lens, c["w1"], c["w2"], c["gamma"], gate, keep=keep, scale=float(scale))
    g = _bwd(name, dropped, _dev(c["dy"]), drop_p=p, seed=seed, sparse=True)
    errs.update({k: rel_l2(g[k], ref[k]) for k in GRADS})
    _report(f"{name} under dropout 0.5: " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert all(v < TOL for v in errs.values()), errs
    assert _behind_are_zero(g["dx"], lens) and _behind_are_zero(dropped["y"], lens)


def test_the_autograd_function_is_the_entry_points_and_eval_ignores_dropout():
    name = "strided"
    B, Pmax, D, Chid, k1, k2, lens, _ = CASES[name]
    c = _case(name)
    x, _, _ = _device_x(name)
    x.requires_grad_(True)
    par = [_dev(c[k]).requires_grad_(True) for k in PARAMS]
    pl = _dev(c["lens"])
    y = ragged_conv_ffn(x, pl, *par, eps=EPS)
    dy = _dev(c["dy"])
    y.backward(dy)
    f = _fwd(name)
    g = _bwd(name, f, dy)
    assert _same_bits(y, f["y"]) and x.grad.shape == x.shape
    for t, k in zip([x] + par, GRADS):
        assert _same_bits(t.grad, g[k]), k
    with torch.no_grad():
        assert _same_bits(ragged_conv_ffn(x, pl, *par, eps=EPS, drop_p=0.5, seed=77, training=False), f["y"])
        dropped = ragged_conv_ffn(x, pl, *par, eps=EPS, drop_p=0.5, seed=77)
        assert _same_bits(dropped, _fwd(name, drop_p=0.5, seed=77)["y"]) and not _same_bits(dropped, f["y"])
    m = ConvFeedForward(D, Chid, kernel_sizes=(k1, k2), dropout=0.5).to(DEV)
    with torch.no_grad():
        for t, k in zip((m.w_1.weight, m.w_1.bias, m.w_2.weight, m.w_2.bias, m.layer_norm.weight, m.layer_norm.bias), PARAMS):
            t.copy_(_dev(c[k]))
        assert _same_bits(m.eval()(x, pl), f["y"])
        a, b = m.train()(x, pl), m(x, pl)
        assert not _same_bits(a, b)                                   # a fresh seed per call


# ------------------------------------------------------------------------------------------------ the block, the student
def _held_to_stock(tag, kernel, stock, ref):
    """the rule of tests/test_hip_model.py: below twice the stock fp32 path's error against the same fp64, and below 1e-4"""
    bad = {}
    for k in ref:
        e, e32 = rel_l2(kernel[k], ref[k]), rel_l2(stock[k], ref[k])
        _report(f"{tag} {k}: kernels {e:.3e} stock fp32 {e32:.3e}")
        if not (e < 2.0 * e32 and e < 1e-4):
            bad[k] = (e, e32)
    assert not bad, bad


def _grads_of(out_of, leaves, weights):
    """sum(out * weights) differentiated by the leaves"""
    return torch.autograd.grad((out_of * weights).sum(), leaves)


BLOCKS = {"d64_hidden288": (3, 70, 64, 2, 288, (70, 12, 1)), "shipped": (2, 40, 256, 2, 1024, (40, 33))}


@pytest.mark.parametrize("name", list(BLOCKS))
def test_the_fft_block_against_fp64_and_the_stock_fp32_path(name):
    B, Pmax, D, H, Chid, lens = BLOCKS[name]
    torch.manual_seed(sum(map(ord, name)))
    m = FFTBlock(D, H, Chid, (9, 1), dropout=0.2).eval()
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.05 * torch.randn_like(p))
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    assert tuple(sd) == BLOCK_PARAMS
    x = torch.randn(B, Pmax, D)                                       # finite everywhere: the attention half's contract
    dy = torch.from_numpy(poison(lens, torch.randn(B, Pmax, D).numpy()))
    w = torch.nan_to_num(dy)
    res = {}
    for tag, dtype, dev in (("ref", torch.float64, "cpu"), ("stock", torch.float32, DEV)):
        p = {k: v.to(dev, dtype).requires_grad_(True) for k, v in sd.items()}
        xr = x.to(dev, dtype).requires_grad_(True)
        out = fft_block_ref(xr, lens, p, H)
        gr = _grads_of(out, [xr] + list(p.values()), w.to(dev, dtype))
        res[tag] = dict(out=out.detach(), dx=gr[0], **dict(zip(p, gr[1:])))
    m = m.to(DEV)
    xk, pl = x.to(DEV).requires_grad_(True), torch.tensor(lens, device=DEV)
    out = m(xk, pl)
    out.backward(dy.to(DEV))
    assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(xk.grad).any())
    assert _behind_are_zero(out, lens) and _behind_are_zero(xk.grad, lens)
    kernel = dict(out=out.detach(), dx=xk.grad, **{k: p.grad for k, p in m.named_parameters()})
    _held_to_stock(f"FFTBlock {name}", kernel, res["stock"], res["ref"])


STUDENT = dict(n_vocab=20, d_model=64, encoder_layers=2, decoder_layers=2, n_head=2, d_hidden=96, n_mels=16)
STUDENT_LENS, STUDENT_PMAX, STUDENT_TMAX = (12, 7, 3), 12, 48


def _student():
    from transformertts_amd import KernelVariancePredictor
    torch.manual_seed(23)
    m = FastSpeech2Student(**STUDENT, predictor=lambda d: KernelVariancePredictor(d, hidden=96), n_bins=8,
                           min_duration=1).eval()
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return m


def _student_loss(out, mel_target, dur, pitch, energy, lens, mel_lens):
    """VarianceLoss's three masked means (weights 1, 0.5, 2) + a masked L1 on the mel, in out's dtype"""
    P, T = dur.shape[1], mel_target.shape[1]
    dev = out["melspec"].device
    v = torch.arange(P, device=dev)[None, :] < torch.as_tensor(lens, device=dev)[:, None]
    vm = (torch.arange(T, device=dev)[None, :] < mel_lens.to(dev)[:, None])[:, :, None]
    dt = out["melspec"].dtype
    n = v.sum().to(dt)
    terms = [(torch.where(v, out[k] - t.to(dt), out[k].new_zeros(())) ** 2).sum() / n
             for k, t in (("log_duration", torch.log(dur.to(dt) + 1)), ("pitch", pitch), ("energy", energy))]
    l1 = torch.where(vm, (out["melspec"] - mel_target.to(dt)).abs(), out["melspec"].new_zeros(())).sum() / (vm.sum().to(dt) * mel_target.shape[2])
    return (terms[0] + 0.5 * terms[1]) + 2.0 * terms[2] + l1


def test_the_student_with_targets_against_fp64_and_the_stock_fp32_path():
    from transformertts_amd import VarianceLoss
    m = _student()
    B, P, T = len(STUDENT_LENS), STUDENT_PMAX, STUDENT_TMAX
    rng = np.random.default_rng(8)
    phoneme = torch.from_numpy(rng.integers(1, STUDENT["n_vocab"], (B, P)))
    dur = torch.from_numpy(rng.integers(1, 5, (B, P)))
    pitch = torch.from_numpy(rng.uniform(70, 500, (B, P)).astype(np.float32))
    energy = torch.from_numpy(rng.uniform(0, 1, (B, P)).astype(np.float32))
    mel_target = torch.from_numpy(rng.standard_normal((B, T, STUDENT["n_mels"])).astype(np.float32))
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    names = [k for k, _ in m.named_parameters()]
    keys = ("melspec", "log_duration", "pitch", "energy")
    res = {}
    for tag, dtype, dev in (("ref", torch.float64, "cpu"), ("stock", torch.float32, DEV)):
        p = {k: (v.to(dev, dtype) if v.is_floating_point() else v.to(dev)) for k, v in sd.items()}
        for k in names:
            p[k].requires_grad_(True)
        out = student_ref(p, STUDENT, phoneme.to(dev), STUDENT_LENS, dur.to(dev), pitch.to(dev), energy.to(dev), T)
        loss = _student_loss(out, mel_target.to(dev), dur.to(dev), pitch.to(dev), energy.to(dev), STUDENT_LENS, out["mel_lens"])
        gr = torch.autograd.grad(loss, [p[k] for k in names])
        res[tag] = dict({k: out[k].detach() for k in keys}, **dict(zip(names, gr)))
        mel_lens_ref = out["mel_lens"].cpu()
    m = m.to(DEV)
    pl = torch.tensor(STUDENT_LENS, device=DEV)
    # NaN behind the lengths of the targets (the durations: a NaN's bits): nothing there is read
    durk, pitchk, energyk = dur.clone(), pitch.clone(), energy.clone()
    for b, n in enumerate(STUDENT_LENS):
        durk[b, n:], pitchk[b, n:], energyk[b, n:] = 0x7FF8000000000000, float("nan"), float("nan")
    out = m(phoneme.to(DEV), pl, durations=durk.to(DEV), pitch=pitchk.to(DEV), energy=energyk.to(DEV), max_len=T)
    assert torch.equal(out["mel_lens"].cpu(), mel_lens_ref)
    var = VarianceLoss((1.0, 0.5, 2.0))(out, durk.to(DEV), pitchk.to(DEV), energyk.to(DEV), pl)["total"]
    vm = (torch.arange(T, device=DEV)[None, :] < out["mel_lens"][:, None])[:, :, None]
    l1 = torch.where(vm, (out["melspec"] - mel_target.to(DEV)).abs(), torch.zeros((), device=DEV)).sum() / (vm.sum() * STUDENT["n_mels"])
    (var + l1).backward()
    assert _behind_are_zero(out["melspec"], out["mel_lens"].tolist()) and not bool(torch.isnan(out["melspec"]).any())
    assert int(out["mel_lens"].min()) >= 1 and int(out["mel_lens"].max()) <= T
    kernel = dict({k: out[k].detach() for k in keys}, **{k: q.grad for k, q in m.named_parameters()})
    assert all(v is not None for v in kernel.values())
    _held_to_stock("student", kernel, res["stock"], res["ref"])


def test_a_captured_eval_call_of_the_student_replayed_on_another_input():
    m = _student().to(DEV)
    B, P, T = len(STUDENT_LENS), STUDENT_PMAX, STUDENT_TMAX
    rng = np.random.default_rng(9)
    ids = [torch.from_numpy(rng.integers(1, STUDENT["n_vocab"], (B, P))).to(DEV) for _ in range(2)]
    static, pl = ids[0].clone(), torch.tensor(STUDENT_LENS, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():                    # (warm-up: the library is loaded, the allocator primed)
        m(static, pl, max_len=T)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        got = m(static, pl, max_len=T)
    seen = []
    for x in ids:
        static.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        with torch.no_grad():
            eager = m(x.clone(), pl, max_len=T)
        assert _same_bits(got["melspec"], eager["melspec"]) and torch.equal(got["mel_lens"], eager["mel_lens"])
        assert not bool(torch.isnan(got["melspec"]).any()) and _behind_are_zero(got["melspec"], got["mel_lens"].tolist())
        seen.append(got["melspec"].clone())
    assert not torch.equal(seen[0], seen[1])                          # the replay did follow the input
