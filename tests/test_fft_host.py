"""The conv feed-forward sublayer, the FFT block and the FastSpeech-2 student (csrc/predictor.hip, transformertts_amd/fft.py), host
side: the fp64 oracle of tests/fft_reference.py against a plain stock-torch chain, its backward against autograd, the adjoint
identity by central differences; every refusal of the new entry points and of the Python checks with its message, before any
launch; the header, the bindings, the exports and the source scan; the `state_dict` layouts.  No GPU."""
import os
import re
import types

import numpy as np
import pytest
import torch
from torch import nn

from fft_reference import BLOCK_PARAMS, ffn_bwd_ref, ffn_ref, fft_block_ref, poison, valid_mask
from transformertts_amd import _lib
from transformertts_amd.fft import ConvFeedForward, FastSpeech2Student, FFTBlock, FFTStack, ragged_conv_ffn  # noqa: F401 -- no feature, no tests

_lib.load()                                                           # raises when the library lacks the entries

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ttts_ragged_conv_ffn_fwd", "ttts_ragged_conv_ffn_workspace_bytes", "ttts_ragged_conv_ffn_bwd")
EXPORTS = ("ragged_conv_ffn", "ConvFeedForward", "FFTBlock", "FFTStack", "FastSpeech2Student")
NAMES = ("x", "w1", "b1", "w2", "b2", "gamma", "beta")
GRADS = ("dx", "dw1", "db1", "dw2", "db2", "dgamma", "dbeta")


def test_the_header_declares_each_entry_point_once_and_the_exports_agree():
    from transformertts_amd import fft, predictor
    import transformertts_amd
    lib = _lib.load()
    hdr = open(os.path.join(REPO, "include", "ttts_hip.h")).read()
    for name in NEW:
        decls = re.findall(r"^(?:int|size_t) " + name + r"\s*\(([^;]*)\)\s*;", hdr, re.M)
        assert len(decls) == 1, f"{name} must be declared exactly once in ttts_hip.h, found {len(decls)}"
        assert name in _lib.SIGNATURES and hasattr(lib, name), f"{name} is not exported / bound"
        assert len(decls[0].split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert lib.ttts_abi_version() == 24                               # additive
    for name in EXPORTS:
        assert getattr(transformertts_amd, name) is getattr(fft, name) and name in transformertts_amd.__all__
    assert tuple(fft.__all__) == EXPORTS
    assert tuple(predictor.__all__) == ("ragged_conv_norm", "RaggedConvNorm", "KernelVariancePredictor")
    src = open(os.path.join(REPO, "transformertts_amd", "csrc", "predictor.hip")).read()
    assert all(("int " if "bytes" not in name else "size_t ") + name + "(" in src for name in NEW)     # the file that holds the kernels
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert "atomic" not in code.replace("__ATOMIC_", "") and "hipMalloc" not in code and "hipMemcpy" not in code
    assert "getenv" not in code and "hipDeviceSynchronize" not in code and "hipStreamSynchronize" not in code
    for const, value in (("RC_MAX_P", fft.MAX_ROWS), ("RC_MAX_CIN", fft.MAX_HIDDEN), ("RC_COLS", fft.MAX_D), ("RC_MAX_TAPS", fft.MAX_TAPS)):
        assert re.search(const + r" = (\d+)", src).group(1) == str(value)
    assert lib.ttts_ragged_conv_ffn_workspace_bytes(0, 10, 32, 64, 3, 1) == 0
    assert lib.ttts_ragged_conv_ffn_workspace_bytes(2, 10, 32, 64, 3, 0) == 0
    # ds, dz2, dz1, one flipped weight, the row kernel's partials
    assert lib.ttts_ragged_conv_ffn_workspace_bytes(2, 10, 32, 64, 3, 1) >= 4 * (2 * 2 * 10 * 32 + 2 * 10 * 64 + 32 * 64 * 3 + 2 * 2 * 32)


# ------------------------------------------------------------------------------------------------ the oracle
def _inputs(seed, B, Pmax, D, Chid, k1, k2, lens):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, Pmax, D))
    w1, b1 = rng.standard_normal((Chid, D, k1)) / np.sqrt(D * k1), 0.3 * rng.standard_normal(Chid)
    w2, b2 = rng.standard_normal((D, Chid, k2)) / np.sqrt(Chid * k2), 0.3 * rng.standard_normal(D)
    gamma, beta = 1 + 0.2 * rng.standard_normal(D), 0.2 * rng.standard_normal(D)
    dy = rng.standard_normal((B, Pmax, D))
    return [poison(lens, x), w1, b1, w2, b2, gamma, beta], poison(lens, dy)


@pytest.mark.parametrize("k1,k2", [(9, 1), (3, 3), (1, 1)])
def test_the_oracle_is_the_stock_chain_in_fp64(k1, k2):
    B, Pmax, D, Chid, lens = 3, 14, 32, 64, (14, 5, 0)
    (x, w1, b1, w2, b2, gamma, beta), _ = _inputs(k1 + k2, B, Pmax, D, Chid, k1, k2, lens)
    c1, c2, ln = nn.Conv1d(D, Chid, k1, padding=k1 // 2).double(), nn.Conv1d(Chid, D, k2, padding=k2 // 2).double(), nn.LayerNorm(D).double()
    with torch.no_grad():
        for t, v in ((c1.weight, w1), (c1.bias, b1), (c2.weight, w2), (c2.bias, b2), (ln.weight, gamma), (ln.bias, beta)):
            t.copy_(torch.from_numpy(v))
        pad = ~valid_mask(lens, Pmax)[:, :, None]
        xm = torch.from_numpy(x).masked_fill(pad, 0.0)
        h = torch.relu(c1(xm.transpose(1, 2)).transpose(1, 2)).masked_fill(pad, 0.0)
        z = nn.functional.dropout(c2(h.transpose(1, 2)).transpose(1, 2), 0.5, training=False)
        want = ln(xm + z).masked_fill(pad, 0.0)
    got = ffn_ref(x, lens, w1, b1, w2, b2, gamma, beta, ln.eps)
    assert not torch.isnan(got["y"]).any() and (got["y"] - want).abs().max().item() <= 1e-12 * max(want.abs().max().item(), 1.0)
    assert (got["h"] - h).abs().max().item() <= 1e-12
    assert all((got[k][b, n:] == 0).all() for k in ("y", "h", "s", "mean", "rstd", "xm") for b, n in enumerate(lens))


def _fixture(k1, k2, lens):
    """inputs whose hidden pre-activations stay at least 1e-5 from the kink: the first seed, from 10 on, that does"""
    B, Pmax, D, Chid = len(lens), 12, 32, 64
    for seed in range(10, 30):
        inputs, dy = _inputs(seed, B, Pmax, D, Chid, k1, k2, lens)
        fwd = ffn_ref(*inputs[:1], lens, *inputs[1:])
        valid = valid_mask(lens, Pmax)[:, :, None].expand_as(fwd["z1"])
        if fwd["z1"].abs()[valid].min().item() >= 1e-5:
            return inputs, dy, fwd
    raise AssertionError("no seed keeps the pre-activations away from the kink")


@pytest.mark.parametrize("k1,k2,lens", [(9, 1, (12, 5, 0)), (3, 3, (12, 3, 1)), (1, 1, (12, 12, 7))])
def test_the_backward_oracle_against_autograd_and_the_adjoint_identity(k1, k2, lens):
    Pmax = 12
    inputs, dy, fwd = _fixture(k1, k2, lens)
    valid = valid_mask(lens, Pmax)[:, :, None]
    assert fwd["z1"].abs()[valid.expand_as(fwd["z1"])].min().item() >= 1e-5      # the property the differences below rest on
    bwd = ffn_bwd_ref(dy, fwd, lens, inputs[1], inputs[3], inputs[5], fwd["z1"] > 0)
    leaves = [torch.from_numpy(np.nan_to_num(v)).requires_grad_(True) for v in inputs]
    y = ffn_ref(leaves[0], lens, *leaves[1:])["y"]
    g = torch.where(valid, torch.from_numpy(dy), torch.zeros((), dtype=torch.float64))
    auto = torch.autograd.grad(y, leaves, g)
    for name, a in zip(GRADS, auto):
        assert (bwd[name] - a).abs().max().item() <= 1e-11 * max(a.abs().max().item(), 1.0), name
    assert all((bwd["dx"][b, n:] == 0).all() for b, n in enumerate(lens)) and not torch.isnan(bwd["dx"]).any()
    # <ffn'(v) dv, dy> = <dv, ffn'^T dy> with ffn'(v) dv from central differences over x and all six parameters
    rng = np.random.default_rng(99)
    dirs = [rng.standard_normal(v.shape) for v in inputs]
    step = 1e-6
    base = [np.nan_to_num(v) for v in inputs]
    yp = ffn_ref(base[0] + step * dirs[0], lens, *[b + step * d for b, d in zip(base[1:], dirs[1:])])["y"]
    ym = ffn_ref(base[0] - step * dirs[0], lens, *[b - step * d for b, d in zip(base[1:], dirs[1:])])["y"]
    lhs = (((yp - ym) / (2 * step)) * g).sum().item()
    rhs = sum((torch.from_numpy(d) * bwd[n]).sum().item() for d, n in zip(dirs, GRADS))
    assert abs(lhs - rhs) <= 1e-6 * max(abs(rhs), 1.0), (lhs, rhs)


def test_the_dropout_of_the_oracle_sits_on_the_branch():
    from oracle.dropmask import drop_scale, keep_flat
    lens = (6, 2)
    inputs, _ = _inputs(3, 2, 6, 32, 64, 3, 1, lens)
    keep = keep_flat(1234, 2 * 6 * 32, 0.5).reshape(2, 6, 32)
    a, b = ffn_ref(inputs[0], lens, *inputs[1:]), ffn_ref(inputs[0], lens, *inputs[1:], keep=keep, scale=drop_scale(0.5))
    branch = a["s"] - a["xm"]
    assert torch.allclose(b["s"], a["xm"] + branch * torch.from_numpy(keep) * 2.0, rtol=0, atol=1e-14) and 0.3 < keep.mean() < 0.7
    assert torch.equal(b["h"], a["h"])


def test_the_block_oracle_ignores_what_stands_behind_a_length():
    torch.manual_seed(1)
    m = FFTBlock(32, 2, 64, (3, 1)).double().eval()
    sd = dict(m.state_dict())
    lens = (9, 4)
    x = torch.randn(2, 9, 32, dtype=torch.float64)
    a = fft_block_ref(x, lens, sd, 2)
    x2 = x.clone()
    x2[1, 4:] = 7.0
    b = fft_block_ref(x2, lens, sd, 2)
    assert torch.allclose(a, b, rtol=0, atol=1e-12) and bool((a[1, 4:] == 0).all())


# ------------------------------------------------------------------------------------------------ state_dict layouts
def test_the_state_dicts_carry_the_usual_names_and_shapes():
    m = ConvFeedForward(64, 96, (9, 1), 0.1)
    assert {n: tuple(v.shape) for n, v in m.state_dict().items()} == {
        "w_1.weight": (96, 64, 9), "w_1.bias": (96,), "w_2.weight": (64, 96, 1), "w_2.bias": (64,), "layer_norm.weight": (64,),
        "layer_norm.bias": (64,)}
    blk = FFTBlock(64, 2, 96, (9, 1), 0.1)
    assert tuple(blk.state_dict()) == BLOCK_PARAMS
    assert [tuple(v.shape) for v in blk.state_dict().values()] == [(192, 64), (192,), (64, 64), (64,), (64,), (64,), (96, 64, 9), (96,),
                                                                   (64, 96, 1), (64,), (64,), (64,)]
    stack = FFTStack(2, 64, 2, 96, max_len=50)
    assert list(stack.state_dict()) == [f"layers.{i}.{k}" for i in range(2) for k in BLOCK_PARAMS]      # the table is no parameter
    assert tuple(stack.pe.shape) == (50, 64) and float(stack.alpha) == 1.0
    assert stack.pe[0, 0] == 0 and stack.pe[0, 1] == 1 and abs(float(stack.pe[1, 0]) - np.sin(1.0)) < 1e-7
    from transformertts_amd import KernelVariancePredictor
    from predictor_reference import PARAMS as PREDICTOR
    s = FastSpeech2Student(20, d_model=64, encoder_layers=1, decoder_layers=2, n_head=2, d_hidden=96, n_mels=16,
                           predictor=lambda d: KernelVariancePredictor(d, hidden=96), n_bins=8)
    want = ["embedding.weight"] + [f"encoder.layers.0.{k}" for k in BLOCK_PARAMS]
    want += [f"adaptor.{p}_predictor.{k}" for p in ("duration", "pitch", "energy") for k in PREDICTOR]
    want += ["adaptor.embedding.pitch_bins", "adaptor.embedding.energy_bins", "adaptor.embedding.pitch_table", "adaptor.embedding.energy_table"]
    want += [f"decoder.layers.{i}.{k}" for i in range(2) for k in BLOCK_PARAMS] + ["mel_linear.weight", "mel_linear.bias"]
    sd = s.state_dict()
    assert sorted(sd) == sorted(want)
    assert tuple(sd["embedding.weight"].shape) == (20, 64) and tuple(sd["mel_linear.weight"].shape) == (16, 64)
    assert tuple(sd["adaptor.duration_predictor.conv1.weight"].shape) == (96, 64, 3)
    assert tuple(sd["adaptor.embedding.pitch_table"].shape) == (8, 64) and tuple(sd["decoder.layers.1.ffn.w_1.weight"].shape) == (96, 64, 9)
    assert isinstance(FastSpeech2Student(20, d_model=32, encoder_layers=1, decoder_layers=1, d_hidden=32, n_bins=4).adaptor.duration_predictor,
                      KernelVariancePredictor)


# ------------------------------------------------------------------------------------------------ refusals of the C entries
def _call(lib, entry, order, pointers, defaults, kw):
    """an entry point on a host buffer: every case below is refused before a launch, so nothing dereferences it.  A pointer
    argument is None or a byte offset into the buffer."""
    buf = np.zeros(64, dtype=np.int64)
    a = dict(defaults)
    a.update(kw)
    for name in pointers:
        a[name] = None if a[name] is None else buf.ctypes.data + a[name]
    return getattr(lib, entry)(*[a[k] for k in order], None)


FWD_PTRS = ("x", "lens", "w1", "b1", "w2", "b2", "gamma", "beta", "step_seed", "h", "y", "s", "mean", "rstd", "x_masked")
FWD = dict(order=("x", "ld_row", "ld_batch", "lens", "w1", "b1", "w2", "b2", "gamma", "beta", "B", "Pmax", "D", "Chid", "k1", "k2", "eps",
                  "drop_p", "seed", "step_seed", "h", "y", "s", "mean", "rstd", "x_masked"),
           pointers=FWD_PTRS,
           defaults=dict(dict.fromkeys(FWD_PTRS, 0), ld_row=32, ld_batch=320, B=2, Pmax=10, D=32, Chid=64, k1=3, k2=1, eps=1e-5, drop_p=0.0,
                         seed=0, step_seed=None))
BWD_PTRS = ("dy", "s", "mean", "rstd", "h", "x_masked", "lens", "w1", "w2", "gamma", "step_seed", "dx", "dw1", "db1", "dw2", "db2", "dgamma",
            "dbeta", "ws")
BWD = dict(order=("dy", "s", "mean", "rstd", "h", "x_masked", "lens", "w1", "w2", "gamma", "B", "Pmax", "D", "Chid", "k1", "k2", "drop_p", "seed",
                  "step_seed", "dx", "dw1", "db1", "dw2", "db2", "dgamma", "dbeta", "ws", "ws_bytes", "accumulate"),
           pointers=BWD_PTRS,
           defaults=dict(dict.fromkeys(BWD_PTRS, 0), B=2, Pmax=10, D=32, Chid=64, k1=3, k2=1, drop_p=0.0, seed=0, step_seed=None,
                         ws_bytes=1 << 30, accumulate=0))
SHAPE = [(dict(B=0), "B must be in [1, 65535] (one grid row per utterance), got 0"), (dict(B=65536), "got 65536"),
         (dict(Pmax=0), "Pmax must be in [1, 4096] rows, got 0"), (dict(Pmax=4097), "Pmax must be in [1, 4096] rows, got 4097"),
         (dict(D=0), "D must be a multiple of 32 in [32, 256], got 0"), (dict(D=48, ld_row=48), "D must be a multiple of 32 in [32, 256], got 48"),
         (dict(D=288, ld_row=288), "D must be a multiple of 32 in [32, 256], got 288"),
         (dict(Chid=0), "Chid must be a multiple of 32 in [32, 1024], got 0"), (dict(Chid=80), "Chid must be a multiple of 32 in [32, 1024], got 80"),
         (dict(Chid=1056), "got 1056"),
         (dict(k1=0), "k1 must be odd in [1, 9], got 0"), (dict(k1=4), "k1 must be odd in [1, 9], got 4"), (dict(k1=11), "k1 must be odd in [1, 9], got 11"),
         (dict(k2=0), "k2 must be odd in [1, 9], got 0"), (dict(k2=2), "k2 must be odd in [1, 9], got 2"), (dict(k2=11), "k2 must be odd in [1, 9], got 11"),
         (dict(drop_p=1.0), "drop_p must be in [0, 1), got 1"), (dict(drop_p=-0.5), "drop_p must be in [0, 1), got -0.5"),
         (dict(drop_p=float("nan")), "drop_p must be in [0, 1), got nan")]
REFUSALS = (
    [("ttts_ragged_conv_ffn_fwd", FWD, kw, needle) for kw, needle in
     [(dict([(n, None)]), "null pointer") for n in ("x", "lens", "w1", "b1", "w2", "b2", "gamma", "beta", "h", "y")] + SHAPE + [
        (dict(s=None), "null pointer (s, mean and rstd go together: all three or none)"), (dict(mean=None), "all three or none"),
        (dict(rstd=None, s=None), "all three or none"),
        (dict(eps=0.0), "eps must be positive and finite, got 0"), (dict(eps=-1.0), "eps must be positive and finite, got -1"),
        (dict(eps=float("inf")), "eps must be positive and finite, got inf"), (dict(eps=float("nan")), "got nan"),
        (dict(ld_row=28), "the row stride must be a multiple of 4 and >= D (ld_row 28, D 32)"),
        (dict(ld_row=34), "the row stride must be a multiple of 4 and >= D (ld_row 34, D 32)"),
        (dict(ld_batch=316), "the batch stride must be a multiple of 4 and cover an utterance (ld_batch 316, ld_row 32, Pmax 10, D 32)"),
        (dict(ld_batch=322), "the batch stride must be a multiple of 4 and cover an utterance (ld_batch 322"),
        (dict(B=1, ld_batch=-4), "the batch stride"),
        (dict(x=8), "x, w1, w2, h, y, s and x_masked must be 16-byte aligned"), (dict(w1=4), "16-byte aligned"), (dict(w2=8), "16-byte aligned"),
        (dict(h=8), "16-byte aligned"), (dict(y=8), "16-byte aligned"), (dict(s=8), "16-byte aligned"), (dict(x_masked=4), "16-byte aligned"),
        (dict(b1=2), "b1, b2, gamma, beta, mean and rstd must be 4-byte aligned"), (dict(b2=2), "4-byte aligned"), (dict(gamma=1), "4-byte aligned"),
        (dict(beta=3), "4-byte aligned"), (dict(mean=2), "4-byte aligned"), (dict(rstd=2), "4-byte aligned"),
        (dict(lens=4), "lens and step_seed must be 8-byte aligned"), (dict(step_seed=4), "8-byte aligned")]] +
    [("ttts_ragged_conv_ffn_bwd", BWD, kw, needle) for kw, needle in
     [(dict([(n, None)]), "null pointer") for n in ("dy", "s", "mean", "rstd", "h", "lens", "w1", "w2", "gamma", "dgamma", "dbeta", "ws")] + SHAPE + [
        (dict(dw1=None), "null pointer (dw1, db1, dw2 and db2 go together: all four or none)"), (dict(db1=None), "all four or none"),
        (dict(dw2=None, db2=None), "all four or none"), (dict(dw1=None, db1=None, dw2=None), "all four or none"),
        (dict(x_masked=None), "null pointer (the weight gradient needs x_masked)"),
        (dict(B=40000, Pmax=4096, Chid=1024), "the weight gradient takes operands below 4 GiB (B 40000, Pmax 4096, D 32, Chid 1024)"),
        (dict(dy=8), "dy, s, h, x_masked, w1, w2, dx, dw1, dw2 and ws must be 16-byte aligned"), (dict(s=4), "16-byte aligned"),
        (dict(h=8), "16-byte aligned"), (dict(x_masked=8), "16-byte aligned"), (dict(w1=8), "16-byte aligned"), (dict(w2=4), "16-byte aligned"),
        (dict(dx=8), "16-byte aligned"), (dict(dw1=4), "16-byte aligned"), (dict(dw2=8), "16-byte aligned"), (dict(ws=8), "16-byte aligned"),
        (dict(mean=2), "mean, rstd, gamma, db1, db2, dgamma and dbeta must be 4-byte aligned"), (dict(rstd=1), "4-byte aligned"),
        (dict(gamma=2), "4-byte aligned"), (dict(db1=2), "4-byte aligned"), (dict(db2=2), "4-byte aligned"), (dict(dgamma=3), "4-byte aligned"),
        (dict(dbeta=2), "4-byte aligned"),
        (dict(lens=4), "lens and step_seed must be 8-byte aligned"), (dict(step_seed=12), "8-byte aligned"),
        (dict(ws_bytes=64), "workspace too small (64 bytes, need ")]])


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_every_refusal_names_its_value_before_any_launch(case):
    lib = _lib.load()
    entry, spec, kw, needle = REFUSALS[case]
    rc = _call(lib, entry, spec["order"], spec["pointers"], spec["defaults"], kw)
    assert rc != 0 and needle in _lib.last_error() and entry[5:] in _lib.last_error(), (entry, kw, _lib.last_error())
    with pytest.raises(RuntimeError, match=re.escape(needle)):       # ... and reaches Python through _lib.check
        _lib.check(rc, entry)


# ------------------------------------------------------------------------------------------------ refusals of the Python checks
def _cuda(shape, dtype=torch.float32, **kw):
    """what the checks read of a device tensor, on the CPU: those in front of the launch can be reached without a device"""
    strides = tuple(int(np.prod(shape[i + 1:])) for i in range(len(shape)))
    d = dict(shape=tuple(shape), dim=lambda: len(shape), is_cuda=True, dtype=dtype, device=torch.device("cpu"), stride=lambda i: strides[i],
             data_ptr=lambda: 0, size=lambda i: shape[i], contiguous=lambda: None)
    d.update(kw)
    return types.SimpleNamespace(**d)


def test_ragged_conv_ffn_refuses():
    pl = torch.tensor([12, 3, 1])
    x = _cuda((3, 12, 32))
    w1, b1, w2, v = _cuda((64, 32, 3)), _cuda((64,)), _cuda((32, 64, 1)), _cuda((32,))
    fn = "ragged_conv_ffn"
    for args, kw, needle in (
            ((torch.zeros(3, 12), pl, w1, b1, w2, v, v, v), {}, "x must be (B, Pmax, D), got (3, 12)"),
            ((torch.zeros(3, 12, 32), pl, w1, b1, w2, v, v, v), {}, f"{fn}.x: expected a CUDA/HIP tensor (the HIP path has no CPU fallback), got cpu"),
            ((_cuda((3, 12, 32), dtype=torch.float64), pl, w1, b1, w2, v, v, v), {}, f"{fn}.x: expected dtype torch.float32, got torch.float64"),
            ((_cuda((3, 12, 36)), pl, w1, b1, w2, v, v, v), {}, "D must be a multiple of 32 in [32, 256], got 36"),
            ((_cuda((3, 12, 288)), pl, w1, b1, w2, v, v, v), {}, "D must be a multiple of 32 in [32, 256], got 288"),
            ((_cuda((3, 4097, 32)), pl, w1, b1, w2, v, v, v), {}, "Pmax must be in [1, 4096] rows, got 4097"),
            ((_cuda((65536, 2, 32)), pl, w1, b1, w2, v, v, v), {}, "B must be in [1, 65535], got 65536"),
            ((x, torch.tensor([12, 3]), w1, b1, w2, v, v, v), {}, f"{fn}.lens must have shape (3,), got (2,)"),
            ((x, torch.tensor([12.0, 3.0, 1.0]), w1, b1, w2, v, v, v), {}, f"{fn}.lens must be integers, got torch.float32"),
            ((x, pl, _cuda((64, 16, 3)), b1, w2, v, v, v), {}, "w1 must be (Chid, 32, k1), got (64, 16, 3)"),
            ((x, pl, _cuda((80, 32, 3)), b1, w2, v, v, v), {}, "Chid must be a multiple of 32 in [32, 1024], got 80"),
            ((x, pl, _cuda((1056, 32, 3)), b1, w2, v, v, v), {}, "Chid must be a multiple of 32 in [32, 1024], got 1056"),
            ((x, pl, w1, b1, _cuda((32, 96, 1)), v, v, v), {}, "w2 must be (32, 64, k2), got (32, 96, 1)"),
            ((x, pl, w1, b1, _cuda((64, 64, 1)), v, v, v), {}, "w2 must be (32, 64, k2), got (64, 64, 1)"),
            ((x, pl, _cuda((64, 32, 4)), b1, w2, v, v, v), {}, "the kernel sizes must be odd in [1, 9], got 4"),
            ((x, pl, w1, b1, _cuda((32, 64, 11)), v, v, v), {}, "the kernel sizes must be odd in [1, 9], got 11"),
            ((x, pl, _cuda((64, 32, 3), dtype=torch.float16), b1, w2, v, v, v), {}, f"{fn}.w1: expected a torch.float32 CUDA/HIP tensor"),
            ((x, pl, w1, _cuda((32,)), w2, v, v, v), {}, "b1 must be (64,), got (32,)"),
            ((x, pl, w1, b1, w2, _cuda((64,)), v, v), {}, "b2 must be (32,), got (64,)"),
            ((x, pl, w1, b1, w2, v, _cuda((31,)), v), {}, "gamma must be (32,), got (31,)"),
            ((x, pl, w1, b1, w2, v, v, torch.zeros(32)), {}, f"{fn}.beta: expected a torch.float32 CUDA/HIP tensor, got torch.float32 on cpu"),
            ((x, pl, w1, b1, w2, v, v, v), dict(eps=0.0), "eps must be positive and finite, got 0.0"),
            ((x, pl, w1, b1, w2, v, v, v), dict(eps=float("nan")), "eps must be positive and finite, got nan"),
            ((x, pl, w1, b1, w2, v, v, v), dict(drop_p=1.0), "drop_p must be in [0, 1), got 1.0"),
            ((x, pl, w1, b1, w2, v, v, v), dict(drop_p=-0.1), "drop_p must be in [0, 1), got -0.1")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            ragged_conv_ffn(*args, **kw)
    for make, needle in ((lambda: ConvFeedForward(64, 96, (4, 1)), "ConvFeedForward: kernel_sizes must be odd in [1, 9], got 4"),
                         (lambda: ConvFeedForward(64, 96, (9, 11)), "ConvFeedForward: kernel_sizes must be odd in [1, 9], got 11"),
                         (lambda: ConvFeedForward(64, 96, (9,)), "ConvFeedForward: kernel_sizes must be two odd sizes, got (9,)"),
                         (lambda: ConvFeedForward(64, 96, dropout=1.0), "ConvFeedForward: drop_p must be in [0, 1), got 1.0"),
                         (lambda: ConvFeedForward(48, 96), "ConvFeedForward: d_model must be a multiple of 32 in [32, 256], got 48"),
                         (lambda: ConvFeedForward(64, 2048), "ConvFeedForward: d_hidden must be a multiple of 32 in [32, 1024], got 2048"),
                         (lambda: FFTBlock(512), "FFTBlock: d_model must be a multiple of 32 in [32, 256], got 512"),
                         (lambda: FFTBlock(64, 2, 100), "FFTBlock: d_hidden must be a multiple of 32 in [32, 1024], got 100"),
                         (lambda: FFTBlock(64, 2, 96, dropout=-1), "FFTBlock: drop_p must be in [0, 1), got -1.0"),
                         (lambda: FFTStack(0, 64, 2, 96), "FFTStack: n_layers must be a positive integer, got 0"),
                         (lambda: FFTStack(1, 64, 2, 96, max_len=5000), "FFTStack: max_len must be an integer in [1, 4096] rows, got 5000"),
                         (lambda: FastSpeech2Student(0), "FastSpeech2Student: n_vocab must be a positive integer, got 0"),
                         (lambda: FastSpeech2Student(10, n_mels=81), "FastSpeech2Student: n_mels must be a positive multiple of 4, got 81"),
                         (lambda: FastSpeech2Student(10, d_model=320), "FastSpeech2Student: d_model must be a multiple of 32 in [32, 256], got 320")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            make()
    stack = FFTStack(1, 32, 2, 32, max_len=8)
    with pytest.raises(ValueError, match=re.escape("FFTStack: x must be (B, Pmax <= 8, d_model), got (2, 9, 32)")):
        stack(torch.zeros(2, 9, 32), torch.tensor([9, 2]))
    s = FastSpeech2Student(10, d_model=32, encoder_layers=1, decoder_layers=1, d_hidden=32, n_bins=4)
    with pytest.raises(ValueError, match=re.escape("FastSpeech2Student: phoneme must be (B, Pmax) int64, got (2, 3) torch.int32")):
        s(torch.zeros(2, 3, dtype=torch.int32), torch.tensor([3, 2]))
