"""The variance predictor on the library's kernels (csrc/predictor.hip, transformertts_amd/predictor.py), host side: the fp64
oracle of tests/predictor_reference.py against the shipped stock `VariancePredictor`, its backward against autograd, the adjoint
identity and finite differences; the `state_dict` interchange; every refusal of the new entry points and of the Python checks
with its message, before any launch; the header, the bindings, the exports and the source scan.  No GPU."""
import os
import re
import types

import numpy as np
import pytest
import torch

from predictor_reference import PARAMS, poison, predictor_grads_ref, predictor_ref, stage_bwd_ref, stage_ref, valid_mask
from transformertts_amd import _lib
from transformertts_amd.predictor import KernelVariancePredictor, RaggedConvNorm, ragged_conv_norm  # noqa: F401 -- no feature, no tests

_lib.load()                                                           # raises when the library lacks the entries of predictor.hip

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ttts_ragged_conv_norm_fwd", "ttts_ragged_conv_norm_workspace_bytes", "ttts_ragged_conv_norm_bwd")
EXPORTS = ("ragged_conv_norm", "RaggedConvNorm", "KernelVariancePredictor")


def test_the_header_declares_each_entry_point_once_and_the_exports_agree():
    from transformertts_amd import _lib, predictor
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
        assert getattr(transformertts_amd, name) is getattr(predictor, name) and name in transformertts_amd.__all__
    assert tuple(predictor.__all__) == EXPORTS
    src = open(os.path.join(REPO, "transformertts_amd", "csrc", "predictor.hip")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert "atomic" not in code.replace("__ATOMIC_", "") and "hipMalloc" not in code and "hipMemcpy" not in code
    assert "getenv" not in code and "hipDeviceSynchronize" not in code and "hipStreamSynchronize" not in code
    for const, value in (("RC_MAX_P", predictor.MAX_PHONEMES), ("RC_MAX_CIN", predictor.MAX_CIN), ("RC_COLS", predictor.MAX_COUT),
                         ("RC_MAX_TAPS", predictor.MAX_TAPS)):
        assert re.search(const + r" = (\d+)", src).group(1) == str(value)
    assert lib.ttts_ragged_conv_norm_workspace_bytes(0, 10, 16, 32, 3) == 0
    assert lib.ttts_ragged_conv_norm_workspace_bytes(2, 10, 16, 32, 3) >= 4 * (2 * 10 * 32 + 16 * 32 * 3 + 2 * 3 * 32)


# ------------------------------------------------------------------------------------------------ the oracle
def _stage_inputs(seed, B, Pmax, Cin, Cout, k, lens):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, Pmax, Cin))
    w = rng.standard_normal((Cout, Cin, k)) / np.sqrt(Cin * k)
    bias, gamma, beta = 0.3 * rng.standard_normal(Cout), 1 + 0.2 * rng.standard_normal(Cout), 0.2 * rng.standard_normal(Cout)
    dy = rng.standard_normal((B, Pmax, Cout))
    return poison(lens, x), w, bias, gamma, beta, poison(lens, dy)


@pytest.mark.parametrize("d_model,hidden,k,B,Pmax,lens", [(36, 96, 3, 3, 20, (20, 7, 0)), (16, 32, 5, 2, 9, (9, 1)), (8, 32, 1, 1, 4, (3,))])
def test_the_oracle_is_the_stock_predictor_in_fp64(d_model, hidden, k, B, Pmax, lens):
    from transformertts_amd.variance import VariancePredictor
    torch.manual_seed(7)
    stock = VariancePredictor(d_model, hidden=hidden, kernel_size=k).double().eval()
    with torch.no_grad():
        for p in stock.parameters():
            p.add_(0.1 * torch.randn_like(p))                         # (LayerNorm's 1 / 0 and the zero biases say little)
    x = torch.from_numpy(poison(lens, np.random.default_rng(1).standard_normal((B, Pmax, d_model))))
    with torch.no_grad():
        want = stock(x, torch.tensor(lens))
    got = predictor_ref(x, lens, {n: v.detach() for n, v in stock.state_dict().items()})
    assert tuple(stock.state_dict()) == PARAMS
    assert not torch.isnan(got).any() and (got - want).abs().max().item() <= 1e-12 * max(want.abs().max().item(), 1.0)
    assert all((got[b, n:] == 0).all() for b, n in enumerate(lens))


@pytest.mark.parametrize("k,lens", [(3, (12, 5, 0)), (9, (12, 3, 1)), (1, (12, 12, 7))])
def test_the_backward_oracle_against_autograd_the_adjoint_identity_and_finite_differences(k, lens):
    B, Pmax, Cin, Cout = 3, 12, 8, 32
    x, w, bias, gamma, beta, dy = _stage_inputs(10 + k, B, Pmax, Cin, Cout, k, lens)
    fwd = stage_ref(x, lens, w, bias, gamma, beta)
    valid = valid_mask(lens, Pmax)[:, :, None]
    zmin = fwd["z"].abs()[valid.expand_as(fwd["z"])].min().item()
    assert zmin > 1e-5, zmin                                          # the pre-activations stay away from the kink
    bwd = stage_bwd_ref(dy, fwd, lens, w, gamma, fwd["z"] > 0)
    # autograd through the differentiable forward
    leaves = [torch.from_numpy(np.nan_to_num(v)).requires_grad_(True) for v in (x, w, bias, gamma, beta)]
    y = stage_ref(leaves[0], lens, *leaves[1:])["y"]
    g = torch.where(valid, torch.from_numpy(dy), torch.zeros((), dtype=torch.float64))
    auto = torch.autograd.grad(y, leaves, g)
    for name, a in zip(("dx", "dw", "dbias", "dgamma", "dbeta"), auto):
        assert (bwd[name] - a).abs().max().item() <= 1e-11 * max(a.abs().max().item(), 1.0), name
    assert all((bwd["dx"][b, n:] == 0).all() for b, n in enumerate(lens)) and not torch.isnan(bwd["dx"]).any()
    # <stage'(v) dv, dy> = <dv, stage'^T dy> with stage'(v) dv from central differences
    rng = np.random.default_rng(99)
    dirs = [rng.standard_normal(v.shape) for v in (x, w, bias, gamma, beta)]
    h = 1e-6
    base = [np.nan_to_num(v) for v in (x, w, bias, gamma, beta)]
    yp = stage_ref(*[base[0] + h * dirs[0]], lens, *[b + h * d for b, d in zip(base[1:], dirs[1:])])["y"]
    ym = stage_ref(*[base[0] - h * dirs[0]], lens, *[b - h * d for b, d in zip(base[1:], dirs[1:])])["y"]
    lhs = (((yp - ym) / (2 * h)) * g).sum().item()
    rhs = sum((torch.from_numpy(d) * bwd[n]).sum().item() for d, n in zip(dirs, ("dx", "dw", "dbias", "dgamma", "dbeta")))
    assert abs(lhs - rhs) <= 1e-6 * max(abs(rhs), 1.0), (lhs, rhs)


def test_the_dropout_of_the_oracle_is_the_mask_times_the_fp32_scale():
    from oracle.dropmask import drop_scale, keep_flat
    lens = (6, 2)
    x, w, bias, gamma, beta, _ = _stage_inputs(3, 2, 6, 8, 32, 3, lens)
    keep = keep_flat(1234, 2 * 6 * 32, 0.5).reshape(2, 6, 32)
    a, b = stage_ref(x, lens, w, bias, gamma, beta), stage_ref(x, lens, w, bias, gamma, beta, keep=keep, scale=drop_scale(0.5))
    assert torch.equal(b["y"], a["y"] * torch.from_numpy(keep) * 2.0) and 0.3 < keep.mean() < 0.7


def test_state_dicts_load_either_way_with_strict():
    from transformertts_amd.predictor import KernelVariancePredictor, RaggedConvNorm
    from transformertts_amd.variance import VariancePredictor
    torch.manual_seed(0)
    for kw in (dict(d_model=36, hidden=96, kernel_size=3), dict(d_model=256, hidden=256, kernel_size=5)):
        ours, stock = KernelVariancePredictor(**kw), VariancePredictor(**kw)
        assert list(ours.state_dict()) == list(stock.state_dict()) == list(PARAMS)
        assert [tuple(v.shape) for v in ours.state_dict().values()] == [tuple(v.shape) for v in stock.state_dict().values()]
        ours.load_state_dict(stock.state_dict(), strict=True)
        assert all(torch.equal(a, b) for a, b in zip(ours.state_dict().values(), stock.state_dict().values()))
        fresh = KernelVariancePredictor(**kw)
        stock.load_state_dict(fresh.state_dict(), strict=True)
        assert all(torch.equal(a, b) for a, b in zip(fresh.state_dict().values(), stock.state_dict().values()))
    m = RaggedConvNorm(16, 64, kernel_size=5, dropout=0.1)
    assert {n: tuple(v.shape) for n, v in m.state_dict().items()} == {"conv.weight": (64, 16, 5), "conv.bias": (64,), "norm.weight": (64,),
                                                                      "norm.bias": (64,)}


def test_the_adaptor_takes_the_kernel_predictor_through_its_callable_path():
    from transformertts_amd import KernelVariancePredictor, VarianceAdaptor
    a = VarianceAdaptor(64, n_bins=8, predictor=KernelVariancePredictor)
    assert all(isinstance(m, KernelVariancePredictor) for m in (a.duration_predictor, a.pitch_predictor, a.energy_predictor))
    assert a.duration_predictor.conv1.weight.shape == (256, 64, 3)
    assert isinstance(VarianceAdaptor(64, n_bins=8).duration_predictor, __import__("transformertts_amd").VariancePredictor)


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


FWD_PTRS = ("x", "lens", "w", "bias", "gamma", "beta", "step_seed", "y", "r", "mean", "rstd", "x_masked")
FWD = dict(order=("x", "ld_row", "ld_batch", "lens", "w", "bias", "gamma", "beta", "B", "Pmax", "Cin", "Cout", "taps", "eps", "drop_p",
                  "seed", "step_seed", "y", "r", "mean", "rstd", "x_masked"),
           pointers=FWD_PTRS,
           defaults=dict(dict.fromkeys(FWD_PTRS, 0), ld_row=16, ld_batch=160, B=2, Pmax=10, Cin=16, Cout=32, taps=3, eps=1e-5, drop_p=0.0,
                         seed=0, step_seed=None))
BWD_PTRS = ("dy", "r", "mean", "rstd", "x_masked", "lens", "w", "gamma", "step_seed", "dx", "dw", "dbias", "dgamma", "dbeta", "ws")
BWD = dict(order=("dy", "r", "mean", "rstd", "x_masked", "lens", "w", "gamma", "B", "Pmax", "Cin", "Cout", "taps", "drop_p", "seed",
                  "step_seed", "dx", "dw", "dbias", "dgamma", "dbeta", "ws", "ws_bytes", "accumulate"),
           pointers=BWD_PTRS,
           defaults=dict(dict.fromkeys(BWD_PTRS, 0), B=2, Pmax=10, Cin=16, Cout=32, taps=3, drop_p=0.0, seed=0, step_seed=None,
                         ws_bytes=1 << 30, accumulate=0))
SHAPE = [(dict(B=0), "B must be in [1, 65535] (one grid row per utterance), got 0"), (dict(B=65536), "got 65536"),
         (dict(Pmax=0), "Pmax must be in [1, 4096] phonemes, got 0"), (dict(Pmax=4097), "Pmax must be in [1, 4096] phonemes, got 4097"),
         (dict(Cin=0), "Cin must be a multiple of 4 in [4, 1024], got 0"), (dict(Cin=18, ld_row=20), "Cin must be a multiple of 4 in [4, 1024], got 18"),
         (dict(Cin=1028, ld_row=1028), "got 1028"),
         (dict(Cout=0), "Cout must be a multiple of 32 in [32, 256], got 0"), (dict(Cout=48), "Cout must be a multiple of 32 in [32, 256], got 48"),
         (dict(Cout=288), "got 288"),
         (dict(taps=0), "taps must be odd in [1, 9], got 0"), (dict(taps=4), "taps must be odd in [1, 9], got 4"), (dict(taps=11), "got 11"),
         (dict(drop_p=1.0), "drop_p must be in [0, 1), got 1"), (dict(drop_p=-0.5), "drop_p must be in [0, 1), got -0.5"),
         (dict(drop_p=float("nan")), "drop_p must be in [0, 1), got nan")]
REFUSALS = (
    [("ttts_ragged_conv_norm_fwd", FWD, kw, needle) for kw, needle in
     [(dict([(n, None)]), "null pointer") for n in ("x", "lens", "w", "bias", "gamma", "beta", "y")] + SHAPE + [
        (dict(r=None), "null pointer (r, mean and rstd go together: all three or none)"), (dict(mean=None), "all three or none"),
        (dict(rstd=None, r=None), "all three or none"),
        (dict(eps=0.0), "eps must be positive and finite, got 0"), (dict(eps=-1.0), "eps must be positive and finite, got -1"),
        (dict(eps=float("inf")), "eps must be positive and finite, got inf"), (dict(eps=float("nan")), "got nan"),
        (dict(ld_row=12), "the row stride must be a multiple of 4 and >= Cin (ld_row 12, Cin 16)"),
        (dict(ld_row=18), "the row stride must be a multiple of 4 and >= Cin (ld_row 18, Cin 16)"),
        (dict(ld_batch=156), "the batch stride must be a multiple of 4 and cover an utterance (ld_batch 156, ld_row 16, Pmax 10, Cin 16)"),
        (dict(ld_batch=162), "the batch stride must be a multiple of 4 and cover an utterance (ld_batch 162"),
        (dict(B=1, ld_batch=-4), "the batch stride"),
        (dict(x=8), "x, w, y, r and x_masked must be 16-byte aligned"), (dict(w=4), "16-byte aligned"), (dict(y=8), "16-byte aligned"),
        (dict(r=8), "16-byte aligned"), (dict(x_masked=4), "16-byte aligned"),
        (dict(bias=2), "bias, gamma, beta, mean and rstd must be 4-byte aligned"), (dict(gamma=1), "4-byte aligned"), (dict(beta=3), "4-byte aligned"),
        (dict(mean=2), "4-byte aligned"), (dict(rstd=2), "4-byte aligned"),
        (dict(lens=4), "lens and step_seed must be 8-byte aligned"), (dict(step_seed=4), "8-byte aligned")]] +
    [("ttts_ragged_conv_norm_bwd", BWD, kw, needle) for kw, needle in
     [(dict([(n, None)]), "null pointer") for n in ("dy", "r", "mean", "rstd", "lens", "w", "gamma", "dbias", "dgamma", "dbeta", "ws")] + SHAPE + [
        (dict(x_masked=None), "null pointer (the weight gradient needs x_masked)"),
        (dict(dy=8), "dy, r, x_masked, w, dx, dw and ws must be 16-byte aligned"), (dict(r=4), "16-byte aligned"), (dict(x_masked=8), "16-byte aligned"),
        (dict(w=8), "16-byte aligned"), (dict(dx=8), "16-byte aligned"), (dict(dw=4), "16-byte aligned"), (dict(ws=8), "16-byte aligned"),
        (dict(mean=2), "mean, rstd, gamma, dbias, dgamma and dbeta must be 4-byte aligned"), (dict(rstd=1), "4-byte aligned"),
        (dict(gamma=2), "4-byte aligned"), (dict(dbias=2), "4-byte aligned"), (dict(dgamma=3), "4-byte aligned"), (dict(dbeta=2), "4-byte aligned"),
        (dict(lens=4), "lens and step_seed must be 8-byte aligned"), (dict(step_seed=12), "8-byte aligned"),
        (dict(ws_bytes=64), "workspace too small (64 bytes, need ")]])


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_every_refusal_names_its_value_before_any_launch(case):
    from transformertts_amd import _lib
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


def test_ragged_conv_norm_refuses():
    from transformertts_amd.predictor import KernelVariancePredictor, RaggedConvNorm, ragged_conv_norm
    pl = torch.tensor([12, 3, 1])
    x = _cuda((3, 12, 16))
    w, v = _cuda((32, 16, 3)), _cuda((32,))
    for args, kw, needle in (
            ((torch.zeros(3, 12), pl, w, v, v, v), {}, "x must be (B, Pmax, Cin), got (3, 12)"),
            ((torch.zeros(3, 12, 16), pl, w, v, v, v), {}, "ragged_conv_norm.x: expected a CUDA/HIP tensor (the HIP path has no CPU fallback), got cpu"),
            ((_cuda((3, 12, 16), dtype=torch.float64), pl, w, v, v, v), {}, "ragged_conv_norm.x: expected dtype torch.float32, got torch.float64"),
            ((_cuda((3, 12, 18)), pl, w, v, v, v), {}, "Cin must be a multiple of 4 in [4, 1024], got 18"),
            ((_cuda((3, 12, 1028)), pl, w, v, v, v), {}, "Cin must be a multiple of 4 in [4, 1024], got 1028"),
            ((_cuda((3, 4097, 16)), pl, w, v, v, v), {}, "Pmax must be in [1, 4096] phonemes, got 4097"),
            ((_cuda((65536, 2, 16)), pl, w, v, v, v), {}, "B must be in [1, 65535], got 65536"),
            ((x, torch.tensor([12, 3]), w, v, v, v), {}, "ragged_conv_norm.lens must have shape (3,), got (2,)"),
            ((x, torch.tensor([12.0, 3.0, 1.0]), w, v, v, v), {}, "ragged_conv_norm.lens must be integers, got torch.float32"),
            ((x, pl, _cuda((32, 8, 3)), v, v, v), {}, "weight must be (Cout, 16, k), got (32, 8, 3)"),
            ((x, pl, _cuda((48, 16, 3)), v, v, v), {}, "Cout must be a multiple of 32 in [32, 256], got 48"),
            ((x, pl, _cuda((288, 16, 3)), v, v, v), {}, "Cout must be a multiple of 32 in [32, 256], got 288"),
            ((x, pl, _cuda((32, 16, 4)), v, v, v), {}, "the kernel size must be odd in [1, 9], got 4"),
            ((x, pl, _cuda((32, 16, 11)), v, v, v), {}, "the kernel size must be odd in [1, 9], got 11"),
            ((x, pl, _cuda((32, 16, 3), dtype=torch.float16), v, v, v), {}, "ragged_conv_norm.weight: expected a torch.float32 CUDA/HIP tensor"),
            ((x, pl, w, _cuda((16,)), v, v), {}, "bias must be (32,), got (16,)"),
            ((x, pl, w, v, _cuda((31,)), v), {}, "gamma must be (32,), got (31,)"),
            ((x, pl, w, v, v, torch.zeros(32)), {}, "ragged_conv_norm.beta: expected a torch.float32 CUDA/HIP tensor, got torch.float32 on cpu"),
            ((x, pl, w, v, v, v), dict(eps=0.0), "eps must be positive and finite, got 0.0"),
            ((x, pl, w, v, v, v), dict(eps=float("nan")), "eps must be positive and finite, got nan"),
            ((x, pl, w, v, v, v), dict(drop_p=1.0), "drop_p must be in [0, 1), got 1.0"),
            ((x, pl, w, v, v, v), dict(drop_p=-0.1), "drop_p must be in [0, 1), got -0.1")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            ragged_conv_norm(*args, **kw)
    for make, needle in ((lambda: RaggedConvNorm(16, 32, kernel_size=4), "RaggedConvNorm: kernel_size must be odd in [1, 9], got 4"),
                         (lambda: RaggedConvNorm(16, 32, dropout=1.0), "RaggedConvNorm: drop_p must be in [0, 1), got 1.0"),
                         (lambda: KernelVariancePredictor(16, kernel_size=11), "KernelVariancePredictor: kernel_size must be odd in [1, 9], got 11"),
                         (lambda: KernelVariancePredictor(16, hidden=100), "hidden must be a multiple of 32 in [32, 256], got 100"),
                         (lambda: KernelVariancePredictor(16, hidden=512), "hidden must be a multiple of 32 in [32, 256], got 512"),
                         (lambda: KernelVariancePredictor(18), "d_model must be a multiple of 4 in [4, 1024], got 18"),
                         (lambda: KernelVariancePredictor(16, dropout=-1), "KernelVariancePredictor: drop_p must be in [0, 1), got -1.0")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            make()
