"""Variance adaptor (csrc/variance.hip, transformertts_amd/variance.py): the oracles of tests/variance_reference.py against the
naive repeat loop and against each other, the transpose identity, rounding at exact halves, every refusal of the six entry
points and of the Python checks with its message, before any launch; the header, the bindings and the exports.  Host logic
only, no GPU."""
import os
import re
import types

import numpy as np
import pytest
import torch

from variance_reference import (HUGE, bucket_ref, durations_from_log_ref, embedding_bwd_ref, embedding_bwd_stock, length_regulate_bwd_stock,
                                length_regulate_naive, length_regulate_ref, length_regulate_transpose_ref, poison, round_half_even_ref,
                                spans_ref, variance_embed_ref, variance_loss_grad_ref, variance_loss_grad_stock, variance_loss_ref,
                                variance_loss_stock)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ttts_length_regulate_frames", "ttts_length_regulate_fwd", "ttts_length_regulate_bwd", "ttts_durations_from_log",
       "ttts_variance_embed_fwd", "ttts_variance_loss_fwd", "ttts_variance_loss_bwd")
EXPORTS = ("length_regulate", "LengthRegulator", "durations_from_log", "variance_embed", "VarianceEmbedding", "variance_bins",
           "VarianceLoss", "VariancePredictor", "VarianceAdaptor")


def test_the_header_declares_each_entry_point_once_and_the_exports_agree():
    from transformertts_amd import _lib, variance
    import transformertts_amd
    lib = _lib.load()
    hdr = open(os.path.join(REPO, "include", "ttts_hip.h")).read()
    for name in NEW:
        decls = re.findall(r"^(?:int|size_t) " + name + r"\s*\(([^;]*)\)\s*;", hdr, re.M)
        assert len(decls) == 1, f"{name} must be declared exactly once in ttts_hip.h, found {len(decls)}"
        assert name in _lib.SIGNATURES and hasattr(lib, name), f"{name} is not exported / bound"
        n_args = 0 if decls[0].strip() == "void" else len(decls[0].split(","))
        assert n_args == len(_lib.SIGNATURES[name][1]), name
    assert lib.ttts_abi_version() == 24                               # additive
    for name in EXPORTS:
        assert getattr(transformertts_amd, name) is getattr(variance, name) and name in transformertts_amd.__all__
    assert tuple(variance.__all__) == EXPORTS
    assert lib.ttts_length_regulate_frames() == 32
    src = open(os.path.join(REPO, "transformertts_amd", "csrc", "variance.hip")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert "atomic" not in code.replace("__ATOMIC_", "") and "hipMalloc" not in code and "hipMemcpy" not in code
    for const, value in (("VAR_MAX_P", variance.MAX_PHONEMES), ("VAR_MAX_D", variance.MAX_WIDTH), ("VAR_MAX_BINS", variance.MAX_BINS)):
        assert re.search(const + r" = (\d+)", src).group(1) == str(value)
    assert variance.MAX_FRAMES == 1 << 20 and "VAR_MAX_T = 1 << 20" in src
    assert "LOSS_THREADS = 1024" in src                               # the stock form's order is the kernel's


# ------------------------------------------------------------------------------------------------ the oracles
def test_the_regulator_oracle_against_the_naive_repeat_loop():
    rng = np.random.default_rng(0)
    for B, Pmax, D, Tmax, lens in ((3, 12, 4, 40, [12, 5, 0]), (1, 1, 8, 7, [1]), (2, 70, 4, 300, [70, 33]), (2, 9, 4, 11, [9, 9])):
        x, dur, _, _ = poison(rng, B, Pmax, D, lens)
        dur[0, 0] = -3 if lens[0] else dur[0, 0]
        y, frames, index = length_regulate_ref(x, dur, lens, Tmax)
        want = length_regulate_naive(x, dur, lens, Tmax)
        assert np.array_equal(y, want) and not np.isnan(y).any()
        for b in range(B):
            total = int(np.maximum(dur[b, :lens[b]], 0).sum())
            assert frames[b] == min(total, Tmax) and (index[b, frames[b]:] == -1).all() and (y[b, frames[b]:] == 0).all()
            assert (np.diff(index[b, :frames[b]]) >= 0).all() and (index[b, :frames[b]] < lens[b]).all()
            assert np.array_equal(y[b, :frames[b]], x[b, index[b, :frames[b]]])
    a, e, frames = spans_ref(np.array([[2, 0, 3, 9]]), [4], 8)
    assert a.tolist() == [[0, 2, 2, 5]] and e.tolist() == [[2, 2, 5, 8]] and frames.tolist() == [8]


def test_the_transpose_identity_and_the_sequential_form():
    rng = np.random.default_rng(1)
    B, Pmax, D, Tmax, lens = 3, 20, 8, 90, [20, 11, 0]
    x, dur, _, _ = poison(rng, B, Pmax, D, lens)
    dur[0, 3] = 40
    g = rng.standard_normal((B, Tmax, D))
    xz = np.where(np.isnan(x), 0.0, x).astype(np.float64)
    y, _, _ = length_regulate_ref(xz, dur, lens, Tmax)
    gt = length_regulate_transpose_ref(g, dur, lens, Pmax)
    assert abs((y * g).sum() - (xz * gt).sum()) <= 1e-12 * np.abs(y * g).sum()            # <L x, g> = <x, L^T g>
    g32 = g.astype(np.float32)
    stock = length_regulate_bwd_stock(g32, dur, lens, Pmax)
    ref = length_regulate_transpose_ref(g32, dur, lens, Pmax)
    assert stock.dtype == np.float32 and np.abs(stock - ref).max() <= 1e-6 * np.abs(ref).max()
    assert (stock[2] == 0).all() and (stock[1, 11:] == 0).all() and (stock[0][dur[0] == 0] == 0).all()
    into = rng.standard_normal((B, Pmax, D)).astype(np.float32)
    assert np.array_equal(length_regulate_bwd_stock(g32, dur, lens, Pmax, into=into), into + stock)


def test_durations_round_half_to_even():
    assert round_half_even_ref([0.5, 1.5, 2.5, -0.5, 3.5]).tolist() == [0.0, 2.0, 2.0, -0.0, 4.0]
    # exp(2^-30) - 1 is 2^-30 exactly in fp64, so alpha = 2^29, 3 2^29, 5 2^29 land on 0.5, 1.5, 2.5 exactly
    tiny = np.full((1, 1), 2.0 ** -30, np.float32)
    assert (np.exp(np.float64(tiny[0, 0])) - 1.0) * 2.0 ** 29 == 0.5
    assert [int(durations_from_log_ref(tiny, [1], alpha=k * 2.0 ** 29)[0, 0]) for k in (1, 3, 5)] == [0, 2, 2]
    assert np.exp(np.log(2.0)) == 2.0
    ln2 = np.full((1, 1), np.log(2.0))
    assert [int(durations_from_log_ref(ln2, [1], alpha=a)[0, 0]) for a in (0.5, 1.5, 2.5, 1.0)] == [0, 2, 2, 1]
    log_d = np.array([[np.nan, np.inf, -np.inf, -50.0, 0.0, np.log(4.0), 100.0, 1000.0, 3.0]], np.float32)
    assert durations_from_log_ref(log_d, [8]).tolist() == [[0, 0, 0, 0, 0, 3, 2 ** 31 - 1, 2 ** 31 - 1, 0]]
    assert durations_from_log_ref(log_d, [8], min_duration=2).tolist() == [[2, 2, 2, 2, 2, 3, 2 ** 31 - 1, 2 ** 31 - 1, 0]]
    assert durations_from_log_ref(log_d, [9], alpha=2.0)[0, 5:6].tolist() == [6]


def test_the_embedding_oracle_buckets_like_torch_bucketize():
    bins = np.array([1.0, 2.0, 2.0, 5.0], np.float32)
    v = np.array([0.0, 1.0, 1.5, 2.0, 2.5, 5.0, 6.0, -np.inf, np.inf], np.float32)
    want = torch.bucketize(torch.from_numpy(v), torch.from_numpy(bins), right=False).numpy()
    assert np.array_equal(bucket_ref(v, bins), want) and want.tolist() == [0, 0, 1, 1, 3, 3, 4, 0, 4]
    assert bucket_ref(np.array([np.nan]), bins).tolist() == [0]       # the kernel's rule for a NaN (torch puts it last)
    rng = np.random.default_rng(2)
    x, _, pitch, energy = poison(rng, 2, 6, 4, [6, 2])
    pb, eb = np.linspace(100, 600, 7).astype(np.float32), np.linspace(0, 1, 3).astype(np.float32)
    Ep, Ee = rng.standard_normal((8, 4)).astype(np.float32), rng.standard_normal((4, 4)).astype(np.float32)
    y, i, j = variance_embed_ref(x, [6, 2], pitch, pb, Ep, energy, eb, Ee)
    s, _, _ = variance_embed_ref(x, [6, 2], pitch, pb, Ep, energy, eb, Ee, dtype=np.float32)
    assert (i[1, 2:] == -1).all() and (j[1, 2:] == -1).all() and np.isnan(y[1, 2:]).all() and not np.isnan(y[0]).any()
    assert s.dtype == np.float32 and np.array_equal(s[0], (x[0] + Ep[i[0]]) + Ee[j[0]]) and np.abs(s[0] - y[0]).max() <= 1e-6
    y2, i2, j2 = variance_embed_ref(x, [6, 2], energy=energy, energy_bins=eb, Ee=Ee)
    assert i2 is None and np.array_equal(j2, j) and np.array_equal(y2[0], x[0].astype(np.float64) + Ee[j[0]])
    ids = np.array([[0, 2, -1], [2, 2, 1]])
    g = rng.standard_normal((2, 3, 4)).astype(np.float32)
    stock, ref = embedding_bwd_stock(ids, g, 3), embedding_bwd_ref(ids, g, 3)
    assert np.array_equal(stock[2], (g[0, 1] + g[1, 0]) + g[1, 1]) and np.abs(stock - ref).max() <= 1e-6


def test_the_loss_oracle_and_its_stock_form():
    rng = np.random.default_rng(3)
    B, Pmax, lens = 3, 700, [700, 401, 0]                             # more than 1024 valid elements: every thread adds twice
    _, dur, pitch, energy = poison(rng, B, Pmax, 4, lens)
    dur[0, 0] = -4                                                    # counts as 0: the target is log(1) = 0
    preds = [rng.standard_normal((B, Pmax)).astype(np.float32) for _ in range(3)]
    pitch, energy = (pitch / 100).astype(np.float32), energy
    w = (1.0, 0.5, 2.0)
    args = (preds[0], dur, preds[1], pitch, preds[2], energy, lens)
    ref, stock = variance_loss_ref(*args, weights=w), variance_loss_stock(*args, weights=w)
    assert stock.dtype == np.float32 and np.isfinite(ref).all() and np.abs(stock / ref - 1).max() <= 1e-6
    n = sum(lens)
    valid = np.arange(Pmax)[None, :] < np.array(lens)[:, None]
    direct = ((preds[1].astype(np.float64) - pitch)[valid] ** 2).sum() / n
    assert abs(ref[1] / direct - 1) <= 1e-14 and abs(ref[3] - (ref[0] + 0.5 * ref[1] + 2 * ref[2])) <= 1e-12
    tgt0 = np.log(np.maximum(dur[0, :2], 0) + 1.0)
    assert tgt0[0] == 0.0
    gout = np.array([0.0, 0.0, 0.0, 1.5], np.float32)
    gs, gr = variance_loss_grad_stock(*args, w, gout), variance_loss_grad_ref(*args, w, gout)
    for a, r in zip(gs, gr):
        assert a.dtype == np.float32 and (a[~valid] == 0).all() and np.abs(a - r).max() <= 1e-6 * np.abs(r).max()
    eps = 1e-3                                                         # the gradient is the total's derivative
    bumped = preds[1].copy()
    bumped[1, 7] += eps
    num = (variance_loss_ref(preds[0], dur, bumped, pitch, preds[2], energy, lens, weights=w)[3] - ref[3]) / (bumped[1, 7] - preds[1][1, 7])
    assert abs(num * 1.5 - gr[1][1, 7]) <= 1e-3 * abs(gr[1][1, 7]) + 1e-6
    empty = (preds[0], dur, preds[1], pitch, preds[2], energy, [0, 0, 0])
    assert (variance_loss_ref(*empty) == 0).all() and (variance_loss_stock(*empty) == 0).all()
    assert all((g == 0).all() for g in variance_loss_grad_stock(*empty, w, gout))


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


FWD = dict(order=("x", "ld_row", "ld_batch", "durations", "phoneme_lens", "B", "Pmax", "Tmax", "D", "y", "mel_lens", "index"),
           pointers=("x", "durations", "phoneme_lens", "y", "mel_lens", "index"),
           defaults=dict(x=0, ld_row=16, ld_batch=160, durations=0, phoneme_lens=0, B=2, Pmax=10, Tmax=40, D=16, y=0, mel_lens=0, index=0))
BWD = dict(order=("dy", "durations", "phoneme_lens", "B", "Pmax", "Tmax", "D", "dx", "accumulate"),
           pointers=("dy", "durations", "phoneme_lens", "dx"),
           defaults=dict(dy=0, durations=0, phoneme_lens=0, B=2, Pmax=10, Tmax=40, D=16, dx=0, accumulate=0))
DFL = dict(order=("log_d", "phoneme_lens", "B", "Pmax", "alpha", "min_duration", "durations"), pointers=("log_d", "phoneme_lens", "durations"),
           defaults=dict(log_d=0, phoneme_lens=0, B=2, Pmax=10, alpha=1.0, min_duration=0, durations=0))
EMB = dict(order=("x", "ld_row", "ld_batch", "pitch", "energy", "pitch_bins", "n_pitch", "energy_bins", "n_energy", "pitch_table",
                  "energy_table", "phoneme_lens", "B", "Pmax", "D", "y", "pitch_ids", "energy_ids"),
           pointers=("x", "pitch", "energy", "pitch_bins", "energy_bins", "pitch_table", "energy_table", "phoneme_lens", "y", "pitch_ids",
                     "energy_ids"),
           defaults=dict(x=0, ld_row=16, ld_batch=160, pitch=0, energy=0, pitch_bins=0, n_pitch=8, energy_bins=0, n_energy=8, pitch_table=0,
                         energy_table=0, phoneme_lens=0, B=2, Pmax=10, D=16, y=0, pitch_ids=0, energy_ids=0))
LOSS_ORDER = ("log_d_pred", "durations", "pitch_pred", "pitch_target", "energy_pred", "energy_target", "phoneme_lens", "B", "Pmax", "w_d",
              "w_p", "w_e")
LOSS_PTRS = ("log_d_pred", "durations", "pitch_pred", "pitch_target", "energy_pred", "energy_target", "phoneme_lens")
LOSS_DEFAULTS = dict(dict.fromkeys(LOSS_PTRS, 0), B=2, Pmax=10, w_d=1.0, w_p=1.0, w_e=1.0)
LFW = dict(order=LOSS_ORDER + ("out",), pointers=LOSS_PTRS + ("out",), defaults=dict(LOSS_DEFAULTS, out=0))
LBW = dict(order=LOSS_ORDER + ("gout", "d_log_d", "d_pitch", "d_energy"), pointers=LOSS_PTRS + ("gout", "d_log_d", "d_pitch", "d_energy"),
           defaults=dict(LOSS_DEFAULTS, gout=0, d_log_d=0, d_pitch=0, d_energy=0))

SHAPE = [(dict(B=0), "B must be in [1, 65535] (one grid row per utterance), got 0"), (dict(B=65536), "got 65536"),
         (dict(Pmax=0), "Pmax must be in [1, 4096] phonemes, got 0"), (dict(Pmax=4097), "Pmax must be in [1, 4096] phonemes, got 4097")]
TMAX = [(dict(Tmax=0), "Tmax must be in [1, 2^20] frames, got 0"), (dict(Tmax=(1 << 20) + 1), f"got {(1 << 20) + 1}")]
WIDTH = [(dict(D=0), "D must be a multiple of 4 in [4, 4096], got 0"), (dict(D=18, ld_row=20), "got 18"),
         (dict(D=4100, ld_row=4100), "D must be a multiple of 4 in [4, 4096], got 4100")]
STRIDES = [(dict(ld_row=12), "the row stride must be a multiple of 4 and >= D (ld_row 12, D 16)"),
           (dict(ld_row=18), "the row stride must be a multiple of 4 and >= D (ld_row 18, D 16)"),
           (dict(ld_batch=156), "the batch stride must be a multiple of 4 and cover an utterance (ld_batch 156, ld_row 16, Pmax 10, D 16)"),
           (dict(ld_batch=162), "the batch stride must be a multiple of 4 and cover an utterance (ld_batch 162"),
           (dict(ld_row=32, ld_batch=300), "cover an utterance (ld_batch 300, ld_row 32, Pmax 10, D 16)")]
WEIGHTS = [(dict(w_d=float("nan")), "the weights must be finite, got nan, 1, 1"), (dict(w_e=float("inf")), "the weights must be finite, got 1, 1, inf")]


def _nulls(spec, optional=()):
    return [(dict([(name, None)]), "null pointer") for name in spec["pointers"] if name not in optional]


REFUSALS = (
    [("ttts_length_regulate_fwd", FWD, kw, needle) for kw, needle in _nulls(FWD) + SHAPE + TMAX + WIDTH + STRIDES + [
        (dict(x=8), "x and y must be 16-byte aligned"), (dict(y=4), "x and y must be 16-byte aligned"),
        (dict(durations=4), "durations, phoneme_lens and mel_lens must be 8-byte aligned"), (dict(phoneme_lens=12), "8-byte aligned"),
        (dict(mel_lens=4), "8-byte aligned"), (dict(index=2), "index must be 4-byte aligned")]] +
    [("ttts_length_regulate_bwd", BWD, kw, needle) for kw, needle in _nulls(BWD) + SHAPE + TMAX + WIDTH + [
        (dict(dy=8), "dy and dx must be 16-byte aligned"), (dict(dx=4), "dy and dx must be 16-byte aligned"),
        (dict(durations=4), "durations and phoneme_lens must be 8-byte aligned"), (dict(phoneme_lens=4), "8-byte aligned")]] +
    [("ttts_durations_from_log", DFL, kw, needle) for kw, needle in _nulls(DFL) + SHAPE + [
        (dict(alpha=0.0), "alpha must be positive and finite, got 0"), (dict(alpha=-1.0), "alpha must be positive and finite, got -1"),
        (dict(alpha=float("inf")), "alpha must be positive and finite, got inf"), (dict(alpha=float("nan")), "got nan"),
        (dict(min_duration=-1), "min_duration must be in [0, 2^31 - 1], got -1"), (dict(min_duration=1 << 31), f"got {1 << 31}"),
        (dict(log_d=2), "log_d must be 4-byte aligned"), (dict(phoneme_lens=4), "phoneme_lens and durations must be 8-byte aligned"),
        (dict(durations=4), "phoneme_lens and durations must be 8-byte aligned")]] +
    [("ttts_variance_embed_fwd", EMB, kw, needle) for kw, needle in
     _nulls(EMB, optional=("pitch", "energy", "pitch_bins", "energy_bins", "pitch_table", "energy_table", "pitch_ids", "energy_ids")) +
     SHAPE + WIDTH + STRIDES + [
        (dict(pitch=None), "null pointer (a pitch table needs pitch, pitch_bins and pitch_ids)"), (dict(pitch_bins=None), "a pitch table needs"),
        (dict(pitch_ids=None), "a pitch table needs"), (dict(energy=None), "null pointer (an energy table needs energy, energy_bins and energy_ids)"),
        (dict(energy_bins=None), "an energy table needs"), (dict(energy_ids=None), "an energy table needs"),
        (dict(n_pitch=1), "n_pitch must be in [2, 4096] table rows, got 1"), (dict(n_pitch=4097), "n_pitch must be in [2, 4096] table rows, got 4097"),
        (dict(n_energy=1), "n_energy must be in [2, 4096] table rows, got 1"), (dict(n_energy=4097), "got 4097"),
        (dict(x=8), "x, y and the tables must be 16-byte aligned"), (dict(y=4), "16-byte aligned"), (dict(pitch_table=8), "16-byte aligned"),
        (dict(energy_table=4), "16-byte aligned"), (dict(pitch=2), "pitch, energy and the boundaries must be 4-byte aligned"),
        (dict(energy=1), "4-byte aligned"), (dict(pitch_bins=2), "4-byte aligned"), (dict(energy_bins=3), "4-byte aligned"),
        (dict(phoneme_lens=4), "phoneme_lens and the ids must be 8-byte aligned"), (dict(pitch_ids=4), "8-byte aligned"),
        (dict(energy_ids=12), "8-byte aligned")]] +
    [("ttts_variance_loss_fwd", LFW, kw, needle) for kw, needle in _nulls(LFW) + SHAPE + WEIGHTS + [
        (dict(log_d_pred=2), "the predictions and targets must be 4-byte aligned"), (dict(pitch_pred=1), "4-byte aligned"),
        (dict(pitch_target=2), "4-byte aligned"), (dict(energy_pred=3), "4-byte aligned"), (dict(energy_target=2), "4-byte aligned"),
        (dict(durations=4), "durations and phoneme_lens must be 8-byte aligned"), (dict(phoneme_lens=4), "8-byte aligned"),
        (dict(out=2), "out must be 4-byte aligned")]] +
    [("ttts_variance_loss_bwd", LBW, kw, needle) for kw, needle in _nulls(LBW) + SHAPE + WEIGHTS + [
        (dict(log_d_pred=2), "the predictions and targets must be 4-byte aligned"), (dict(durations=4), "8-byte aligned"),
        (dict(gout=2), "gout and the gradients must be 4-byte aligned"), (dict(d_log_d=1), "4-byte aligned"), (dict(d_pitch=2), "4-byte aligned"),
        (dict(d_energy=3), "4-byte aligned")]])


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_every_refusal_names_its_value_before_any_launch(case):
    from transformertts_amd import _lib
    lib = _lib.load()
    entry, spec, kw, needle = REFUSALS[case]
    rc = _call(lib, entry, spec["order"], spec["pointers"], spec["defaults"], kw)
    assert rc != 0 and needle in _lib.last_error() and entry[5:] in _lib.last_error(), (entry, kw, _lib.last_error())
    with pytest.raises(RuntimeError, match=re.escape(needle)):       # ... and reaches Python through _lib.check
        _lib.check(rc, entry)


def test_one_utterance_needs_no_batch_stride():
    """B = 1 accepts any non-negative batch stride, as the other ragged entries do: only a negative one is refused"""
    from transformertts_amd import _lib
    lib = _lib.load()
    rc = _call(lib, "ttts_length_regulate_fwd", FWD["order"], FWD["pointers"], FWD["defaults"], dict(B=1, ld_batch=-4))
    assert rc != 0 and "the batch stride" in _lib.last_error()


# ------------------------------------------------------------------------------------------------ refusals of the Python checks
def _cuda(shape, dtype=torch.float32, **kw):
    """what the checks read of a device tensor, on the CPU: those in front of the launch can be reached without a device"""
    d = dict(shape=tuple(shape), dim=lambda: len(shape), is_cuda=True, dtype=dtype, device="cuda:0")
    d.update(kw)
    return types.SimpleNamespace(**d)


def test_length_regulate_refuses():
    from transformertts_amd.variance import LengthRegulator, length_regulate
    d, pl = torch.zeros(3, 12, dtype=torch.int64), torch.tensor([12, 3, 1])
    for args, needle in (
            ((torch.zeros(12, 8), d, pl, 40), "length_regulate: x must be (B, Pmax, D), got (12, 8)"),
            ((torch.zeros(3, 0, 8), d, pl, 40), "length_regulate: x must be (B, Pmax, D), got (3, 0, 8)"),
            ((torch.zeros(3, 12, 8), d, pl, 40), "length_regulate.x: expected a CUDA/HIP tensor (the HIP path has no CPU fallback), got cpu"),
            ((_cuda((3, 12, 8), torch.float64), d, pl, 40), "length_regulate.x: expected dtype torch.float32, got torch.float64"),
            ((_cuda((3, 12, 6)), d, pl, 40), "length_regulate: D must be a multiple of 4 in [4, 4096], got 6"),
            ((_cuda((3, 12, 4100)), d, pl, 40), "length_regulate: D must be a multiple of 4 in [4, 4096], got 4100"),
            ((_cuda((3, 4097, 8)), d, pl, 40), "length_regulate: Pmax must be in [1, 4096] phonemes, got 4097"),
            ((_cuda((65536, 12, 8)), d, pl, 40), "length_regulate: B must be in [1, 65535], got 65536")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            length_regulate(*args)
    from transformertts_amd import variance
    dev = torch.device("cpu")
    for t, needle in ((torch.zeros(2, 12, dtype=torch.int64), "length_regulate: durations must be (3, 12), got (2, 12)"),
                      (torch.zeros(3, dtype=torch.int64), "length_regulate: durations must be (3, 12), got (3,)"),
                      (d.to(torch.int32), "length_regulate.durations: expected dtype torch.int64, got torch.int32")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            variance._per_phoneme(t, 3, 12, "length_regulate", "durations", torch.int64, dev)
    for t, needle in ((pl[:2], "length_regulate.phoneme_lens must have shape (3,), got (2,)"),
                      (pl.float(), "length_regulate.phoneme_lens must be integers, got torch.float32"),
                      (pl > 1, "length_regulate.phoneme_lens must be integers, got torch.bool")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            variance._lens(t, 3, "length_regulate", "phoneme_lens", dev)
    assert variance._lens(pl.to(torch.int32), 3, "f", "phoneme_lens", dev).dtype == torch.int64
    for bad in (0, -1, (1 << 20) + 1, 2.5, True, "40"):
        with pytest.raises(ValueError, match=re.escape(f"max_len must be an integer in [1, 2^20] frames, got {bad!r}")):
            variance._max_len(bad, "length_regulate")
    with pytest.raises(ValueError, match=re.escape("LengthRegulator: max_len must be an integer in [1, 2^20] frames, got 0")):
        LengthRegulator(max_len=0)
    assert LengthRegulator().max_len is None and LengthRegulator(870).max_len == 870


def test_durations_from_log_refuses():
    from transformertts_amd.variance import durations_from_log
    pl = torch.tensor([12, 3, 1])
    for args, kw, needle in (
            ((torch.zeros(12), pl), {}, "durations_from_log: log_d must be (B, Pmax), got (12,)"),
            ((torch.zeros(3, 12), pl), {}, "durations_from_log.log_d: expected a CUDA/HIP tensor (the HIP path has no CPU fallback), got cpu"),
            ((_cuda((3, 12), torch.float64), pl), {}, "durations_from_log.log_d: expected dtype torch.float32, got torch.float64"),
            ((_cuda((3, 4097)), pl), {}, "durations_from_log: Pmax must be in [1, 4096] phonemes, got 4097"),
            ((_cuda((3, 12)), pl[:2]), {}, "durations_from_log.phoneme_lens must have shape (3,), got (2,)")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            durations_from_log(*args, **kw)
    ok = _cuda((3, 12), to=lambda *a: None)
    for kw, needle in ((dict(alpha=0.0), "alpha must be positive and finite, got 0.0"), (dict(alpha=float("inf")), "got inf"),
                       (dict(alpha=float("nan")), "alpha must be positive and finite, got nan"),
                       (dict(min_duration=-1), "min_duration must be an integer in [0, 2^31 - 1], got -1"),
                       (dict(min_duration=1.5), "min_duration must be an integer in [0, 2^31 - 1], got 1.5")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            durations_from_log(ok, pl, **kw)


def test_variance_bins_and_the_embedding_constructor():
    from transformertts_amd.variance import VarianceEmbedding, variance_bins
    b = variance_bins(0.0, 1.0, 5)
    assert b.dtype == torch.float32 and b.tolist() == pytest.approx([0.0, 1 / 3, 2 / 3, 1.0], abs=1e-7)      # n_bins - 1 boundaries
    g = variance_bins(65.0, 600.0, 256, "log")
    assert g.numel() == 255 and abs(float(g[0]) - 65.0) < 1e-4 and abs(float(g[-1]) - 600.0) < 1e-3 and bool((g[1:] > g[:-1]).all())
    assert torch.allclose(g[1:] / g[:-1], (g[1] / g[0]).expand(254), rtol=1e-5)
    assert variance_bins(1.0, 2.0, 2).tolist() == [1.0]
    for args, needle in (((0, 1, 1), "n_bins must be an integer in [2, 4096], got 1"), ((0, 1, 4097), "got 4097"), ((0, 1, 2.0), "got 2.0"),
                         ((0, 1, 8, "mel"), "scale must be 'linear' or 'log', got 'mel'"), ((1, 1, 8), "need finite lo < hi (lo 1.0, hi 1.0)"),
                         ((0, float("inf"), 8), "need finite lo < hi"), ((0, 1, 8, "log"), "a log scale needs lo > 0, got 0.0")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            variance_bins(*args)
    m = VarianceEmbedding(8, 4, 16)
    assert m.pitch_bins.shape == (7,) and m.energy_bins.shape == (3,) and m.pitch_table.shape == (8, 16) and m.energy_table.shape == (4, 16)
    assert sorted(k for k, _ in m.named_parameters()) == ["energy_table", "pitch_table"] and sorted(m.state_dict()) == [
        "energy_bins", "energy_table", "pitch_bins", "pitch_table"]
    assert torch.equal(m.pitch_bins, variance_bins(65.0, 600.0, 8, "log")) and torch.equal(m.energy_bins, variance_bins(0.0, 1.0, 4))
    only = VarianceEmbedding(0, 4, 16, energy_bins=[0.1, 0.2, 0.2])
    assert only.pitch_table is None and only.pitch_bins is None and only.energy_bins.tolist() == pytest.approx([0.1, 0.2, 0.2])
    for args, kw, needle in (((8, 4, 18), {}, "d_model must be a multiple of 4 in [4, 4096], got 18"), ((8, 4, 0), {}, "got 0"),
                             ((1, 4, 16), {}, "n_pitch_bins must be 0 (no pitch) or in [2, 4096], got 1"),
                             ((8, 4097, 16), {}, "n_energy_bins must be 0 (no energy) or in [2, 4096], got 4097"),
                             ((8, 4, 16), dict(pitch_bins=[1.0, 2.0]), "pitch_bins must hold n_bins - 1 = 7 boundaries, got (2,)"),
                             ((8, 4, 16), dict(energy_bins=[3.0, 2.0, 4.0]), "energy_bins must be ascending and free of NaN"),
                             ((8, 4, 16), dict(energy_bins=[1.0, float("nan"), 4.0]), "energy_bins must be ascending and free of NaN")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            VarianceEmbedding(*args, **kw)
    with pytest.raises(ValueError, match="pitch given, but the module was built without a pitch table"):
        only(torch.zeros(1, 2, 16), torch.tensor([2]), pitch=torch.zeros(1, 2))
    with pytest.raises(ValueError, match=re.escape("variance_embed.x: expected a CUDA/HIP tensor")):
        m(torch.zeros(1, 2, 16), torch.tensor([2]), pitch=torch.zeros(1, 2))


def test_variance_embed_refuses():
    from transformertts_amd.variance import variance_embed
    x = _cuda((3, 12, 8), stride=lambda i: (96, 8, 1)[i], data_ptr=lambda: 0, device=torch.device("cpu"))
    pl = torch.tensor([12, 3, 1])
    v, bins, table = torch.zeros(3, 12), torch.zeros(7), torch.zeros(8, 8)
    dev_table = _cuda((8, 8), size=lambda i: 8, requires_grad=False)
    for kw, needle in (
            (dict(pitch=v), "variance_embed: pitch, pitch_bins and pitch_table go together (all three or none)"),
            (dict(energy=v, energy_bins=bins), "variance_embed: energy, energy_bins and energy_table go together"),
            (dict(pitch=torch.zeros(3, 11), pitch_bins=bins, pitch_table=table), "variance_embed: pitch must be (3, 12), got (3, 11)"),
            (dict(pitch=v.double(), pitch_bins=bins, pitch_table=table), "variance_embed.pitch: expected dtype torch.float32, got torch.float64"),
            (dict(pitch=v, pitch_bins=bins, pitch_table=torch.zeros(8, 4)), "variance_embed: pitch_table must be (n, 8) with n in [2, 4096], got (8, 4)"),
            (dict(pitch=v, pitch_bins=bins, pitch_table=torch.zeros(1, 8)), "with n in [2, 4096], got (1, 8)"),
            (dict(pitch=v, pitch_bins=bins, pitch_table=table), "variance_embed.pitch_table: expected a torch.float32 CUDA/HIP tensor, got torch.float32 on cpu"),
            (dict(energy=v, energy_bins=bins[:6], energy_table=dev_table), "variance_embed: energy_bins must be (7,) torch.float32 on the device, got (6,)"),
            (dict(energy=v, energy_bins=bins, energy_table=dev_table), "variance_embed: energy_bins must be (7,) torch.float32 on the device, got (7,) torch.float32 on cpu")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            variance_embed(x, pl, **kw)
    with pytest.raises(ValueError, match=re.escape("variance_embed.phoneme_lens must have shape (3,), got (2,)")):
        variance_embed(x, pl[:2])


def test_variance_loss_refuses():
    from transformertts_amd.variance import VarianceLoss
    for w, needle in (((1, 1), "weights must be three finite numbers (duration, pitch, energy), got (1.0, 1.0)"),
                      ((1, float("nan"), 1), "weights must be three finite numbers")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            VarianceLoss(w)
    loss = VarianceLoss()
    assert loss.weights == (1.0, 1.0, 1.0) and VarianceLoss((1, 0.5, 2)).weights == (1.0, 0.5, 2.0)
    d, v, pl = torch.zeros(3, 12, dtype=torch.int64), torch.zeros(3, 12), torch.tensor([12, 3, 1])
    ok = _cuda((3, 12), contiguous=lambda: None, device=torch.device("cpu"))
    for pred, args, needle in (
            (dict(log_duration=torch.zeros(12)), (d, v, v, pl), "VarianceLoss: pred['log_duration'] must be (B, Pmax), got (12,)"),
            (dict(log_duration=v), (d, v, v, pl), "VarianceLoss.log_duration: expected a CUDA/HIP tensor (the HIP path has no CPU fallback), got cpu"),
            (dict(log_duration=_cuda((3, 4097))), (d, v, v, pl), "VarianceLoss: Pmax must be in [1, 4096] phonemes, got 4097"),
            (dict(log_duration=ok, pitch=_cuda((3, 11)), energy=ok), (d, v, v, pl), "VarianceLoss: pred['pitch'] must be (3, 12), got (3, 11)"),
            (dict(log_duration=ok, pitch=ok, energy=_cuda((3, 12), torch.float64)), (d, v, v, pl),
             "VarianceLoss.energy: expected dtype torch.float32, got torch.float64"),
            (dict(log_duration=ok, pitch=ok, energy=ok), (d[:2], v, v, pl), "VarianceLoss: durations must be (3, 12), got (2, 12)"),
            (dict(log_duration=ok, pitch=ok, energy=ok), (d.int(), v, v, pl), "VarianceLoss.durations: expected dtype torch.int64, got torch.int32"),
            (dict(log_duration=ok, pitch=ok, energy=ok), (d, v[:, :5], v, pl), "VarianceLoss: pitch must be (3, 12), got (3, 5)"),
            (dict(log_duration=ok, pitch=ok, energy=ok), (d, v, v.double(), pl), "VarianceLoss.energy: expected dtype torch.float32, got torch.float64")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            loss(pred, *args)


def test_the_adaptor_and_the_predictor_on_the_host():
    from transformertts_amd.variance import VarianceAdaptor, VariancePredictor
    torch.manual_seed(0)
    p = VariancePredictor(16, hidden=8, dropout=0.0)
    x, pl = torch.randn(2, 9, 16), torch.tensor([9, 4])
    out = p(x, pl)
    assert out.shape == (2, 9) and (out[1, 4:] == 0).all()
    x2 = x.clone()
    x2[1, 4:] = float("nan")                                          # the padding does not leak into the valid rows
    assert torch.equal(p(x2, pl), out)
    q = VariancePredictor(16, hidden=8, kernel_size=5, dropout=0.0).double()      # the taps as one matrix product are nn.Conv1d
    xd = x.double()
    assert (q._conv(q.conv1, xd) - q.conv1(xd.transpose(1, 2)).transpose(1, 2)).abs().max() <= 1e-12
    assert sorted(k for k, _ in p.named_parameters()) == ["conv1.bias", "conv1.weight", "conv2.bias", "conv2.weight", "norm1.bias",
                                                          "norm1.weight", "norm2.bias", "norm2.weight", "out.bias", "out.weight"]
    assert "STOCK TORCH" in VariancePredictor.__doc__
    with pytest.raises(ValueError, match="kernel_size must be odd and positive, got 4"):
        VariancePredictor(16, kernel_size=4)

    class Mean(torch.nn.Module):
        def __init__(self, d_model=16):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(d_model))

        def forward(self, x, phoneme_lens):
            return (x * self.w).mean(-1)

    a = VarianceAdaptor(16, n_bins=8, predictor=Mean())
    assert a.duration_predictor is not a.pitch_predictor and isinstance(a.energy_predictor, Mean)
    b = VarianceAdaptor(16, n_bins=8, predictor=Mean, max_len=50, min_duration=1)
    assert isinstance(b.pitch_predictor, Mean) and b.max_len == 50 and b.min_duration == 1
    c = VarianceAdaptor(16, n_bins=8)
    assert isinstance(c.duration_predictor, VariancePredictor) and c.embedding.pitch_table.shape == (8, 16)
    names = sorted(k.split(".")[0] for k, _ in c.named_parameters())
    assert set(names) == {"duration_predictor", "pitch_predictor", "energy_predictor", "embedding"}
    with pytest.raises(ValueError, match="predictor must be None, a module or a callable"):
        VarianceAdaptor(16, predictor=3)
    with pytest.raises(ValueError, match=re.escape("VarianceAdaptor: max_len must be an integer in [1, 2^20] frames, got 0")):
        VarianceAdaptor(16, n_bins=8, max_len=0)
    with pytest.raises(ValueError, match=re.escape("variance_embed.x: expected a CUDA/HIP tensor")):
        a(torch.zeros(1, 3, 16), torch.tensor([3]))
    assert HUGE > 1 << 62
