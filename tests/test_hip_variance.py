"""Variance adaptor on the device (csrc/variance.hip through transformertts_amd/variance.py) against the oracles of
tests/variance_reference.py.  The regulator, the embedding and every gradient are held bit for bit to the stock fp32 forms in the
kernels' stated order, and to 1e-6 relative of fp64 where they sum; the loss terms to 4 x the stock form's own error (DESIGN.md 25
"Errors"), floored at one fp32 ulp of the value.  NaN (a NaN's bits in the durations) sits behind every length.  The shapes are
the smallest that reach every path: D of 4, 36, 256, 384 (one lane per row up to 64 lanes walking a row twice), Pmax of 1, 70,
300 (across a 64-phoneme scan tile, across 256 threads), Tmax no multiple of the 32 frames a workgroup owns.  Measured values:
parity_reports/variance_margin.txt (as measured on one MI355X: tests/reports/variance_margin.txt)."""
import functools
import os

import numpy as np
import pytest
import torch

from test_hip_dropout_parity import REPORT_DIR
from variance_reference import (HUGE, durations_from_log_ref, embedding_bwd_ref, embedding_bwd_stock, length_regulate_bwd_stock,
                                length_regulate_ref, length_regulate_transpose_ref, poison, variance_embed_ref, variance_loss_grad_ref,
                                variance_loss_grad_stock, variance_loss_ref, variance_loss_stock)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# name -> B, Pmax, D, Tmax, phoneme_lens, (row stride, batch stride) of x or None
REGULATOR = {
    "one_phoneme_d4": (1, 1, 4, 7, (1,), None),
    "tile_edge_d36": (3, 70, 36, 100, (70, 12, 0), None),             # utterance 0 overshoots Tmax: clipped; utterance 1 falls short
    "threads_edge_d256": (3, 300, 256, 333, (300, 257, 64), None),    # every sum falls short of Tmax: zeros behind
    "strided_d384": (2, 70, 384, 75, (66, 70), (388, 70 * 388 + 8)),
    "long_d4": (1, 300, 4, 1030, (300,), None),
    "all_zero_d36": (2, 5, 36, 33, (5, 3), None),
}


def _report(line):
    print(line)
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(f"{REPORT_DIR}/variance_margin.txt", "a") as f:
        f.write(line + "\n")


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _reg_case(name):
    """inputs with NaN behind every length, the oracle's forward, an upstream gradient and both forms of the transpose (computed
    once, never modified)"""
    B, Pmax, D, Tmax, lens, strides = REGULATOR[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    x, dur, _, _ = poison(rng, B, Pmax, D, lens)
    if name == "all_zero_d36":
        dur[:, :] = np.where(dur == HUGE, HUGE, 0)
    elif name == "threads_edge_d256":
        dur = np.where(dur == HUGE, HUGE, dur % 2)                    # about 150 frames per utterance
        dur[0, 299] = 0
    elif Pmax >= 70:
        dur[0, 0], dur[0, 1], dur[0, 30:33], dur[0, lens[0] - 1] = 0, 0, 0, 0      # zeros at the start, in the middle, at the end
        dur[0, 5] = 40                                                # longer than the 32 frames of a workgroup
        dur[0, 7] = -3                                                # negative: counts as 0
    y, frames, index = length_regulate_ref(x, dur, lens, Tmax)
    dy = rng.standard_normal((B, Tmax, D)).astype(np.float32)
    dy[0, Tmax - 1] = np.float32(1e4)                                 # (a large row: the order of a sum shows)
    return dict(x=x, dur=dur, lens=np.array(lens, np.int64), y=y, frames=frames, index=index, dy=dy,
                stock=length_regulate_bwd_stock(dy, dur, lens, Pmax), ref=length_regulate_transpose_ref(dy, dur, lens, Pmax))


def _device_x(name, requires_grad=False):
    B, Pmax, D, Tmax, lens, strides = REGULATOR[name]
    x = torch.from_numpy(_reg_case(name)["x"]).to(DEV)
    if strides is not None:
        ld_row, ld_batch = strides
        store = torch.full((B * ld_batch,), float("nan"), device=DEV)
        view = store.as_strided((B, Pmax, D), (ld_batch, ld_row, 1))
        view.copy_(x)
        x = view
    return x.requires_grad_(True) if requires_grad else x


@pytest.mark.parametrize("name", list(REGULATOR))
def test_the_regulator_forward_is_the_oracles_bit_for_bit(name):
    from transformertts_amd import length_regulate
    B, Pmax, D, Tmax, lens, strides = REGULATOR[name]
    c = _reg_case(name)
    x = _device_x(name)
    out = length_regulate(x, torch.from_numpy(c["dur"]).to(DEV), torch.from_numpy(c["lens"]).to(DEV), Tmax)
    torch.cuda.synchronize()
    assert out["frames"].dtype == torch.float32 and out["mel_lens"].dtype == torch.int64 and out["index"].dtype == torch.int32
    assert tuple(out["frames"].shape) == (B, Tmax, D) and tuple(out["index"].shape) == (B, Tmax)
    assert np.array_equal(out["mel_lens"].cpu().numpy(), c["frames"]) and np.array_equal(out["index"].cpu().numpy(), c["index"])
    assert _same_bits(out["frames"], c["y"]) and not bool(torch.isnan(out["frames"]).any())
    if name == "tile_edge_d36":
        assert c["frames"].tolist()[0] == Tmax and 0 < c["frames"][1] < Tmax and c["frames"][2] == 0
        assert (c["index"][0] == 5).sum() == 40
    if name == "all_zero_d36":
        assert not bool(out["frames"].any()) and bool((out["index"] == -1).all()) and not bool(out["mel_lens"].any())
    if name == "threads_edge_d256":
        assert (c["frames"] < Tmax).all() and c["index"][0].max() > 256
    if name == "strided_d384":
        assert not x.is_contiguous()


@pytest.mark.parametrize("name", list(REGULATOR))
def test_the_regulator_backward_is_the_sequential_sum_bit_for_bit(name):
    from transformertts_amd import _lib, length_regulate
    from transformertts_amd.ops import _p, _stream
    B, Pmax, D, Tmax, lens, strides = REGULATOR[name]
    c = _reg_case(name)
    x = _device_x(name, requires_grad=True)
    dur, pl = torch.from_numpy(c["dur"]).to(DEV), torch.from_numpy(c["lens"]).to(DEV)
    out = length_regulate(x, dur, pl, Tmax)
    dy = torch.from_numpy(c["dy"]).to(DEV)
    wide = torch.zeros(B, Tmax, 2 * D, device=DEV)                    # the upstream gradient as a view: made contiguous inside
    wide[:, :, :D] = dy
    (g,) = torch.autograd.grad(out["frames"], x, wide[:, :, :D])
    torch.cuda.synchronize()
    got = g.cpu().numpy()
    assert _same_bits(got, c["stock"])                                # through autograd, accumulate off
    scale = max(float(np.abs(c["ref"]).max()), 1e-30)
    err = float(np.abs(got - c["ref"]).max()) / scale
    _report(f"regulator backward {name}: max-abs error over max|fp64| {err:.3e} (stock {float(np.abs(c['stock'] - c['ref']).max()) / scale:.3e})")
    assert err <= 1e-6
    into = np.random.default_rng(5).standard_normal((B, Pmax, D)).astype(np.float32)
    for accumulate, want in ((1, into + c["stock"]), (0, c["stock"])):
        dx = torch.from_numpy(into).to(DEV)
        _lib.check(_lib.load().ttts_length_regulate_bwd(_p(dy), _p(dur), _p(pl), B, Pmax, Tmax, D, _p(dx), accumulate, _stream()), "bwd")
        torch.cuda.synchronize()
        assert _same_bits(dx, want), accumulate
    for b, n in enumerate(lens):                                      # exact zeros behind the length and for a phoneme without a frame
        assert not got[b, n:].any() and not got[b, :n][np.maximum(c["dur"][b, :n], 0) == 0].any()


def test_max_len_none_reads_the_longest_sum_once():
    from transformertts_amd import LengthRegulator
    c = _reg_case("tile_edge_d36")
    x, dur, pl = _device_x("tile_edge_d36"), torch.from_numpy(c["dur"]).to(DEV), torch.from_numpy(c["lens"])
    out = LengthRegulator()(x, dur, pl)                               # host lengths are moved; HUGE behind the lengths is not summed
    total = int(np.maximum(c["dur"][0, :70], 0).sum())
    assert tuple(out["frames"].shape) == (3, total, 36) and int(out["mel_lens"].max()) == total
    y, frames, index = length_regulate_ref(c["x"], c["dur"], c["lens"], total)
    assert _same_bits(out["frames"], y) and np.array_equal(out["index"].cpu().numpy(), index)
    assert tuple(LengthRegulator(50)(x, dur, pl)["frames"].shape) == (3, 50, 36)


def test_durations_from_log_is_the_oracles():
    from transformertts_amd import durations_from_log
    rng = np.random.default_rng(7)
    B, Pmax, lens = 3, 300, (300, 70, 0)
    log_d = (rng.standard_normal((B, Pmax)) * 1.5 + 1.0).astype(np.float32)
    special = [2.0 ** -30, 0.0, -0.0, np.nan, np.inf, -np.inf, -50.0, -1e30, 100.0, 1e30, np.log(2.0), np.log(1.5), np.log(2.5), np.log(3.5),
               88.7, 89.0, 21.5, 1e-8, -1e-8]
    log_d[0, :len(special)] = np.array(special, np.float32)
    log_d[1, :len(special)] = np.array(special, np.float32)
    for b, n in enumerate(lens):
        log_d[b, n:] = np.nan
    dev, pl = torch.from_numpy(log_d).to(DEV), torch.tensor(lens, device=DEV)
    for alpha, min_duration in ((1.0, 0), (2.0 ** 29, 0), (3 * 2.0 ** 29, 0), (5 * 2.0 ** 29, 1), (0.5, 0), (1.5, 2), (2.5, 0), (0.75, 0)):
        got = durations_from_log(dev, pl, alpha=alpha, min_duration=min_duration)
        torch.cuda.synchronize()
        want = durations_from_log_ref(log_d, lens, alpha, min_duration)
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want), (alpha, min_duration)
        assert not want[2].any() and not want[1, 70:].any()
    halves = [int(durations_from_log_ref(log_d, lens, k * 2.0 ** 29)[0, 0]) for k in (1, 3, 5)]
    assert halves == [0, 2, 2]                                        # exp(2^-30) - 1 = 2^-30 in fp64: exactly 0.5, 1.5, 2.5
    assert durations_from_log_ref(log_d, lens)[0, 3:10].tolist() == [0, 0, 0, 0, 0, 2 ** 31 - 1, 2 ** 31 - 1]


EMBED = {"np2_d4": (1, 5, 4, (5,), 2, 2, None), "np256_d36": (3, 70, 36, (70, 33, 0), 256, 7, None),
         "np256_d384_strided": (2, 40, 384, (40, 9), 256, 256, (388, 40 * 388 + 8))}


@functools.lru_cache(maxsize=None)
def _embed_case(name):
    B, Pmax, D, lens, n_p, n_e, strides = EMBED[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    x, _, pitch, energy = poison(rng, B, Pmax, D, lens)
    pb = np.exp(np.linspace(np.log(65.0), np.log(600.0), n_p - 1)).astype(np.float32)
    eb = np.linspace(0.0, 1.0, n_e - 1).astype(np.float32)
    k = min(lens[0], 5)
    pitch[0, :k] = np.array([pb[0], pb[-1], 10.0, 1e4, pb[(n_p - 2) // 2]], np.float32)[:k]       # on a boundary, below the first, above the last
    energy[0, :k] = np.array([eb[-1], eb[0], -1.0, 2.0, eb[(n_e - 2) // 2]], np.float32)[:k]
    Ep, Ee = rng.standard_normal((n_p, D)).astype(np.float32), rng.standard_normal((n_e, D)).astype(np.float32)
    dy = rng.standard_normal((B, Pmax, D)).astype(np.float32)
    return dict(x=x, pitch=pitch, energy=energy, pb=pb, eb=eb, Ep=Ep, Ee=Ee, dy=dy, lens=np.array(lens, np.int64))


@pytest.mark.parametrize("name", list(EMBED))
@pytest.mark.parametrize("features", ["both", "pitch", "energy"])
def test_the_embedding_and_its_table_gradients_bit_for_bit(name, features):
    from transformertts_amd import variance_embed
    B, Pmax, D, lens, n_p, n_e, strides = EMBED[name]
    c = _embed_case(name)
    x = torch.from_numpy(c["x"]).to(DEV)
    if strides is not None:
        store = torch.full((B * strides[1],), float("nan"), device=DEV)
        view = store.as_strided((B, Pmax, D), (strides[1], strides[0], 1))
        view.copy_(x)
        x = view
    x.requires_grad_(True)
    kw, ref_kw, tables = {}, {}, {}
    if features in ("both", "pitch"):
        tables["pitch"] = torch.from_numpy(c["Ep"]).to(DEV).requires_grad_(True)
        kw.update(pitch=torch.from_numpy(c["pitch"]).to(DEV), pitch_bins=torch.from_numpy(c["pb"]).to(DEV), pitch_table=tables["pitch"])
        ref_kw.update(pitch=c["pitch"], pitch_bins=c["pb"], Ep=c["Ep"])
    if features in ("both", "energy"):
        tables["energy"] = torch.from_numpy(c["Ee"]).to(DEV).requires_grad_(True)
        kw.update(energy=torch.from_numpy(c["energy"]).to(DEV), energy_bins=torch.from_numpy(c["eb"]).to(DEV), energy_table=tables["energy"])
        ref_kw.update(energy=c["energy"], energy_bins=c["eb"], Ee=c["Ee"])
    out = variance_embed(x, torch.from_numpy(c["lens"]).to(DEV), **kw)
    torch.cuda.synchronize()
    stock, i, j = variance_embed_ref(c["x"], lens, dtype=np.float32, **ref_kw)
    ref, _, _ = variance_embed_ref(c["x"], lens, **ref_kw)
    assert _same_bits(out["x"], stock)                                # (x + Ep[i]) + Ee[j] in that order; x itself, NaN and all, behind the length
    for b, n in enumerate(lens):
        assert n == 0 or (not np.isnan(stock[b, :n]).any() and np.abs(stock[b, :n] - ref[b, :n]).max() <= 1e-6 * np.abs(ref[b, :n]).max())
    for key, ids in (("pitch_ids", i), ("energy_ids", j)):
        if ids is None:
            assert out[key] is None
            continue
        assert out[key].dtype == torch.int64 and np.array_equal(out[key].cpu().numpy(), ids)
        assert all((ids[b, n:] == -1).all() and (ids[b, :n] >= 0).all() for b, n in enumerate(lens))
    if features != "energy" and n_p > 2 and lens[0] >= 5:
        assert i[0, :5].tolist() == [0, n_p - 2, 0, n_p - 1, (n_p - 2) // 2]      # a value on a boundary belongs to the bucket below
    dy = torch.from_numpy(c["dy"]).to(DEV)
    grads = torch.autograd.grad(out["x"], [x] + list(tables.values()), dy)
    torch.cuda.synchronize()
    assert _same_bits(grads[0], c["dy"])                              # dx is dy itself
    for (key, table), g, ids in zip(tables.items(), grads[1:], [t for t in (i, j) if t is not None]):
        n = table.size(0)
        want, want64 = embedding_bwd_stock(ids, c["dy"], n), embedding_bwd_ref(ids, c["dy"], n)
        assert _same_bits(g, want), key
        err = float(np.abs(g.cpu().numpy() - want64).max() / np.abs(want64).max())
        _report(f"embedding table gradient {name} {features} {key}: max-abs error over max|fp64| {err:.3e}")
        assert err <= 1e-6


def test_the_embedding_module_skips_a_feature_it_is_not_given():
    from transformertts_amd import VarianceEmbedding
    c = _embed_case("np256_d36")
    m = VarianceEmbedding(256, 7, 36, pitch_bins=c["pb"], energy_bins=c["eb"]).to(DEV)
    with torch.no_grad():
        m.pitch_table.copy_(torch.from_numpy(c["Ep"]))
        m.energy_table.copy_(torch.from_numpy(c["Ee"]))
    x, pl = torch.from_numpy(c["x"]).to(DEV), torch.from_numpy(c["lens"]).to(DEV)
    both = m(x, pl, pitch=torch.from_numpy(c["pitch"]).to(DEV), energy=torch.from_numpy(c["energy"]).to(DEV), return_ids=True)
    want, i, j = variance_embed_ref(c["x"], c["lens"], c["pitch"], c["pb"], c["Ep"], c["energy"], c["eb"], c["Ee"], dtype=np.float32)
    assert _same_bits(both["x"], want) and np.array_equal(both["pitch_ids"].cpu().numpy(), i)
    only = m(x, pl, energy=torch.from_numpy(c["energy"]).to(DEV))
    want, _, _ = variance_embed_ref(c["x"], c["lens"], energy=c["energy"], energy_bins=c["eb"], Ee=c["Ee"], dtype=np.float32)
    assert _same_bits(only, want) and _same_bits(m(x, pl), c["x"])


LOSS = {"two_passes": (3, 700, (700, 401, 0)), "small": (2, 5, (5, 2)), "one": (1, 1, (1,))}


@functools.lru_cache(maxsize=None)
def _loss_case(name):
    B, Pmax, lens = LOSS[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    _, dur, pitch, energy = poison(rng, B, Pmax, 4, lens)
    dur[0, 0] = -4
    pitch = (pitch / 100).astype(np.float32)
    preds = [rng.standard_normal((B, Pmax)).astype(np.float32) for _ in range(3)]
    return dict(args=(preds[0], dur, preds[1], pitch, preds[2], energy, lens))


def _run_loss(args, weights, coef):
    from transformertts_amd import VarianceLoss
    log_d, dur, pp, pitch, ep, energy, lens = args
    t = lambda a, grad=False: torch.from_numpy(a).to(DEV).requires_grad_(grad)
    pred = {"log_duration": t(log_d, True), "pitch": t(pp, True), "energy": t(ep, True)}
    out = VarianceLoss(weights)(pred, t(dur), t(pitch), t(energy), torch.tensor(lens, device=DEV))
    vec = torch.stack([out["duration"], out["pitch"], out["energy"], out["total"]])
    grads = torch.autograd.grad(vec, list(pred.values()), torch.tensor(coef, device=DEV))
    torch.cuda.synchronize()
    return vec.detach().cpu().numpy(), [g.cpu().numpy() for g in grads]


@pytest.mark.parametrize("name", list(LOSS))
def test_the_losses_within_four_times_the_stock_forms_error_and_their_gradients_bit_for_bit(name):
    B, Pmax, lens = LOSS[name]
    args = _loss_case(name)["args"]
    valid = np.arange(Pmax)[None, :] < np.array(lens)[:, None]
    for weights, coef in (((1.0, 1.0, 1.0), (0.0, 0.0, 0.0, 1.0)), ((1.0, 0.5, 2.0), (0.25, -1.0, 0.0, 1.5))):
        got, grads = _run_loss(args, weights, coef)
        ref, stock = variance_loss_ref(*args, weights=weights), variance_loss_stock(*args, weights=weights)
        assert got.dtype == np.float32
        for k, term in enumerate(("duration", "pitch", "energy", "total")):
            ulp = float(np.spacing(np.float32(abs(ref[k]))))
            bound = 4 * max(abs(float(stock[k]) - ref[k]), ulp)
            err = abs(float(got[k]) - ref[k])
            _report(f"loss {name} weights {weights} {term}: value {ref[k]:.9e} error {err:.3e} stock form {abs(float(stock[k]) - ref[k]):.3e} "
                    f"ulp {ulp:.3e} bound {bound:.3e} same bits as the stock form: {bool(_same_bits(got[k:k + 1], stock[k:k + 1]))}")
            assert err <= bound, term
        want = variance_loss_grad_stock(*args, weights, coef)
        want64 = variance_loss_grad_ref(*args, weights, coef)
        for g, w, w64 in zip(grads, want, want64):
            assert _same_bits(g, w) and not g[~valid].any()
            assert np.abs(g - w64).max() <= 1e-6 * max(np.abs(w64).max(), 1e-30)


def test_an_all_empty_batch_gives_exact_zeros():
    args = list(_loss_case("small")["args"])
    args[6] = (0, 0)
    got, grads = _run_loss(tuple(args), (1.0, 1.0, 1.0), (1.0, 1.0, 1.0, 1.0))
    assert _same_bits(got, np.zeros(4, np.float32)) and all(_same_bits(g, np.zeros((2, 5), np.float32)) for g in grads)


def test_the_same_bits_whatever_the_call_or_the_neighbours():
    from transformertts_amd import length_regulate, variance_embed
    name = "tile_edge_d36"
    B, Pmax, D, Tmax, lens, _ = REGULATOR[name]
    c = _reg_case(name)
    e = _embed_case("np256_d36")

    def run(x, dur, pl, pitch, energy, dy):
        x = torch.from_numpy(x).to(DEV).requires_grad_(True)
        emb = variance_embed(x, torch.from_numpy(pl).to(DEV), torch.from_numpy(pitch).to(DEV), torch.from_numpy(e["pb"]).to(DEV),
                             torch.from_numpy(e["Ep"]).to(DEV), torch.from_numpy(energy).to(DEV), torch.from_numpy(e["eb"]).to(DEV),
                             torch.from_numpy(e["Ee"]).to(DEV))
        out = length_regulate(emb["x"], torch.from_numpy(dur).to(DEV), torch.from_numpy(pl).to(DEV), Tmax)
        (g,) = torch.autograd.grad(out["frames"], x, torch.from_numpy(dy).to(DEV))
        torch.cuda.synchronize()
        return [t.detach().cpu().numpy() for t in (emb["x"], emb["pitch_ids"], emb["energy_ids"], out["frames"], out["mel_lens"], out["index"], g)]

    first = run(c["x"], c["dur"], c["lens"], e["pitch"], e["energy"], c["dy"])
    again = run(c["x"], c["dur"], c["lens"], e["pitch"], e["energy"], c["dy"])
    assert all(_same_bits(a, b) for a, b in zip(first, again))
    rng = np.random.default_rng(11)                                   # five utterances: the three at positions 3, 0, 4 among others
    place = (3, 0, 4)
    wx, wdur, wpitch, wenergy = poison(rng, 5, Pmax, D, (Pmax, 12, Pmax, Pmax, Pmax))
    wdy, wpl = rng.standard_normal((5, Tmax, D)).astype(np.float32), np.array([Pmax, 12, Pmax, Pmax, Pmax], np.int64)
    wpitch[1, :12], wenergy[1, :12] = 100.0, 0.5
    for b, at in enumerate(place):
        wx[at], wdur[at], wpitch[at], wenergy[at], wdy[at], wpl[at] = c["x"][b], c["dur"][b], e["pitch"][b], e["energy"][b], c["dy"][b], c["lens"][b]
    wide = run(wx, wdur, wpl, wpitch, wenergy, wdy)
    for b, at in enumerate(place):
        assert all(_same_bits(w[at], f[b]) for w, f in zip(wide, first)), b


def _adaptor(d_model=16, n_bins=8, max_len=None):
    from transformertts_amd import VarianceAdaptor, variance_bins
    torch.manual_seed(3)
    a = VarianceAdaptor(d_model, n_bins=n_bins, pitch_bins=variance_bins(-1.0, 1.0, n_bins), energy_bins=variance_bins(-1.0, 1.0, n_bins),
                        min_duration=1, max_len=max_len).to(DEV)
    with torch.no_grad():
        a.duration_predictor.out.bias.fill_(1.2)                      # durations of about exp(1.2) - 1 = 2.3 frames
    return a


def test_a_captured_inference_call_replayed_on_another_input():
    a = _adaptor(max_len=48).eval()
    gen = torch.Generator().manual_seed(9)
    x0, x1 = torch.randn(2, 11, 16, generator=gen).to(DEV), torch.randn(2, 11, 16, generator=gen).to(DEV) * 2.0
    static, pl = x0.clone(), torch.tensor([11, 6], device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():                    # (warm-up: the library is loaded, the allocator primed)
        a(static, pl, d_control=1.25)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        got = a(static, pl, d_control=1.25)
    seen = []
    for x in (x0, x1):
        static.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        with torch.no_grad():
            eager = a(x.clone(), pl, d_control=1.25)
        torch.cuda.synchronize()
        for k in ("frames", "mel_lens", "index", "log_duration", "pitch", "energy", "durations"):
            assert _same_bits(got[k], eager[k]), k
        assert int(got["mel_lens"].min()) >= 6 and bool((got["durations"][1, 6:] == 0).all())
        seen.append(got["frames"].clone())
    assert not torch.equal(seen[0], seen[1])                          # the replay did follow the input
    from transformertts_amd import length_regulate
    dur = torch.ones(2, 11, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="max_len=None reads the durations back to the host and cannot be captured"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            length_regulate(static, dur, pl)                          # refused in front of the host read: nothing was captured


def test_the_chain_from_teacher_durations_to_the_variance_losses():
    from oracle import synth_batch
    from pitch_reference import SMALL, glide_signal
    from test_hip_model import _build
    from test_hip_pitch import _config
    from transformertts_amd import PitchEnergy, VarianceLoss, phoneme_average, teacher_durations
    cfg, m = _build("tiny", 11)
    batch = synth_batch(3, 12, 40, cfg["n_mels"], cfg["n_phon"], ragged=True, seed=21)
    args = [batch[k].to(DEV) for k in ("phoneme", "melspec", "phoneme_lens", "melspec_lens")]
    dur = teacher_durations(m, *args, method="mas")["durations"]
    hop = SMALL["hop_length"]
    n = [(int(t) - 1) * hop + hop // 2 for t in batch["melspec_lens"]]            # 1 + n // hop frames: the mel's
    wave = np.zeros((3, max(n)), np.float32)
    for b, k in enumerate(n):
        wave[b, :k] = glide_signal(k, SMALL, 60 + b)
    pe = PitchEnergy(_config(SMALL), fmin=SMALL["fmin"], fmax=SMALL["fmax"], frame_length=SMALL["frame_length"], window=SMALL["window"], device=DEV)
    fr = pe(torch.from_numpy(wave).to(DEV), torch.tensor(n, device=DEV))
    assert torch.equal(fr["frames"], args[3].to(torch.int64))
    pitch = phoneme_average(fr["f0"], dur, args[2], fr["frames"], mask=fr["voiced"])["mean"] / 200.0 - 1.0
    energy = phoneme_average(fr["energy"], dur, args[2], fr["frames"])["mean"] / 10.0 - 1.0
    a = _adaptor().train()
    x = torch.randn(3, 12, 16, generator=torch.Generator().manual_seed(2)).to(DEV).requires_grad_(True)
    out = a(x, args[2], durations=dur, pitch=pitch, energy=energy, max_len=40)
    loss = VarianceLoss((1.0, 0.5, 0.5))(out, dur, pitch, energy, args[2])
    (loss["total"] + out["frames"].square().mean()).backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss["total"])) and float(loss["total"].detach()) > 0
    for name, p in a.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    assert bool(a.embedding.pitch_table.grad.any()) and bool(a.embedding.energy_table.grad.any()) and bool(torch.isfinite(x.grad).all())
    total = torch.where(torch.arange(12, device=DEV)[None, :] < args[2][:, None], dur, torch.zeros_like(dur)).sum(1).clamp(max=40)
    assert torch.equal(out["mel_lens"], total.to(torch.int64)) and out["durations"] is dur
    rows = (out["index"] >= 0).sum(1)
    assert torch.equal(rows, out["mel_lens"])                         # as many regulated rows as mel_lens says, zeros behind them
    for b in range(3):
        assert not bool(out["frames"][b, int(rows[b]):].any()) and bool(out["frames"][b, :int(rows[b])].abs().sum(1).gt(0).all())
    valid = batch["melspec_lens"] >= batch["phoneme_lens"]
    assert bool(valid.any()) and torch.equal(out["mel_lens"].cpu()[valid], batch["melspec_lens"][valid].to(torch.int64))      # MAS tiles the frames
