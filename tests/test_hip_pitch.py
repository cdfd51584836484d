"""Frame pitch and energy on the GPU (csrc/pitch.hip, transformertts_amd.audio.PitchEnergy / phoneme_average) against the fp64
oracle of tests/pitch_reference.py.  A frame counts as decided when the oracle's decision margin exceeds m = 8 x the largest
|d'| error of the stock fp32 form on the same input; on decided frames `voiced` must be equal and f0 within the bound, and
aperiodicity and energy within the bound on every frame.  The bound is the project's: 4 x the stock fp32 form's own error against
the oracle on the same input, and never looser than 1e-4 relative (0.17 cent for f0).  At most 5 % of an input's frames may be
undecided.  Then: reads inside the lengths (NaN behind them), zeros behind the frames, silence, the two ends of the lag range,
an empty utterance, the same bits across calls, views, batches and a captured call, the front end's frame count and
spectrogram, the phoneme means, and the chain from teacher_durations.  Measured values: parity_reports/pitch_margin.txt (as
measured on one MI355X: tests/reports/pitch_margin.txt)."""
import functools
import os

import numpy as np
import pytest
import torch

from pitch_reference import (LONG_LAGS, ODD_WINDOW, SHIPPED, SHORT_FRAME, SMALL, THRESHOLD, cents, energy_ref, frame_count_ref, glide_signal, lags_ref,
                             pitch_ref, pitch_stock, segment_mean_ref)
from test_hip_dropout_parity import REPORT_DIR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 37
CENT_1E4 = 1200.0 * np.log2(1.0 + 1e-4)                                      # 1e-4 relative in cents: 0.173
# name -> (shape, lengths): small has F/2 + 1 (one frame short of refusal), a multiple of hop, one less, about 1 s; shipped is
# where tau_max = 340 exceeds one pass of 256 threads; odd_window has W no multiple of hop; short_frame has F < n_fft; long_lags
# has F > n_fft and 2000 lags, so that a workgroup holds two frames, unshared partials, and runs two waves in its second phase
CASES = {"small": (SMALL, (129, 640, 639, 8000)), "shipped": (SHIPPED, (11025, 7000, 4096)),
         "odd_window": (ODD_WINDOW, (3000, 1000, 129)), "short_frame": (SHORT_FRAME, (3000, 257)),
         "long_lags": (LONG_LAGS, (2049, 9000, 6000))}


def _config(p):
    return dict(sample_rate=p["sample_rate"], n_fft=p["n_fft"], hop_length=p["hop_length"], win_length=p["win_length"], n_mels=20,
                fmin=0.0, fmax=p["sample_rate"] / 2.0)


@functools.lru_cache(maxsize=None)
def _pe(name):
    from transformertts_amd.audio import PitchEnergy
    p = CASES[name][0]
    return PitchEnergy(_config(p), fmin=p["fmin"], fmax=p["fmax"], frame_length=p["frame_length"], window=p["window"],
                       threshold=THRESHOLD, device=DEV)


@functools.lru_cache(maxsize=None)
def _case(name):
    """the ragged batch of a shape with NaN behind every length, the oracle and the stock form per utterance (computed once,
    never modified) and the stock form's errors"""
    p, lens = CASES[name]
    wave = np.full((len(lens), max(lens) + PAD), np.nan, dtype=np.float32)
    refs, stocks, energies = [], [], []
    for b, n in enumerate(lens):
        x = glide_signal(n, p, 10 + b)
        wave[b, :n] = x
        refs.append(pitch_ref(x, p))
        stocks.append(pitch_stock(x, p))
        energies.append(energy_ref(x, p))
    dp_err = max(float(np.abs(s["dprime"] - r["dprime"]).max()) for s, r in zip(stocks, refs))
    m = 8.0 * dp_err
    f0_err = ap_err = en_err = 0.0
    for s, r, e in zip(stocks, refs, energies):
        v = (r["margin"] > m) & r["voiced"] & s["voiced"]
        if v.any():
            f0_err = max(f0_err, float(cents(s["f0"][v], r["f0"][v]).max()))
        ap_err = max(ap_err, float(np.abs(s["aperiodicity"] - r["aperiodicity"]).max()))
        en_err = max(en_err, float(np.abs(s["energy"] - e).max()))
    for r in refs:
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return dict(p=p, lens=lens, wave=wave, refs=refs, energies=energies, m=m, dp_err=dp_err, f0_err=f0_err, ap_err=ap_err, en_err=en_err)


def _run(name, wave=None, lens=None):
    case = _case(name)
    wave = torch.from_numpy(case["wave"]).to(DEV) if wave is None else wave
    lens = torch.tensor(case["lens"], device=DEV) if lens is None else lens
    out = _pe(name)(wave, lens)
    torch.cuda.synchronize()
    return out


def _same(a, b, rows=None):
    for k in ("f0", "voiced", "aperiodicity", "energy", "frames"):
        x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
        assert torch.equal(x.cpu(), y.cpu()), k


@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_the_fp64_oracle(name):
    case = _case(name)
    p, m = case["p"], case["m"]
    out = {k: v.cpu().numpy() for k, v in _run(name).items()}
    Tmax = 1 + case["wave"].shape[1] // p["hop_length"]
    assert out["f0"].shape == out["voiced"].shape == out["aperiodicity"].shape == out["energy"].shape == (len(case["lens"]), Tmax)
    assert out["voiced"].dtype == np.bool_ and out["frames"].dtype == np.int64
    assert out["frames"].tolist() == [frame_count_ref(n, p) for n in case["lens"]] == [r["frames"] for r in case["refs"]]
    worst = dict(f0=0.0, ap=0.0, en=0.0)
    ap_num = ap_den = en_num = en_den = 0.0
    total = undecided = 0
    for b, (r, e) in enumerate(zip(case["refs"], case["energies"])):
        T = r["frames"]
        for k in ("f0", "aperiodicity", "energy"):
            assert np.isfinite(out[k][b]).all() and (out[k][b, T:] == 0).all(), (k, b)      # nothing behind a length was read
        assert not out["voiced"][b, T:].any()
        ok = r["margin"] > m
        total, undecided = total + T, undecided + int((~ok).sum())
        assert (out["voiced"][b, :T][ok] == r["voiced"][ok]).all(), b
        assert (out["f0"][b, :T][~out["voiced"][b, :T]] == 0).all()
        v = ok & r["voiced"]
        if v.any():
            worst["f0"] = max(worst["f0"], float(cents(out["f0"][b, :T][v], r["f0"][v]).max()))
        da, de = out["aperiodicity"][b, :T].astype(np.float64) - r["aperiodicity"], out["energy"][b, :T].astype(np.float64) - e
        worst["ap"], worst["en"] = max(worst["ap"], float(np.abs(da).max())), max(worst["en"], float(np.abs(de).max()))
        ap_num, ap_den, en_num, en_den = ap_num + (da ** 2).sum(), ap_den + (r["aperiodicity"] ** 2).sum(), en_num + (de ** 2).sum(), \
            en_den + (e ** 2).sum()
    ap_rel, en_rel = float(np.sqrt(ap_num / ap_den)), float(np.sqrt(en_num / en_den))
    line = (f"{name}: frames {total} undecided {undecided} m {m:.3e} (stock |d'| error {case['dp_err']:.3e}); f0 {worst['f0']:.3e} cent "
            f"(stock {case['f0_err']:.3e}); aperiodicity max-abs {worst['ap']:.3e} (stock {case['ap_err']:.3e}) rel-L2 {ap_rel:.3e}; "
            f"energy max-abs {worst['en']:.3e} (stock {case['en_err']:.3e}) rel-L2 {en_rel:.3e}")
    print(line)
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(f"{REPORT_DIR}/pitch_margin.txt", "a") as f:
        f.write(line + "\n")
    assert undecided <= 0.05 * total                                         # a signal that hides frames fails here
    assert worst["f0"] <= min(4 * case["f0_err"], CENT_1E4)
    assert worst["ap"] <= 4 * case["ap_err"] and ap_rel <= 1e-4
    assert worst["en"] <= 4 * case["en_err"] and en_rel <= 1e-4


def test_silence_is_unvoiced_with_aperiodicity_one():
    p = SMALL
    wave = torch.zeros(2, 2000, device=DEV)
    out = _run("small", wave, torch.tensor([2000, 700], device=DEV))
    for b, n in enumerate((2000, 700)):
        T = frame_count_ref(n, p)
        assert int(out["frames"][b]) == T
        assert not bool(out["voiced"][b].any()) and bool((out["f0"][b] == 0).all()) and bool((out["energy"][b] == 0).all())
        assert bool((out["aperiodicity"][b, :T] == 1).all()) and bool((out["aperiodicity"][b, T:] == 0).all())


@pytest.mark.parametrize("name", ["small", "shipped"])
def test_sines_at_the_two_ends_of_the_lag_range(name):
    p = CASES[name][0]
    tau_min, tau_max = lags_ref(p)
    n = 6 * p["frame_length"]
    t = np.arange(n, dtype=np.float64)
    sig = np.stack([0.4 * np.sin(2 * np.pi * t / tau) for tau in (tau_min + 1, tau_max - 1)]).astype(np.float32)
    out = {k: v.cpu().numpy() for k, v in _run(name, torch.from_numpy(sig).to(DEV), torch.tensor([n, n], device=DEV)).items()}
    for b, tau in enumerate((tau_min + 1, tau_max - 1)):
        r = pitch_ref(sig[b], p)
        T, ok, mid = r["frames"], r["margin"] > 1e-4, slice(3, r["frames"] - 3)
        assert ok[mid].all() and r["voiced"][mid].all() and (r["lag"][mid] == tau).all()      # (the end frames are mostly reflection)
        assert (out["voiced"][b, :T][ok] == r["voiced"][ok]).all()
        v = ok & r["voiced"]
        err = cents(out["f0"][b, :T][v], r["f0"][v]).max()
        print(f"{name}: sine at sr / {tau}: {err:.3e} cent from the oracle")
        assert err <= CENT_1E4
        assert (np.abs(p["sample_rate"] / out["f0"][b, :T][mid].astype(np.float64) - tau) <= 0.5).all()


def test_an_utterance_of_length_zero():
    case = _case("small")
    wave = torch.from_numpy(case["wave"]).to(DEV)
    full = _run("small")
    out = _run("small", wave, torch.tensor([0, 640, -5, 8000], device=DEV))
    assert out["frames"].tolist() == [0, 11, 0, 126]
    for k in ("f0", "aperiodicity", "energy", "voiced"):
        assert not bool(out[k][0].any()) and not bool(out[k][2].any())
    _same(out, full, rows=[1, 3])
    alone = _run("small", torch.full((1, 300), float("nan"), device=DEV), torch.tensor([0], device=DEV))
    assert alone["frames"].tolist() == [0] and not bool(alone["energy"].any()) and not bool(alone["voiced"].any())


@pytest.mark.parametrize("name", ["small", "shipped"])
def test_the_same_bits_whatever_the_call_the_view_or_the_batch(name):
    case = _case(name)
    first = _run(name)
    _same(_run(name), first)
    B, N = case["wave"].shape
    wide = torch.full((B, 2 * N + 3), float("nan"), device=DEV)
    wide[:, :N] = torch.from_numpy(case["wave"]).to(DEV)
    view = wide[:, :N]
    assert not view.is_contiguous()
    _same(_run(name, view, None), first)
    # a wider batch with other neighbours, in another order, in a longer buffer: a frame's bits follow its samples alone
    order = list(range(B))[::-1]
    big = torch.full((2 * B + 1, N + 5 * case["p"]["hop_length"]), float("nan"), device=DEV)
    lens = torch.zeros(2 * B + 1, dtype=torch.int64, device=DEV)
    for i, b in enumerate(order):
        big[2 * i + 1, :N] = view[b]
        lens[2 * i + 1] = case["lens"][b]
        big[2 * i, :case["lens"][0]] = view[0, :case["lens"][0]] * 0.5
        lens[2 * i] = case["lens"][0]
    out = _run(name, big, lens)
    Tmax = first["f0"].size(1)
    for i, b in enumerate(order):
        for k in ("f0", "voiced", "aperiodicity", "energy"):
            assert torch.equal(out[k][2 * i + 1, :Tmax], first[k][b]), (k, b)
            assert not bool(out[k][2 * i + 1, Tmax:].any())
        assert int(out["frames"][2 * i + 1]) == int(first["frames"][b])


def test_a_captured_call_replayed_on_another_waveform():
    case = _case("small")
    pe = _pe("small")
    wave = torch.from_numpy(case["wave"]).to(DEV)
    static, lens = wave.clone(), torch.tensor(case["lens"], device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                             # (warm-up: the library is loaded, the allocator primed)
        pe(static, lens)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = pe(static, lens)
    other = torch.nan_to_num(wave).flip(0).contiguous() * 0.5
    for w in (wave, other):
        static.copy_(w)
        graph.replay()
        torch.cuda.synchronize()
        _same(got, _run("small", w.clone(), lens))
    assert not torch.equal(got["f0"], _run("small")["f0"])                    # the replay did follow the waveform


@pytest.mark.parametrize("name", ["small", "shipped", "short_frame"])
def test_frames_and_energy_are_the_front_ends(name):
    from transformertts_amd.audio import MelFrontEnd, PitchEnergy
    case = _case(name)
    p = case["p"]
    fe = MelFrontEnd(_config(p), device=DEV)
    pe = PitchEnergy(_config(p), fmin=p["fmin"], fmax=p["fmax"], frame_length=p["frame_length"], window=p["window"], front_end=fe)
    assert pe.hann.data_ptr() == fe.tables.data_ptr() + 4 * 8                 # the front end's window section, not a copy
    wave, lens = torch.from_numpy(case["wave"]).to(DEV), torch.tensor(case["lens"], device=DEV)
    out, mag = pe(wave, lens), fe.spectrogram(wave, lens)
    _same(out, _run(name))
    assert torch.equal(out["frames"], mag["melspec_lens"])
    want = mag["spectrogram"].double().norm(dim=2)
    rel = float((out["energy"].double() - want).norm() / want.norm())
    print(f"{name}: energy against the L2 norm of MelFrontEnd.spectrogram rows: rel-L2 {rel:.3e}")
    assert rel <= 1e-5                                                        # two fp32 routes to one number: an FFT and three sums


def _segments(device):
    """durations that sum to, fall short of and overshoot `frames`, a zero-duration phoneme and a phoneme with no voiced frame"""
    out = _run("small")
    frames = out["frames"].cpu()                                              # [3, 11, 10, 126]
    dur = torch.zeros(4, 70, dtype=torch.int64)
    dur[0, :3] = torch.tensor([1, 0, 2])                                      # sums to its 3 frames, with a zero-duration phoneme
    dur[1, :4] = torch.tensor([2, 3, 0, 2])                                   # falls short of 11
    dur[2, :5] = torch.tensor([4, 4, 4, 4, 4])                                # overshoots 10: the third is cut, two get nothing
    gen = torch.Generator().manual_seed(5)
    dur[3, :66] = torch.randint(0, 4, (66,), generator=gen)                   # more than one tile of 64 phonemes
    dur[3, 66:] = 7                                                           # ... behind phoneme_lens: never counted
    plens = torch.tensor([3, 4, 5, 66])
    return out, dur.to(device), plens.to(device), frames


def test_phoneme_average_against_the_reference():
    from transformertts_amd.audio import phoneme_average
    out, dur, plens, frames = _segments(DEV)
    f0, voiced, energy = out["f0"].cpu().numpy(), out["voiced"].cpu().numpy(), out["energy"].cpu().numpy()
    assert not voiced[0].any()                                                # utterance 0 (three frames, mostly reflection) has no voiced frame
    for values, mask, vm in ((out["f0"], out["voiced"], (f0, voiced)), (out["energy"], None, (energy, None)),
                             (out["energy"], out["voiced"].view(torch.uint8), (energy, voiced))):
        got = phoneme_average(values, dur, plens, out["frames"], mask=mask)
        torch.cuda.synchronize()
        assert got["mean"].dtype == torch.float32 and got["count"].dtype == torch.int32 and tuple(got["mean"].shape) == (4, 70)
        m32, c32 = segment_mean_ref(vm[0], dur.cpu().numpy(), plens.tolist(), frames.tolist(), vm[1], dtype=np.float32)
        m64, c64 = segment_mean_ref(vm[0], dur.cpu().numpy(), plens.tolist(), frames.tolist(), vm[1], dtype=np.float64)
        assert np.array_equal(got["count"].cpu().numpy(), c32) and np.array_equal(c32, c64)
        assert np.array_equal(got["mean"].cpu().numpy(), m32)                 # bit-exact: the stock fp32 form sums in the same order
        assert np.abs(got["mean"].cpu().numpy() - m64).max() <= 1e-6 * np.abs(m64).max()
        assert (c32[3, 66:] == 0).all() and (c32[2, 3:] == 0).all() and (mask is not None or c32[2, :3].tolist() == [4, 4, 2])
        assert mask is None or (c32[0] == 0).all()                            # no voiced frame: the mean is 0, not a division by 0
    strided = torch.zeros(4, 2 * f0.shape[1], device=DEV)
    strided[:, :f0.shape[1]] = out["energy"]
    a = phoneme_average(strided[:, :f0.shape[1]], dur, plens.cpu(), out["frames"].to(torch.int32))
    b = phoneme_average(out["energy"], dur, plens, out["frames"])
    assert torch.equal(a["mean"], b["mean"]) and torch.equal(a["count"], b["count"])


def test_the_chain_from_teacher_durations_to_phoneme_pitch():
    from oracle import synth_batch
    from test_hip_model import _build
    from transformertts_amd import phoneme_average, teacher_durations
    cfg, m = _build("tiny", 11)
    batch = synth_batch(3, 12, 40, cfg["n_mels"], cfg["n_phon"], ragged=True, seed=21)
    args = [batch[k].to(DEV) for k in ("phoneme", "melspec", "phoneme_lens", "melspec_lens")]
    dur = teacher_durations(m, *args, method="mas")["durations"]
    gen = torch.Generator().manual_seed(3)
    voiced = torch.rand(3, 40, generator=gen) < 0.6
    f0 = torch.where(voiced, 100.0 + 200.0 * torch.rand(3, 40, generator=gen), torch.zeros(3, 40))
    got = phoneme_average(f0.to(DEV), dur, args[2], args[3], mask=voiced.to(DEV))
    torch.cuda.synchronize()
    want, count = segment_mean_ref(f0.numpy(), dur.cpu().numpy(), batch["phoneme_lens"].tolist(), batch["melspec_lens"].tolist(),
                                   voiced.numpy(), dtype=np.float32)
    assert np.array_equal(got["mean"].cpu().numpy(), want) and np.array_equal(got["count"].cpu().numpy(), count)
    valid = (batch["melspec_lens"] >= batch["phoneme_lens"]).numpy()
    assert valid.any()
    for b in np.flatnonzero(valid):                                           # the durations tile the frames: every voiced frame counts once
        assert int(count[b].sum()) == int(voiced[b, :int(batch["melspec_lens"][b])].sum())
