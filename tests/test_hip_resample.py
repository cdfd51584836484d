"""Band-limited resampler on the GPU (csrc/resample.hip, transformertts_amd.audio.Resampler) against the fp64 oracle of
tests/resample_reference.py: lengths, reads inside the lengths (NaN behind them), zeros behind the outputs, accuracy (rel-L2 <=
1e-4, and the largest error within 4 x that of the same algorithm in stock fp32 torch on the CPU: both are fp32 sums of K products
and differ only in summation order), output positions whose j M leaves 32 bits, the extremes of the lengths, bit-for-bit
repeatability (two calls, a strided view, another batch and width, a captured call), round trips, and the front end fed
straight from the resampler."""
import functools

import numpy as np
import pytest
import torch

from audio_reference import CONFIG_A, logmel_ref, mel_filterbank_ref
from resample_reference import (PAIRS_SMALL, ZEROS, band_limited, make_wave, out_len_ref, ratio_ref, resample_ref, stock_resample,
                                stock_weights)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (orig, new, zeros): the four small ratios, a down-sampling with L < the workgroup, an up-sampling whose L = 441 exceeds it,
# a short kernel (K = 50) and L = 1
PAIRS = tuple((o, n, 6) for o, n in PAIRS_SMALL) + ((48000, 22050, ZEROS), (16000, 22050, ZEROS), (22050, 16000, 16), (44100, 22050, ZEROS))
PAD = 37


@functools.lru_cache(maxsize=None)
def _resampler(orig, new, zeros=ZEROS):
    from transformertts_amd.audio import Resampler
    return Resampler(orig, new, device=DEV, zeros=zeros)


def _tile():
    from transformertts_amd import _lib
    return _lib.load().ttts_resample_tile()


def _stock(x, rs):
    """the stock fp32 restatement on the CPU of one utterance at its own length, with the kernel's own table"""
    table = torch.from_numpy(rs.table_host)
    return stock_resample(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))[None], stock_weights(table, rs.L, rs.M, rs.K),
                          rs.L, rs.M, rs.K)[0]


@functools.lru_cache(maxsize=None)
def _case(orig, new, zeros, seed=0):
    """the ragged batch of a pair: lengths 1, W, the longest length whose output stays within two tiles (exactly 2 tile when the
    ratio can reach it: every down-sampling does) and the shortest whose output passes them (2 tile + 1 likewise); NaN behind every
    length in a buffer PAD wider than the longest row; the oracle (computed once, never modified) and the stock form's error"""
    rs = _resampler(orig, new, zeros)
    L, M, _, W, K = ratio_ref(orig, new, zeros)
    tile = _tile()
    at = (2 * tile * M) // L
    assert out_len_ref(at, L, M) <= 2 * tile < out_len_ref(at + 1, L, M)
    if L < M:
        assert out_len_ref(at, L, M) == 2 * tile and out_len_ref(at + 1, L, M) == 2 * tile + 1
    lens = [1, W, at, at + 1]
    wave = np.full((4, at + 1 + PAD), np.nan, dtype=np.float32)
    sigs = []
    for b, n in enumerate(lens):
        x = make_wave(n, 22050, 1000 * seed + 10 * b + 1)              # (content up to 0.27 of the input's Nyquist, plus noise)
        wave[b, :n] = x
        sigs.append(x)
    want = [resample_ref(x, orig, new, zeros) for x in sigs]
    stock_err = max(float(np.abs(_stock(x, rs).double().numpy() - w).max()) for x, w in zip(sigs, want))
    for w in want:
        w.setflags(write=False)
    return dict(rs=rs, wave=wave, lens=lens, sigs=sigs, want=want, stock_err=stock_err, out_lens=[w.size for w in want], L=L, M=M, W=W)


def _device_batch(case):
    return torch.from_numpy(case["wave"]).to(DEV), torch.tensor(case["lens"], device=DEV)


@pytest.mark.parametrize("orig,new,zeros", PAIRS)
def test_parity_with_the_fp64_oracle(orig, new, zeros):
    case = _case(orig, new, zeros)
    rs = case["rs"]
    wave, lens = _device_batch(case)
    out = rs(wave, lens)
    y, out_lens = out["wave"], out["wave_lens"]
    Nout = out_len_ref(wave.size(1), case["L"], case["M"])
    assert tuple(y.shape) == (4, Nout) and y.dtype == torch.float32 and out_lens.dtype == torch.int64 and y.is_contiguous()
    assert out_lens.tolist() == case["out_lens"] == [out_len_ref(n, case["L"], case["M"]) for n in case["lens"]]
    assert Nout > max(case["out_lens"])
    assert not bool(torch.isnan(y).any()), "a sample behind a length was read"
    got = y.double().cpu().numpy()
    for b, n in enumerate(case["out_lens"]):
        assert (got[b, n:] == 0).all(), "samples from out_len to Nout must be exactly zero"
    g = np.concatenate([got[b, :n] for b, n in enumerate(case["out_lens"])])
    w = np.concatenate(case["want"])
    rel, err = float(np.linalg.norm(g - w) / np.linalg.norm(w)), float(np.abs(g - w).max())
    print(f"resample {orig} -> {new} (L {case['L']}, M {case['M']}, K {rs.K}): rel-L2 {rel:.3e} max-abs {err:.3e}; "
          f"stock fp32 torch (CPU) max-abs {case['stock_err']:.3e}")
    assert rel <= 1e-4
    assert err <= 4 * case["stock_err"]


def test_positions_past_2_to_the_31():
    """j M leaves 32 bits from output 4.87 M on at M = 441: the last 1400 outputs of a 6.8 M sample utterance (27 MB) against the
    oracle.  Output j_a + e of x, j_a a multiple of L, is output L + e of x[i_a - M:] with i_a = j_a M / L (the M samples in
    front hold every tap that reaches back: W = 24), so the oracle only sees the tail."""
    orig, new, zeros = 22050, 16000, 16
    rs = _resampler(orig, new, zeros)
    L, M = rs.L, rs.M
    n = 6_800_000
    x = make_wave(n, orig, 5)
    out = rs(torch.from_numpy(x)[None].to(DEV), torch.tensor([n], device=DEV))
    m = out_len_ref(n, L, M)
    assert out["wave_lens"].tolist() == [m] and tuple(out["wave"].shape) == (1, m)
    j_a = (m - 1400) // L * L
    i_a = j_a * M // L
    assert j_a * M >= 2 ** 31 and M >= rs.K // 2 - 1
    tail = x[i_a - M:]
    want = resample_ref(tail, orig, new, zeros)[L:]
    stock_err = float(np.abs(_stock(tail, rs).double().numpy()[L:] - want).max())
    got = out["wave"][0, j_a:].double().cpu().numpy()
    assert got.shape == want.shape == (m - j_a,)
    rel, err = float(np.linalg.norm(got - want) / np.linalg.norm(want)), float(np.abs(got - want).max())
    print(f"resample {orig} -> {new}, outputs {j_a} .. {m - 1} (j M up to {(m - 1) * M}): rel-L2 {rel:.3e} max-abs {err:.3e}; "
          f"stock fp32 torch (CPU) max-abs {stock_err:.3e}")
    assert rel <= 1e-4
    assert err <= 4 * stock_err


def test_the_extremes_of_the_lengths():
    case = _case(48000, 22050, ZEROS)
    rs = case["rs"]
    wave, _ = _device_batch(case)
    Nmax = wave.size(1)
    full = wave.clone()
    full[1] = torch.from_numpy(make_wave(Nmax, 22050, 77)).to(DEV)     # the row whose length is above Nmax: finite to the end
    lens = torch.tensor([0, Nmax + 1000, -5, case["lens"][3]], device=DEV)
    out = rs(full, lens)
    Nout = out_len_ref(Nmax, rs.L, rs.M)
    assert out["wave_lens"].tolist() == [0, Nout, 0, case["out_lens"][3]]
    assert not bool(torch.isnan(out["wave"]).any())                    # row 2 is NaN from its first sample, row 0 from its second
    assert bool((out["wave"][[0, 2]] == 0).all())
    same = rs(full, torch.tensor([0, Nmax, 0, case["lens"][3]], device=DEV))
    assert torch.equal(same["wave"], out["wave"]) and torch.equal(same["wave_lens"], out["wave_lens"])
    assert torch.equal(out["wave"][3], rs(wave, torch.tensor(case["lens"], device=DEV))["wave"][3])
    assert rs(full, lens.cpu())["wave_lens"].tolist() == out["wave_lens"].tolist()       # host lengths are accepted
    with pytest.raises(ValueError, match="wave must be \\(B, Nmax\\)"):
        rs(wave[0], lens)
    with pytest.raises(ValueError, match="wave_lens must have shape"):
        rs(wave, lens[:3])
    with pytest.raises(ValueError, match="expected a CUDA/HIP tensor"):
        rs(wave.cpu(), lens)
    with pytest.raises(ValueError, match="expected dtype torch.float32"):
        rs(wave.double(), lens)
    with pytest.raises(ValueError, match="wave_lens must be integers"):
        rs(wave, lens.float())


@pytest.mark.parametrize("orig,new,zeros", [(48000, 22050, ZEROS), (16000, 22050, ZEROS), (2, 1, 6)])
def test_the_same_bits_whatever_the_call_the_strides_the_batch_and_the_grid(orig, new, zeros):
    case = _case(orig, new, zeros)
    rs = case["rs"]
    wave, lens = _device_batch(case)
    first, again = rs(wave, lens), rs(wave, lens)
    assert torch.equal(first["wave"], again["wave"]) and torch.equal(first["wave_lens"], again["wave_lens"])
    big = torch.full((4, wave.size(1) + 8), float("nan"), device=DEV)
    big[:, 3:3 + wave.size(1)] = wave
    view = big[:, 3:3 + wave.size(1)]
    assert view.stride(0) != wave.size(1) and not view.is_contiguous()
    assert torch.equal(rs(view, lens)["wave"], first["wave"])
    # a row alone, in a buffer of another width (another Nout and grid), against the same row in the batch
    for b in (2, 3):
        n = case["lens"][b]
        alone = torch.full((1, n + 300), float("nan"), device=DEV)
        alone[0, :n] = wave[b, :n]
        one = rs(alone, torch.tensor([n], device=DEV))
        m = case["out_lens"][b]
        assert one["wave_lens"].tolist() == [m] and one["wave"].size(1) != first["wave"].size(1)
        assert torch.equal(one["wave"][0, :m], first["wave"][b, :m])
    # captured, then replayed on a second waveform copied into the same buffers
    other = _case(orig, new, zeros, 1)
    wave2 = torch.from_numpy(np.ascontiguousarray(other["wave"][::-1])).to(DEV)          # the utterances in reverse order
    lens2 = torch.tensor(other["lens"][::-1], device=DEV)
    eager2 = rs(wave2, lens2)
    sw, sl = wave.clone(), lens.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = rs(sw, sl)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out["wave"], first["wave"]) and torch.equal(out["wave_lens"], first["wave_lens"])
    sw.copy_(wave2)
    sl.copy_(lens2)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out["wave"], eager2["wave"]) and torch.equal(out["wave_lens"], eager2["wave_lens"])
    assert out["wave_lens"].tolist() == case["out_lens"][::-1]


@functools.lru_cache(maxsize=None)
def _round_trip_case(a, b):
    """a -> b -> a of a sum of sines below 0.8 of the lower Nyquist: the fp64 oracle's round trip and the stock fp32 form's error
    against it over the middle half"""
    n = 4000
    x = band_limited(n, a, 0.8 * min(a, b) / 2.0, seed=a + b)
    there = resample_ref(x, a, b)
    back = resample_ref(there, b, a)
    mid = slice(n // 4, n - n // 4)
    st = _stock(_stock(x, _resampler(a, b)).numpy(), _resampler(b, a)).double().numpy()
    return dict(x=x, back=back, mid=mid, stock_err=float(np.abs(st - back)[mid].max()),
                oracle_err=float(np.abs(back[:n] - x.astype(np.float64))[mid].max()))


@pytest.mark.parametrize("a,b", [(22050, 16000), (16000, 22050)])
def test_round_trip(a, b):
    """On the CPU the oracle's own round trip returns the signal within 2.2e-8 over the middle half (measured: 22050 -> 16000 ->
    22050 2.1e-8, 16000 -> 22050 -> 16000 1.7e-8), so the 1e-5 bound against the signal itself is asserted as it stands."""
    case = _round_trip_case(a, b)
    n = case["x"].size
    wave = torch.full((1, n + PAD), float("nan"), device=DEV)
    wave[0, :n] = torch.from_numpy(case["x"]).to(DEV)
    there = _resampler(a, b)(wave, torch.tensor([n], device=DEV))
    back = _resampler(b, a)(**there)
    m = int(back["wave_lens"][0])
    assert m == case["back"].size >= n and not bool(torch.isnan(back["wave"]).any())
    got = back["wave"][0, :m].double().cpu().numpy()
    err = float(np.abs(got - case["back"])[case["mid"]].max())
    err_signal = float(np.abs(got[:n] - case["x"].astype(np.float64))[case["mid"]].max())
    print(f"resample round trip {a} -> {b} -> {a}: max-abs against the oracle's round trip {err:.3e} (stock fp32 torch (CPU) "
          f"{case['stock_err']:.3e}), against the signal {err_signal:.3e} (the oracle's round trip {case['oracle_err']:.3e})")
    assert err <= 4 * case["stock_err"]
    assert case["oracle_err"] <= 1e-5
    assert err_signal <= 1e-5


def test_the_resampler_feeds_the_front_end():
    """MelFrontEnd(cfg)(**Resampler(16000, 22050)(wave, lens)) against logmel_ref(resample_ref(.)), within the front end's own
    bound: rel-L2 <= 1e-4 and the largest error within 4 x that of the stock fp32 chain on the CPU (the stock resampler above,
    then torch.stft, an fp32 filter-bank matmul and log)"""
    from transformertts_amd.audio import MelFrontEnd
    cfg = CONFIG_A
    rs = _resampler(16000, 22050)
    lens = [700, 2400, 1999]
    sigs = [make_wave(n, 16000, 50 + b) for b, n in enumerate(lens)]
    wave = np.full((3, max(lens) + PAD), np.nan, dtype=np.float32)
    for b, x in enumerate(sigs):
        wave[b, :x.size] = x
    fb = mel_filterbank_ref(cfg["sample_rate"], cfg["n_fft"], cfg["n_mels"], cfg["fmin"], cfg["fmax"])
    want = [logmel_ref(resample_ref(x, 16000, 22050), cfg, fb) for x in sigs]
    win = torch.hann_window(cfg["win_length"], periodic=True, dtype=torch.float32)
    fb32 = torch.from_numpy(fb).float()
    stock_err = 0.0
    for x, w in zip(sigs, want):
        spec = torch.stft(_stock(x, rs), cfg["n_fft"], hop_length=cfg["hop_length"], win_length=cfg["win_length"], window=win,
                          center=True, pad_mode="reflect", return_complex=True).abs().T
        stock_err = max(stock_err, float(np.abs(torch.log(torch.clamp(spec @ fb32.T, min=1e-5)).double().numpy() - w).max()))
    out = MelFrontEnd(cfg, device=DEV)(**rs(torch.from_numpy(wave).to(DEV), torch.tensor(lens, device=DEV)))
    frames = [w.shape[0] for w in want]
    assert out["melspec_lens"].tolist() == frames == [1 + out_len_ref(n, rs.L, rs.M) // cfg["hop_length"] for n in lens]
    mel = out["melspec"].double().cpu().numpy()
    assert not np.isnan(mel).any()
    g = np.concatenate([mel[b, :t].reshape(-1) for b, t in enumerate(frames)])
    w = np.concatenate([r.reshape(-1) for r in want])
    rel, err = float(np.linalg.norm(g - w) / np.linalg.norm(w)), float(np.abs(g - w).max())
    print(f"resampler -> front end: log-mel rel-L2 {rel:.3e} max-abs {err:.3e}; stock fp32 chain (CPU) max-abs {stock_err:.3e}")
    assert rel <= 1e-4
    assert err <= 4 * stock_err


def test_equal_rates_return_the_input_without_a_launch():
    from transformertts_amd.audio import Resampler
    rs = Resampler(22050, 22050, device=DEV)
    assert rs.table is None and (rs.L, rs.M) == (1, 1)
    wave = torch.full((3, 50), float("nan"), device=DEV)
    out = rs(wave, torch.tensor([-3, 20, 99], device=DEV))
    assert out["wave"] is wave and out["wave_lens"].tolist() == [0, 20, 50] and out["wave_lens"].dtype == torch.int64
    host = rs(wave.cpu(), torch.tensor([1, 2, 3]))                     # ... so the identity runs on host tensors too
    assert host["wave"].device.type == "cpu" and host["wave_lens"].tolist() == [1, 2, 3]
