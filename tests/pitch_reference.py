"""Reference of the frame pitch and energy kernels (csrc/pitch.hip), straight from the definition in include/ttts_hip.h:
`pitch_ref` in fp64 numpy with the decision margin of every frame, `pitch_stock` the same algorithm in stock fp32 torch on the
CPU in the kernel's summation order (blocks of BL samples in ascending j, block partials in ascending block order, a running
sum in ascending lag), `energy_ref` from the rfft (not from the identity the kernel uses) and `segment_mean_ref`.  Shared by
tests/test_pitch_host.py and tests/test_hip_pitch.py."""
import math

import numpy as np

from audio_reference import window_ref

# (sample_rate, hop, n_fft, frame_length, window, fmin, fmax)
SMALL = dict(sample_rate=8000, hop_length=64, n_fft=256, win_length=256, frame_length=256, window=128, fmin=80.0, fmax=500.0)
SHIPPED = dict(sample_rate=22050, hop_length=256, n_fft=1024, win_length=1024, frame_length=1024, window=512, fmin=65.0, fmax=600.0)
ODD_WINDOW = dict(sample_rate=8000, hop_length=48, n_fft=256, win_length=200, frame_length=256, window=100, fmin=80.0, fmax=500.0)
SHORT_FRAME = dict(sample_rate=8000, hop_length=64, n_fft=512, win_length=400, frame_length=256, window=128, fmin=80.0, fmax=500.0)
# 2000 lags: a workgroup's LDS holds two frames and no shared partials (block = window), two waves work in its second phase; the
# signal glides from 88 to 96 Hz without bursts (a window is a quarter of a second) while the lags go down to 4 Hz
LONG_LAGS = dict(sample_rate=8000, hop_length=512, n_fft=2048, win_length=2048, frame_length=4096, window=2048, fmin=4.0, fmax=500.0,
                 block=2048, glide_fmin=80.0, glide_top=1.2, bursts=False)
THRESHOLD = 0.1


def lags_ref(p):
    return int(math.floor(p["sample_rate"] / p["fmax"])), int(math.ceil(p["sample_rate"] / p["fmin"]))


def block_ref(p):
    """the block length of the kernel's sum (ttts_pitch_block): hop when it divides the window into at most 8 blocks, else the
    window; a shape whose shared partials do not fit the workgroup's LDS names its block"""
    W, hop = p["window"], p["hop_length"]
    if "block" in p:
        return p["block"]
    return hop if W % hop == 0 and W // hop <= 8 else W


def frame_count_ref(n, p):
    return 1 + n // p["hop_length"] if n > max(p["frame_length"], p["n_fft"]) // 2 else 0


def pitch_frames_ref(x, p, dtype=np.float64):
    """(T, F) frames x_n = x[t hop - F/2 + n], reflected without repeating the edge"""
    x = np.asarray(x, dtype=dtype)
    T, F, hop = frame_count_ref(x.size, p), p["frame_length"], p["hop_length"]
    if T == 0:
        return np.zeros((0, F), dtype=dtype)
    padded = np.pad(x, F // 2, mode="reflect")
    return np.stack([padded[t * hop:t * hop + F] for t in range(T)])


def decide(dp, tau_min, tau_max, threshold, sample_rate):
    """d' (T, tau_max), column tau - 1 holding lag tau, in any float type -> voiced, tau*, f0, aperiodicity, margin (the arithmetic
    of f0 in dp's type)"""
    T = dp.shape[0]
    ft = dp.dtype.type
    voiced = np.zeros(T, dtype=bool)
    lag = np.zeros(T, dtype=np.int64)
    f0 = np.zeros(T, dtype=dp.dtype)
    aper = np.zeros(T, dtype=dp.dtype)
    margin = np.zeros(T, dtype=np.float64)
    for t in range(T):
        d = dp[t]
        val = lambda tau: d[tau - 1]
        tau0 = next((tau for tau in range(tau_min, tau_max + 1) if val(tau) < threshold), None)
        if tau0 is None:
            rng = d[tau_min - 1:tau_max]
            lag[t] = tau_min + int(np.argmin(rng))                    # (numpy's argmin is the first one)
            aper[t] = val(lag[t])
            margin[t] = float(rng.min()) - threshold
            continue
        gaps = [threshold - float(val(tau0))] + [float(val(tau)) - threshold for tau in range(tau_min, tau0)]
        tau = tau0
        while tau + 1 <= tau_max and val(tau + 1) < val(tau):
            gaps.append(float(val(tau)) - float(val(tau + 1)))
            tau += 1
        if tau + 1 <= tau_max:
            gaps.append(float(val(tau + 1)) - float(val(tau)))        # the step that stopped the walk
        s = ft(0)
        if tau_min < tau < tau_max:
            a, b, c = val(tau - 1), val(tau), val(tau + 1)
            den = a - ft(2) * b + c
            if den > 0:
                s = min(max(ft(0.5) * (a - c) / den, ft(-0.5)), ft(0.5))
        voiced[t], lag[t], aper[t], margin[t] = True, tau, val(tau), min(gaps)
        f0[t] = ft(sample_rate) / (ft(tau) + s)
    return voiced, lag, f0, aper, margin


def pitch_ref(x, p, threshold=THRESHOLD):
    """fp64 -> dict(voiced, lag, f0, aperiodicity, margin (T,), dprime (T, tau_max), frames)"""
    tau_min, tau_max = lags_ref(p)
    W = p["window"]
    fr = pitch_frames_ref(x, p)
    T = fr.shape[0]
    d = np.zeros((T, tau_max))
    for tau in range(1, tau_max + 1):
        d[:, tau - 1] = ((fr[:, :W] - fr[:, tau:tau + W]) ** 2).sum(axis=1)
    cs = np.cumsum(d, axis=1)
    taus = np.arange(1, tau_max + 1, dtype=np.float64)[None, :]
    dp = np.where(cs == 0.0, 1.0, d * taus / np.where(cs == 0.0, 1.0, cs))
    voiced, lag, f0, aper, margin = decide(dp, tau_min, tau_max, threshold, p["sample_rate"])
    return dict(voiced=voiced, lag=lag, f0=f0, aperiodicity=aper, margin=margin, dprime=dp, frames=T)


def pitch_stock(x, p, threshold=THRESHOLD):
    """the same algorithm in stock fp32 torch on the CPU, in the kernel's summation order; the same dict as `pitch_ref`, with
    `energy` from torch.fft.rfft in fp32"""
    import torch
    tau_min, tau_max = lags_ref(p)
    W, BL = p["window"], block_ref(p)
    fr = torch.from_numpy(pitch_frames_ref(np.asarray(x, dtype=np.float32), p, dtype=np.float32))
    T = fr.shape[0]
    idx = torch.arange(1, tau_max + 1)
    d = torch.zeros(T, tau_max, dtype=torch.float32)
    for blk in range(W // BL):
        acc = torch.zeros(T, tau_max, dtype=torch.float32)
        for j in range(blk * BL, (blk + 1) * BL):
            diff = fr[:, j:j + 1] - fr[:, idx + j]
            acc = acc + diff * diff
        d = acc if blk == 0 else d + acc
    cs = torch.cumsum(d, dim=1)
    dp = torch.where(cs == 0, torch.ones_like(d), d * idx.to(torch.float32)[None, :] / torch.where(cs == 0, torch.ones_like(cs), cs))
    voiced, lag, f0, aper, margin = decide(dp.numpy(), tau_min, tau_max, np.float32(threshold), p["sample_rate"])
    out = dict(voiced=voiced, lag=lag, f0=f0, aperiodicity=aper, margin=margin, dprime=dp.numpy(), frames=T)
    if T:
        n_fft = p["n_fft"]
        padded = np.pad(np.asarray(x, dtype=np.float32), n_fft // 2, mode="reflect")
        ef = torch.from_numpy(np.stack([padded[t * p["hop_length"]:t * p["hop_length"] + n_fft] for t in range(T)]))
        win = torch.from_numpy(window_ref(p["win_length"], n_fft).astype(np.float32))
        spec = torch.fft.rfft(ef * win[None, :], dim=1)
        out["energy"] = torch.sqrt((spec.real ** 2 + spec.imag ** 2).sum(dim=1)).numpy()
    else:
        out["energy"] = np.zeros(0, dtype=np.float32)
    return out


def energy_frames_ref(x, p):
    """(T, n_fft) fp64 windowed frames centred at t hop, T by the pitch rule"""
    x = np.asarray(x, dtype=np.float64)
    T, n_fft, hop = frame_count_ref(x.size, p), p["n_fft"], p["hop_length"]
    if T == 0:
        return np.zeros((0, n_fft))
    padded = np.pad(x, n_fft // 2, mode="reflect")
    return np.stack([padded[t * hop:t * hop + n_fft] for t in range(T)]) * window_ref(p["win_length"], n_fft)[None, :]


def energy_ref(x, p):
    """(T,) fp64: the L2 norm over the n_fft/2 + 1 bins of the rfft of the windowed frame"""
    return np.sqrt((np.abs(np.fft.rfft(energy_frames_ref(x, p), axis=1)) ** 2).sum(axis=1))


def energy_identity(y):
    """the kernel's identity on windowed frames (T, n_fft): (n sum y^2 + (sum y)^2 + (sum (-1)^n y)^2) / 2, square-rooted"""
    n = y.shape[1]
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    return np.sqrt(0.5 * (n * (y ** 2).sum(axis=1) + y.sum(axis=1) ** 2 + (y * sign[None, :]).sum(axis=1) ** 2))


def segment_mean_ref(values, durations, phoneme_lens, frames, mask=None, dtype=np.float64):
    """-> (mean (B, Pmax) in `dtype`, summed in ascending frame order, count (B, Pmax) int32)"""
    values = np.asarray(values)
    B, Tmax = values.shape
    Pmax = durations.shape[1]
    mean = np.zeros((B, Pmax), dtype=dtype)
    count = np.zeros((B, Pmax), dtype=np.int32)
    for b in range(B):
        fr = min(max(int(frames[b]), 0), Tmax)
        at = 0
        for q in range(min(max(int(phoneme_lens[b]), 0), Pmax)):
            dur = max(int(durations[b, q]), 0)
            acc, n = dtype(0), 0
            for t in range(min(at, fr), min(at + dur, fr)):
                if mask is None or mask[b, t]:
                    acc = dtype(acc + dtype(values[b, t]))
                    n += 1
            at += dur
            mean[b, q] = acc / dtype(n) if n else dtype(0)
            count[b, q] = n
    return mean, count


def glide_signal(n, p, seed):
    """a four-harmonic glide from 1.1 to 2.4 fmin, gated by noise bursts of 0.05 (40 ms of every 190 ms), plus 0.002 of white noise;
    fp32.  A shape may name the glide's base (`glide_fmin`), its top in units of it (`glide_top`) and switch the bursts off."""
    sr, fmin = float(p["sample_rate"]), p.get("glide_fmin", p["fmin"])
    rng = np.random.default_rng(seed)
    f = np.linspace(1.1 * fmin, p.get("glide_top", 2.4) * fmin, max(n, 1))
    phase = 2.0 * np.pi * np.cumsum(f) / sr
    tone = sum(a * np.sin(h * phase + 0.7 * h) for h, a in ((1, 0.30), (2, 0.15), (3, 0.10), (4, 0.06)))
    t = np.arange(n) / sr
    burst = ((t % 0.19) >= 0.15) & p.get("bursts", True)
    x = np.where(burst, 0.05 * rng.standard_normal(n), tone[:n]) + 0.002 * rng.standard_normal(n)
    return x.astype(np.float32)


def cents(f, ref):
    return 1200.0 * np.abs(np.log2(np.asarray(f, dtype=np.float64) / np.asarray(ref, dtype=np.float64)))
