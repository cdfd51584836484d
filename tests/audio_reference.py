"""fp64 numpy reference of the log-mel front end (csrc/audio.hip): reflect padding, explicit framing, the periodic Hann window,
np.fft.rfft, a slaney mel basis written on its own (loops over filters and bins, not the package's broadcast form), log / clip /
normalise and the data-set statistics.  The definitions are librosa's documented ones (stft(center=True, pad_mode='reflect'),
filters.mel(htk=False, norm='slaney')).  Shared by tests/test_audio_host.py and tests/test_hip_audio.py."""
import math

import numpy as np

CONFIG_A = dict(sample_rate=22050, n_fft=1024, hop_length=256, win_length=1024, n_mels=80, fmin=0.0, fmax=8000.0)
CONFIG_B = dict(sample_rate=16000, n_fft=512, hop_length=128, win_length=400, n_mels=40, fmin=50.0, fmax=8000.0)
CLIP = 1e-5


def window_ref(win_length, n_fft):
    w = np.zeros(n_fft)
    left = (n_fft - win_length) // 2
    for n in range(win_length):
        w[left + n] = 0.5 - 0.5 * math.cos(2.0 * math.pi * n / win_length)
    return w


def frames_ref(x, n_fft, hop):
    """(T, n_fft) float64 frames of the reflect-padded signal, T = 1 + len // hop"""
    x = np.asarray(x, dtype=np.float64)
    assert x.size >= n_fft // 2 + 1, "too short to reflect"
    padded = np.pad(x, n_fft // 2, mode="reflect")
    T = 1 + x.size // hop
    return np.stack([padded[t * hop:t * hop + n_fft] for t in range(T)])


def stft_ref(x, n_fft, hop, win_length):
    """(T, n_fft/2+1) complex128"""
    return np.fft.rfft(frames_ref(x, n_fft, hop) * window_ref(win_length, n_fft)[None, :], axis=1)


def _hz_to_mel(f):
    return f / (200.0 / 3.0) if f < 1000.0 else 15.0 + math.log(f / 1000.0) / (math.log(6.4) / 27.0)


def _mel_to_hz(m):
    return (200.0 / 3.0) * m if m < 15.0 else 1000.0 * math.exp((math.log(6.4) / 27.0) * (m - 15.0))


def mel_filterbank_ref(sample_rate, n_fft, n_mels, fmin, fmax):
    bins = n_fft // 2 + 1
    lo, hi = _hz_to_mel(fmin), _hz_to_mel(fmax)
    edge = [_mel_to_hz(lo + (hi - lo) * i / (n_mels + 1)) for i in range(n_mels + 2)]
    fb = np.zeros((n_mels, bins))
    for i in range(n_mels):
        for k in range(bins):
            f = (sample_rate / 2.0) * k / (bins - 1)
            up = (f - edge[i]) / (edge[i + 1] - edge[i])
            down = (edge[i + 2] - f) / (edge[i + 2] - edge[i + 1])
            fb[i, k] = max(0.0, min(up, down)) * 2.0 / (edge[i + 2] - edge[i])
    return fb


def magnitude_ref(x, cfg):
    return np.abs(stft_ref(x, cfg["n_fft"], cfg["hop_length"], cfg["win_length"]))


def logmel_ref(x, cfg, fb=None, clip=CLIP, mean=None, std=None):
    """(T, n_mels) float64"""
    fb = mel_filterbank_ref(cfg["sample_rate"], cfg["n_fft"], cfg["n_mels"], cfg["fmin"], cfg["fmax"]) if fb is None else fb
    mel = np.log(np.maximum(magnitude_ref(x, cfg) @ fb.T, clip))
    return mel if mean is None else (mel - mean) / (std + 1e-8)


def stats_ref(mels):
    """(sum, sum of squares, count) over a list of unnormalised log-mels, and preprocess.py:59-61's mean and std"""
    s = sum(float(m.sum()) for m in mels)
    q = sum(float((m ** 2).sum()) for m in mels)
    n = sum(m.size for m in mels)
    mean = s / n
    return s, q, n, mean, math.sqrt(q / n - mean ** 2 + 1e-8)


def make_signal(n, sample_rate, seed, zero=None):
    """0.3 sin(2 pi 220 t) + 0.05 sin(2 pi 3000 t) + 0.01 N(0, 1) in fp32; samples zero[0] .. zero[1] - 1 set to exact zero"""
    t = np.arange(n) / float(sample_rate)
    rng = np.random.default_rng(seed)
    x = 0.3 * np.sin(2 * np.pi * 220.0 * t) + 0.05 * np.sin(2 * np.pi * 3000.0 * t) + 0.01 * rng.standard_normal(n)
    x = x.astype(np.float32)
    if zero is not None:
        x[zero[0]:zero[1]] = 0.0
    return x


def ragged_batch(cfg, seed=0, pad=37):
    """the tests' batch: wave_lens = [n_fft/2+1, 5 hop, 8 hop - 1, 4000], padded to 4000 + pad with NaN beyond each length;
    samples 1500 .. 2999 of the longest utterance are exact zeros -> (wave (4, Nmax) fp32, lens list, signals list)"""
    n_fft, hop = cfg["n_fft"], cfg["hop_length"]
    lens = [n_fft // 2 + 1, 5 * hop, 8 * hop - 1, 4000]
    wave = np.full((len(lens), 4000 + pad), np.nan, dtype=np.float32)
    sigs = []
    for b, n in enumerate(lens):
        x = make_signal(n, cfg["sample_rate"], seed * 100 + b, zero=(1500, 3000) if n == 4000 else None)
        wave[b, :n] = x
        sigs.append(x)
    return wave, lens, sigs
