"""fp64 numpy reference of the Griffin-Lim vocoder (csrc/vocoder.hip), written from the definitions in include/ttts_hip.h on top of
tests/audio_reference.py: mel -> magnitude through the pseudo-inverse mel basis, the least-squares inverse STFT, the fast
Griffin-Lim iteration and the spectral convergence that judges a result.  Shared by tests/test_vocoder_host.py and
tests/test_hip_vocoder.py."""
import numpy as np

from audio_reference import mel_filterbank_ref, stft_ref, window_ref

TINY = 1.17549435e-38                    # the smallest normal fp32: an envelope at or below it is not divided by
FLOOR = 1e-10


def pinv_ref(cfg):
    """(bins, n_mels) float64 holding fp32 values: pinv of the oracle's own mel basis, formed in fp64 and rounded to fp32 once"""
    fb = mel_filterbank_ref(cfg["sample_rate"], cfg["n_fft"], cfg["n_mels"], cfg["fmin"], cfg["fmax"])
    return np.linalg.pinv(fb).astype(np.float32).astype(np.float64)


def vocodable(frames, cfg):
    return (frames - 1) * cfg["hop_length"] > cfg["n_fft"] // 2


def mel_to_magnitude_ref(mel, pinv, floor=FLOOR, mean=None, std=None):
    """(T, n_mels) (normalised) log-mel -> (T, bins) float64: max(pinv @ exp(x), floor)"""
    x = np.asarray(mel, dtype=np.float64)
    if mean is not None:
        x = x * (std + 1e-8) + mean
    return np.maximum(np.exp(x) @ np.asarray(pinv, dtype=np.float64).T, floor)


def istft_ref(spec, n_fft, hop, win_length):
    """(T, bins) complex -> the (T - 1) hop samples float64: irfft of every frame (the imaginary parts of bins 0 and n_fft/2 do not
    count), windowed overlap-add divided by the overlap-added squared window where that is a normal fp32 number, the n_fft/2
    samples of centring removed"""
    spec = np.array(spec, dtype=np.complex128)
    T = spec.shape[0]
    assert spec.shape[1] == n_fft // 2 + 1 and T >= 1
    spec[:, 0] = spec[:, 0].real
    spec[:, -1] = spec[:, -1].real
    w = window_ref(win_length, n_fft)
    x = np.fft.irfft(spec, n=n_fft, axis=1)
    y = np.zeros(n_fft + (T - 1) * hop)
    env = np.zeros_like(y)
    for t in range(T):
        y[t * hop:t * hop + n_fft] += w * x[t]
        env[t * hop:t * hop + n_fft] += w * w
    ok = env > TINY
    out = np.where(ok, y / np.where(ok, env, 1.0), y)
    return out[n_fft // 2:n_fft // 2 + (T - 1) * hop]


def envelope_zero_count(T, n_fft, hop, win_length):
    """how many of the (T - 1) hop samples no window reaches"""
    w = window_ref(win_length, n_fft)
    env = np.zeros(n_fft + (T - 1) * hop)
    for t in range(T):
        env[t * hop:t * hop + n_fft] += w * w
    return int((env[n_fft // 2:n_fft // 2 + (T - 1) * hop] <= TINY).sum())


def spectral_convergence(wave, mag, n_fft, hop, win_length):
    """|| |STFT(wave)| - mag ||_F / || mag ||_F, the STFT the fp64 oracle's"""
    got = np.abs(stft_ref(np.asarray(wave, dtype=np.float64), n_fft, hop, win_length))
    mag = np.asarray(mag, dtype=np.float64)
    assert got.shape == mag.shape, (got.shape, mag.shape)
    return float(np.linalg.norm(got - mag) / np.linalg.norm(mag))


def griffin_lim_ref(mag, init, n_fft, hop, win_length, n_iter, momentum, trace=None):
    """(T, bins) magnitudes and unit phases -> (T - 1) hop samples; `trace`, a list, receives the spectral convergence of the wave
    of every inverse transform (n_iter + 1 values)"""
    mag = np.asarray(mag, dtype=np.float64)
    spec = mag * np.asarray(init, dtype=np.complex128)
    prev = np.zeros_like(spec)
    c = momentum / (1.0 + momentum)
    for _ in range(n_iter):
        wave = istft_ref(spec, n_fft, hop, win_length)
        if trace is not None:
            trace.append(spectral_convergence(wave, mag, n_fft, hop, win_length))
        reb = stft_ref(wave, n_fft, hop, win_length)
        t = reb - c * prev
        prev = reb
        a2 = t.real ** 2 + t.imag ** 2
        big = a2 > 1e-30
        spec = mag * np.where(big, t / np.sqrt(np.where(big, a2, 1.0)), 1.0)
    wave = istft_ref(spec, n_fft, hop, win_length)
    if trace is not None:
        trace.append(spectral_convergence(wave, mag, n_fft, hop, win_length))
    return wave


def unit_phases(shape, seed):
    """complex64 unit phases exp(2 pi i U) from numpy's generator"""
    u = np.random.default_rng(seed).random(shape)
    return np.exp(2j * np.pi * u).astype(np.complex64)
