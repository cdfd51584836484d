"""fp64 numpy reference of the band-limited resampler (csrc/resample.hip), written from the definition, with no table:

    g = gcd(orig, new), L = new / g, M = orig / g, s = rolloff * min(1, L / M), W = ceil(zeros / s), K = 2 W + 2
    kernel(u) = sinc(u) * I0(beta sqrt(1 - (u / zeros)^2)) / I0(beta) for |u| < zeros, else 0
    y[j] = sum_{k < K} s * kernel(s * (j M / L - i)) * x[i],  i = floor(j M / L) - W + k,  x = 0 outside [0, len)
    len(y) = ceil(len(x) L / M)

and the same algorithm in stock fp32 torch (pad, conv1d with one output channel per phase at stride M, transpose, reshape, trim):
what the GPU tests bound the kernel's error with and tools/resample_bench.py times it against.  I0 is numpy's here (the package
sums the power series; tests/test_resample_host.py holds both against scipy.special.i0).  Shared by tests/test_resample_host.py,
tests/test_hip_resample.py and tools/resample_bench.py."""
import math

import numpy as np

ZEROS, ROLLOFF, BETA = 64, 0.9475937167399596, 14.769656459379492
PAIRS_SMALL = ((2, 1), (1, 2), (7, 5), (5, 7))          # at zeros = 6


def ratio_ref(orig, new, zeros=ZEROS, rolloff=ROLLOFF):
    """-> (L, M, s, W, K)"""
    g = math.gcd(int(orig), int(new))
    L, M = int(new) // g, int(orig) // g
    s = rolloff * min(1.0, L / M)
    W = int(math.ceil(zeros / s))
    return L, M, s, W, 2 * W + 2


def kernel_ref(u, zeros=ZEROS, beta=BETA):
    """sinc(u) times the Kaiser window of half-width `zeros`; exactly 0 at and beyond it"""
    u = np.asarray(u, dtype=np.float64)
    v = u / zeros
    inside = np.abs(v) < 1.0
    win = np.where(inside, np.i0(beta * np.sqrt(np.where(inside, 1.0 - v * v, 0.0))) / np.i0(beta), 0.0)
    return np.sinc(u) * win                              # np.sinc(u) = sin(pi u) / (pi u)


def phase_weights_ref(orig, new, r, zeros=ZEROS, rolloff=ROLLOFF, beta=BETA):
    """the K weights of the outputs j with j mod L == r, tap k first: s * kernel(s * ((W - k) + ((r M) mod L) / L))"""
    L, M, s, W, K = ratio_ref(orig, new, zeros, rolloff)
    return s * kernel_ref(s * ((W - np.arange(K)) + ((r * M) % L) / L), zeros, beta)


def out_len_ref(n, L, M):
    return -((-int(n) * L) // M)


def resample_ref(x, orig, new, zeros=ZEROS, rolloff=ROLLOFF, beta=BETA):
    """float64 (ceil(len L / M),): the sum above, phase by phase (the outputs of one phase share their weights)"""
    x = np.asarray(x, dtype=np.float64)
    L, M, s, W, K = ratio_ref(orig, new, zeros, rolloff)
    n_out = out_len_ref(x.size, L, M)
    y = np.zeros(n_out)
    xp = np.concatenate([np.zeros(W), x, np.zeros(W + 2)])            # xp[i + W] = x[i]
    for r in range(min(L, n_out)):
        js = np.arange(r, n_out, L, dtype=np.int64)
        q = (js * M) // L
        y[js] = xp[q[:, None] + np.arange(K)[None, :]] @ phase_weights_ref(orig, new, r, zeros, rolloff, beta)
    return y


def prototype_ref(orig, new, zeros=ZEROS, rolloff=ROLLOFF, beta=BETA):
    """proto[m + (W + 1) L] = s * kernel(s * m / L), m = -(W + 1) L .. (W + 1) L: the single filter whose polyphase branches are
    the weights above; scipy.signal.resample_poly(x, L, M, window=proto / L) is then the same sum (scipy multiplies explicit
    taps by `up`)"""
    L, M, s, W, K = ratio_ref(orig, new, zeros, rolloff)
    m = np.arange(-(W + 1) * L, (W + 1) * L + 1, dtype=np.float64)
    return s * kernel_ref(s * m / L, zeros, beta)


def stock_weights(table, L, M, K):
    """the conv1d form's kernel (L, 1, K + M - 1) from a tap-major (K, L) table: phase r's taps start floor(r M / L) samples into
    the window that the outputs n L .. n L + L - 1 share (it starts at input n M - W)"""
    import torch
    w = torch.zeros(L, 1, K + M - 1, dtype=table.dtype, device=table.device)
    for r in range(L):
        o = (r * M) // L
        w[r, 0, o:o + K] = table[:, r]
    return w


def stock_resample(x, weights, L, M, K):
    """(B, N) -> (B, ceil(N L / M)) with torch's own operators, in the dtype of `x`: every row at full length"""
    import torch.nn.functional as F
    B, N = x.shape
    W = K // 2 - 1
    n_out = out_len_ref(N, L, M)
    groups = -(-n_out // L)
    need = (groups - 1) * M + K + M - 1                               # padded samples the last window ends at
    xp = F.pad(x, (W, max(0, need - W - N)))
    y = F.conv1d(xp[:, None, :], weights, stride=M)[:, :, :groups]    # (B, L, groups)
    return y.transpose(1, 2).reshape(B, groups * L)[:, :n_out].contiguous()


def make_wave(n, rate, seed):
    """0.3 sin(2 pi 220 t) + 0.05 sin(2 pi 3000 t) + 0.01 N(0, 1), fp32 (the front-end tests' signal)"""
    t = np.arange(n) / float(rate)
    rng = np.random.default_rng(seed)
    x = 0.3 * np.sin(2 * np.pi * 220.0 * t) + 0.05 * np.sin(2 * np.pi * 3000.0 * t) + 0.01 * rng.standard_normal(n)
    return x.astype(np.float32)


def band_limited(n, rate, top, seed, tones=12):
    """a sum of `tones` sines of random phase at frequencies up to `top` Hz, peak below 1, fp32"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / float(rate)
    f = rng.uniform(0.02 * top, top, tones)
    ph = rng.uniform(0.0, 2.0 * np.pi, tones)
    return (np.sin(2 * np.pi * f[:, None] * t[None, :] + ph[:, None]).sum(0) * (0.9 / tones)).astype(np.float32)
