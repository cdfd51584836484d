"""Log-mel front end (csrc/audio.hip, C ABI v23) and Griffin-Lim vocoder (csrc/vocoder.hip, C ABI v24): waveform -> the
model-ready mel batch and back, the counterpart of the reference's `audio.py:15-51,70-75` without librosa.

    fe = MelFrontEnd(config['audio'], device='cuda')          # tables built once (fp64 -> fp32) and uploaded
    out = fe(wave, wave_lens)                                  # {'melspec': (B, Tmax, n_mels) fp32, 'melspec_lens': (B,) int64}
    mag = fe.spectrogram(wave, wave_lens)                      # {'spectrogram': (B, Tmax, n_fft/2+1), 'melspec_lens'}
    s, q, n = fe.stats(out['melspec'], out['melspec_lens'])    # device scalars: sum, sum of squares (fp64), count (int64)
    fe.set_stats(mean, std)                                    # floats or device scalars; later calls normalise

`wave` is (B, Nmax) fp32 on the device, `wave_lens` (B,) integers; samples at or beyond a length are never read.  What is
computed is librosa.stft(center=True, pad_mode='reflect', window='hann') -> abs -> librosa.filters.mel(norm='slaney') ->
log(max(., clip_val)) [-> (x - mean) / (std + 1e-8)], restated from the documented definitions: frame t covers samples
t * hop - n_fft/2 ... + n_fft - 1, indices outside [0, len) reflected without repeating the edge, frames = 1 + len // hop,
Tmax = 1 + Nmax // hop, rows at or beyond a row's frames are zeros.  Nothing is read back: a call captures into a HIP graph.

    voc = Vocoder(config['audio'], device='cuda', n_iter=32, momentum=0.99)   # owns a MelFrontEnd (voc.front_end) and its tables
    out = voc(melspec, melspec_lens)                           # {'wave': (B, (Tmax-1)*hop) fp32, 'wave_lens': (B,) int64}
    voc.magnitude(melspec, melspec_lens)                       # {'spectrogram': (B, Tmax, bins), 'melspec_lens': effective frames}
    voc.griffin_lim(magnitude, frames)                         # the same dict as voc(...), from linear magnitudes
    voc.istft(spectrum, frames) / voc.stft(wave, wave_lens)    # the two transforms on their own (complex64 spectra)

The way back is librosa.feature.inverse.mel_to_audio's fast Griffin-Lim, restated: magnitude = max(pinv(mel basis) @ exp(mel),
floor), then spec = magnitude * init, n_iter times { wave = istft(spec); reb = stft(wave); t = reb - momentum / (1 + momentum) *
prev; prev = reb; spec = magnitude * t / |t| }, wave = istft(spec).  An utterance is vocodable iff (frames - 1) * hop > n_fft/2
(the front end can reflect what comes back); its wave has (frames - 1) * hop samples, any other row 0 samples.

    rs = Resampler(48000, 22050, device='cuda')                # polyphase Kaiser windowed-sinc table built once (fp64 -> fp32)
    out = rs(wave, wave_lens)                                  # {'wave': (B, ceil(Nmax L / M)) fp32, 'wave_lens': (B,) int64}
    samples, rate = read_wav_native(path)                      # a file at its own rate (read_wav refuses another rate)

What `librosa.load(path, sr=...)` does on the way in (csrc/resample.hip): band-limited interpolation, restated from its
definition (`resample_table`); the output is the front end's input as it is, and the vocoder's output resamples the same way.

    pe = PitchEnergy(config['audio'], device='cuda')           # or front_end=fe: that MelFrontEnd's window table, not a copy
    out = pe(wave, wave_lens)                                  # {'f0', 'voiced', 'aperiodicity', 'energy': (B, Tmax); 'frames': (B,)}
    phoneme_average(out['f0'], durations, phoneme_lens, out['frames'], mask=out['voiced'])   # {'mean', 'count'}: (B, Pmax)

Pitch and energy per mel frame and their phoneme means (csrc/pitch.hip): YIN restated from its definition on the front end's
framing, FastSpeech 2's energy as the L2 norm of the front end's STFT frame, one launch over the ragged batch.
"""
from __future__ import annotations

import math
import struct
import wave as _wave
from typing import Dict, Optional, Tuple

import numpy as np

N_FFT = (256, 512, 1024, 2048)                  # audio.hip audio_n_fft_ok
MODES = {"logmel": 0, "magnitude": 1}           # TTTS_AUDIO_LOGMEL / TTTS_AUDIO_MAGNITUDE
MAGIC = 0x4C454D54
HEADER = 8
SPAN_MULT = 2                                   # vocoder.hip VOCODER_SPAN_MULT: an inverse-STFT workgroup owns SPAN_MULT * n_fft samples
MAX_MELS = 512                                  # audio_common.h AUDIO_MAX_MELS
RESAMPLE_ZEROS, RESAMPLE_ROLLOFF, RESAMPLE_BETA = 64, 0.9475937167399596, 14.769656459379492   # the 'kaiser_best' design
RESAMPLE_MAX_L, RESAMPLE_MAX_K, RESAMPLE_MAX_RATIO = 1024, 1280, 8                             # resample.hip RESAMPLE_MAX_*


def hz_to_mel(f):
    """the Slaney scale: linear (200/3 Hz per mel) below 1 kHz, logarithmic (27 mels per factor 6.4) above"""
    f = np.asarray(f, dtype=np.float64)
    lin = f / (200.0 / 3.0)
    log = 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (math.log(6.4) / 27.0)
    return np.where(f >= 1000.0, log, lin)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((math.log(6.4) / 27.0) * (m - 15.0)), (200.0 / 3.0) * m)


def mel_filterbank(sample_rate: float, n_fft: int, n_mels: int, fmin: float = 0.0, fmax: Optional[float] = None) -> np.ndarray:
    """(n_mels, n_fft/2+1) float64: librosa.filters.mel(htk=False, norm='slaney') from its definition.  n_mels + 2 points equally
    spaced in mel between fmin and fmax; weight of bin frequency f in filter i = max(0, min((f - f_i) / (f_{i+1} - f_i),
    (f_{i+2} - f) / (f_{i+2} - f_{i+1}))) * 2 / (f_{i+2} - f_i)."""
    fmax = sample_rate / 2.0 if fmax is None else float(fmax)
    if n_fft < 2 or n_mels < 1 or not 0.0 <= fmin < fmax:
        raise ValueError(f"mel_filterbank: need n_fft >= 2, n_mels >= 1 and 0 <= fmin < fmax (n_fft {n_fft}, n_mels {n_mels}, "
                         f"fmin {fmin}, fmax {fmax})")
    bins = np.linspace(0.0, sample_rate / 2.0, n_fft // 2 + 1)
    edges = mel_to_hz(np.linspace(float(hz_to_mel(fmin)), float(hz_to_mel(fmax)), n_mels + 2))
    width = np.diff(edges)
    ramps = edges[:, None] - bins[None, :]
    lower = -ramps[:-2] / width[:-1, None]
    upper = ramps[2:] / width[1:, None]
    return np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (edges[2:] - edges[:-2]))[:, None]


def inverse_mel_basis(fb: np.ndarray) -> np.ndarray:
    """(bins, n_mels) float32, C-contiguous: numpy.linalg.pinv of the (n_mels, bins) mel basis, formed in float64 and rounded to
    fp32 once"""
    fb = np.asarray(fb, dtype=np.float64)
    if fb.ndim != 2 or min(fb.shape) < 1:
        raise ValueError(f"inverse_mel_basis: the mel basis must be (n_mels, bins), got {fb.shape}")
    return np.ascontiguousarray(np.linalg.pinv(fb).astype(np.float32))


def hann_window(win_length: int, n_fft: int) -> np.ndarray:
    """periodic Hann of win_length, zero-padded to n_fft, left pad (n_fft - win_length) // 2; float64"""
    if not 1 <= win_length <= n_fft:
        raise ValueError(f"win_length must be in [1, n_fft] (win_length {win_length}, n_fft {n_fft})")
    w = np.zeros(n_fft, dtype=np.float64)
    left = (n_fft - win_length) // 2
    w[left:left + win_length] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_length) / win_length)
    return w


def pack_filters(fb: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """dense (n_mels, bins) -> (first, count, offset int32 arrays, weights fp32): per row the span from its first to its last
    non-zero weight (an all-zero row: count 0)"""
    first, count, weights = [], [], []
    for row in fb:
        nz = np.flatnonzero(row)
        a, n = (int(nz[0]), int(nz[-1]) - int(nz[0]) + 1) if nz.size else (0, 0)
        first.append(a)
        count.append(n)
        weights.append(row[a:a + n])
    count = np.asarray(count, dtype=np.int32)
    offset = (np.cumsum(count) - count).astype(np.int32)
    return np.asarray(first, dtype=np.int32), count, offset, np.concatenate(weights).astype(np.float32)


def unpack_filters(first, count, offset, weights, bins: int) -> np.ndarray:
    fb = np.zeros((len(first), bins), dtype=np.float32)
    for f, (a, n, o) in enumerate(zip(first, count, offset)):
        fb[f, a:a + n] = weights[o:o + n]
    return fb


def table_layout(n_fft: int, n_mels: int, nnz: int) -> Dict[str, int]:
    """word offsets of the sections of the table buffer (audio.hip audio_tables)"""
    M = n_fft // 2
    lay, at = {}, HEADER
    for name, n in (("window", n_fft), ("tw_re", M), ("tw_im", M), ("pw_re", M // 2 + 1), ("pw_im", M // 2 + 1), ("first", n_mels),
                    ("count", n_mels), ("offset", n_mels), ("weights", nnz)):
        lay[name] = at
        at += n
    lay["words"] = at
    return lay


def build_tables(n_fft: int, win_length: int, fb: np.ndarray) -> Tuple[np.ndarray, int]:
    """the kernel's table buffer as int32 words (every value built in float64 and rounded to fp32 once) and its nnz"""
    if n_fft not in N_FFT:
        raise ValueError(f"n_fft must be one of {N_FFT}, got {n_fft}")
    M = n_fft // 2
    if fb.shape[1] != M + 1:
        raise ValueError(f"the filter bank must have n_fft/2+1 = {M + 1} columns, got {fb.shape}")
    first, count, offset, weights = pack_filters(fb)
    nnz = int(weights.size)
    if nnz < 1:
        raise ValueError("the filter bank is empty")
    lay = table_layout(n_fft, fb.shape[0], nnz)
    buf = np.zeros(lay["words"], dtype=np.int32)
    buf[:5] = np.asarray([MAGIC, n_fft, win_length, fb.shape[0], nnz], dtype=np.int64).astype(np.int32)
    f32 = buf.view(np.float32)
    k = np.arange(M, dtype=np.float64)
    f32[lay["window"]:lay["window"] + n_fft] = hann_window(win_length, n_fft)
    f32[lay["tw_re"]:lay["tw_re"] + M] = np.cos(2.0 * np.pi * k / M)
    f32[lay["tw_im"]:lay["tw_im"] + M] = -np.sin(2.0 * np.pi * k / M)
    k = np.arange(M // 2 + 1, dtype=np.float64)
    f32[lay["pw_re"]:lay["pw_re"] + M // 2 + 1] = np.cos(2.0 * np.pi * k / n_fft)
    f32[lay["pw_im"]:lay["pw_im"] + M // 2 + 1] = -np.sin(2.0 * np.pi * k / n_fft)
    for name, arr in (("first", first), ("count", count), ("offset", offset)):
        buf[lay[name]:lay[name] + arr.size] = arr
    f32[lay["weights"]:lay["weights"] + nnz] = weights
    return buf, nnz


def normalize(mel, mean, std):
    return (mel - mean) / (std + 1e-8)


def denormalize(mel, mean, std):
    return (mel * (std + 1e-8)) + mean


def read_wav(path: str, sample_rate: int) -> np.ndarray:
    """mono RIFF PCM16 / PCM24 / PCM32 / IEEE float32 -> float32 in [-1, 1); raises if the file's rate is not `sample_rate`
    (nothing is resampled here: `read_wav_native` returns the file's own rate, `Resampler` converts on the device) or it is
    not mono.  Standard library only."""
    return _read_wav(path, sample_rate)[0]


def read_wav_native(path: str) -> Tuple[np.ndarray, int]:
    """-> (samples as `read_wav` returns them, the file's sample rate): the same reader without the rate check"""
    return _read_wav(path, None)


def _read_wav(path: str, sample_rate: Optional[int]) -> Tuple[np.ndarray, int]:
    with open(path, "rb") as fh:
        head = fh.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"WAVE":
            raise ValueError(f"read_wav: {path} is not a RIFF/WAVE file")
        fmt = data = None
        while True:
            ck = fh.read(8)
            if len(ck) < 8:
                break
            tag, size = ck[:4], struct.unpack("<I", ck[4:])[0]
            if tag == b"fmt ":
                fmt = fh.read(size)
            elif tag == b"data":
                data = fh.read(size)
            else:
                fh.seek(size, 1)
            if size & 1:
                fh.seek(1, 1)
            if fmt is not None and data is not None:
                break
    if fmt is None or data is None or len(fmt) < 16:
        raise ValueError(f"read_wav: {path} has no fmt or data chunk")
    code, channels, rate, _, _, bits = struct.unpack("<HHIIHH", fmt[:16])
    if code == 0xFFFE and len(fmt) >= 26:        # WAVE_FORMAT_EXTENSIBLE: the sub-format's first two bytes
        code = struct.unpack("<H", fmt[24:26])[0]
    if channels != 1:
        raise ValueError(f"read_wav: {path} has {channels} channels, mono expected")
    if sample_rate is not None and rate != int(sample_rate):
        raise ValueError(f"read_wav: {path} is sampled at {rate} Hz, {int(sample_rate)} Hz expected (there is no resampler)")
    if code == 1 and bits == 16:
        return np.frombuffer(data[:len(data) // 2 * 2], dtype="<i2").astype(np.float32) / np.float32(32768.0), int(rate)
    if code == 1 and bits == 24:
        raw = np.frombuffer(data[:len(data) // 3 * 3], dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        v = raw[:, 0] | (raw[:, 1] << 8) | (raw[:, 2] << 16)
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        return (v.astype(np.float64) / float(1 << 23)).astype(np.float32), int(rate)
    if code == 1 and bits == 32:
        return (np.frombuffer(data[:len(data) // 4 * 4], dtype="<i4").astype(np.float64) / float(1 << 31)).astype(np.float32), int(rate)
    if code == 3 and bits == 32:
        return np.frombuffer(data[:len(data) // 4 * 4], dtype="<f4").astype(np.float32), int(rate)
    raise ValueError(f"read_wav: {path}: format code {code} with {bits} bits is not PCM16/24/32 or float32")


def write_wav_pcm16(path: str, samples: np.ndarray, sample_rate: int) -> None:
    """mono PCM16 through the standard library's `wave` (tests and examples)"""
    pcm = np.clip(np.round(np.asarray(samples, dtype=np.float64) * 32768.0), -32768, 32767).astype("<i2")
    with _wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(int(sample_rate))
        w.writeframes(pcm.tobytes())


def bessel_i0(x):
    """the modified Bessel function I0 by its power series sum_n ((x/2)^2)^n / (n!)^2, in float64 (every term is positive: no
    cancellation; 60 terms reach 1e-17 of the sum up to |x| = 20 and the loop stops there)"""
    x = np.asarray(x, dtype=np.float64)
    y = (x / 2.0) ** 2
    term = np.ones_like(y)
    total = np.ones_like(y)
    for n in range(1, 500):
        term = term * y / float(n * n)
        total = total + term
        if not np.any(term > 1e-17 * total):
            break
    return total


def resample_ratio(orig_rate: int, new_rate: int) -> Tuple[int, int]:
    """-> (L, M) = (new, orig) / gcd(orig, new)"""
    orig, new = int(orig_rate), int(new_rate)
    if orig < 1 or new < 1 or orig != orig_rate or new != new_rate:
        raise ValueError(f"resample: the rates must be positive integers (orig_rate {orig_rate}, new_rate {new_rate})")
    g = math.gcd(orig, new)
    return new // g, orig // g


def resample_table(orig_rate: int, new_rate: int, zeros: int = RESAMPLE_ZEROS, rolloff: float = RESAMPLE_ROLLOFF,
                   beta: float = RESAMPLE_BETA) -> Tuple[np.ndarray, int, int, int]:
    """-> (table fp32 (K, L) C-contiguous, L, M, K): the polyphase weights of csrc/resample.hip, tap-major (table[k, r] is
    tap k of phase r = j mod L), built in float64 and rounded to fp32 once.  s = rolloff * min(1, L / M), W = ceil(zeros / s),
    K = 2 W + 2, h[r][k] = s * kernel(s * ((W - k) + ((r M) mod L) / L)), kernel(u) = sinc(u) * I0(beta sqrt(1 - (u / zeros)^2)) /
    I0(beta) inside |u| < zeros and exactly 0 outside."""
    L, M = resample_ratio(orig_rate, new_rate)
    if L == M:
        raise ValueError(f"resample_table: the two rates are equal ({orig_rate}): there is nothing to interpolate")
    zeros = int(zeros)
    if zeros < 1 or not 0.0 < rolloff <= 1.0 or not beta >= 0.0:
        raise ValueError(f"resample_table: need zeros >= 1, 0 < rolloff <= 1 and beta >= 0 (zeros {zeros}, rolloff {rolloff}, "
                         f"beta {beta})")
    s = float(rolloff) * min(1.0, L / M)
    W = int(math.ceil(zeros / s))
    K = 2 * W + 2
    if L > RESAMPLE_MAX_L or K > RESAMPLE_MAX_K or max(L, M) > RESAMPLE_MAX_RATIO * min(L, M):
        raise ValueError(f"resample_table: {orig_rate} -> {new_rate} Hz needs L {L}, M {M}, K {K}; the kernel takes L <= "
                         f"{RESAMPLE_MAX_L}, K <= {RESAMPLE_MAX_K} and rates within a factor of {RESAMPLE_MAX_RATIO}")
    frac = ((np.arange(L, dtype=np.int64) * M) % L).astype(np.float64) / L
    u = s * ((W - np.arange(K, dtype=np.float64))[:, None] + frac[None, :])               # (K, L)
    v = u / zeros
    inside = np.abs(v) < 1.0
    window = np.where(inside, bessel_i0(beta * np.sqrt(np.where(inside, 1.0 - v * v, 0.0))) / bessel_i0(beta), 0.0)
    return np.ascontiguousarray((s * np.sinc(u) * window).astype(np.float32)), L, M, K


class Resampler:
    """Band-limited (Kaiser windowed-sinc, polyphase) resampling of a ragged batch on the device: one launch of csrc/resample.hip
    a call, nothing read back, capturable into a HIP graph.

        rs = Resampler(16000, 22050, device='cuda')        # table built once (fp64 -> fp32) and uploaded
        out = rs(wave, wave_lens)                          # {'wave': (B, ceil(Nmax L / M)) fp32, 'wave_lens': (B,) int64}
        mel = MelFrontEnd(cfg)(**out)                      # the output is the front end's input as it is

    Output j sits at input time j M / L (L / M = new / orig in lowest terms); a row of len samples gives ceil(len L / M), the
    rest of its row zeros; samples at or behind a length are never read.  Equal rates: no launch, the input tensor comes back
    with its lengths clamped to [0, Nmax]."""

    def __init__(self, orig_rate: int, new_rate: int, device=None, zeros: int = RESAMPLE_ZEROS, rolloff: float = RESAMPLE_ROLLOFF,
                 beta: float = RESAMPLE_BETA):
        import torch
        self.orig_rate, self.new_rate = int(orig_rate), int(new_rate)
        self.L, self.M = resample_ratio(orig_rate, new_rate)
        self.K, self.table_host, self.table = 0, None, None
        if self.L == self.M:                               # the identity needs neither a table nor the library
            self.device = torch.device(device) if device is not None else None
            return
        from . import _lib
        self.table_host, _, _, self.K = resample_table(orig_rate, new_rate, zeros, rolloff, beta)
        lib = _lib.load()
        if lib.ttts_resample_table_bytes(self.L, self.K) != self.table_host.nbytes:
            raise RuntimeError("Resampler: the table layout disagrees with the library")
        _lib.check(lib.ttts_resample_table_check(self.table_host.ctypes.data, self.table_host.nbytes, self.L, self.M, self.K),
                   "ttts_resample_table_check")
        if not torch.cuda.is_available():
            raise RuntimeError("Resampler needs the HIP device (no CPU fallback)")
        self.device = torch.device(device if device is not None else "cuda")
        self.table = torch.from_numpy(self.table_host).to(self.device)

    def out_len(self, n: int) -> int:
        """samples a row of n samples comes back with: ceil(n L / M)"""
        return -((-int(n) * self.L) // self.M)

    def __call__(self, wave, wave_lens):
        import torch
        if wave.dim() != 2 or min(wave.shape) < 1:
            raise ValueError(f"Resampler: wave must be (B, Nmax), got {tuple(wave.shape)}")
        B, Nmax = wave.shape
        if tuple(wave_lens.shape) != (B,):
            raise ValueError(f"Resampler.wave_lens must have shape ({B},), got {tuple(wave_lens.shape)}")
        identity = self.L == self.M
        if not wave.is_cuda and not identity:
            raise ValueError(f"Resampler.wave: expected a CUDA/HIP tensor (the HIP path has no CPU fallback), got {wave.device}")
        if wave.dtype != torch.float32:
            raise ValueError(f"Resampler.wave: expected dtype {torch.float32}, got {wave.dtype}")
        if wave_lens.dtype.is_floating_point or wave_lens.dtype == torch.bool:
            raise ValueError(f"Resampler.wave_lens must be integers, got {wave_lens.dtype}")
        lens = wave_lens.to(wave.device).to(torch.int64).contiguous()
        if identity:
            return {"wave": wave, "wave_lens": lens.clamp(0, Nmax)}
        from . import _lib
        from .ops import _p, _stream
        wave = wave.detach()
        if (Nmax > 1 and wave.stride(1) != 1) or (B > 1 and wave.stride(0) < Nmax):
            wave = wave.contiguous()
        ld = wave.stride(0) if B > 1 else Nmax
        Nout = self.out_len(Nmax)
        out = torch.empty(B, Nout, dtype=torch.float32, device=wave.device)
        out_lens = torch.empty(B, dtype=torch.int64, device=wave.device)
        _lib.check(_lib.load().ttts_resample(_p(wave), ld, _p(lens), B, Nmax, self.L, self.M, self.K, _p(self.table), _p(out), Nout,
                                             _p(out_lens), _stream()), "ttts_resample")
        return {"wave": out, "wave_lens": out_lens}


class MelFrontEnd:
    """Tables for one audio config, built once; every call is one kernel launch (two for `stats`)."""

    def __init__(self, audio_config: Dict, device=None, mean=None, std=None, clip_val: float = 1e-5):
        import torch
        from . import _lib
        c = audio_config
        self.sample_rate = int(c["sample_rate"])
        self.n_fft, self.hop = int(c["n_fft"]), int(c["hop_length"])
        self.win_length = int(c.get("win_length") or self.n_fft)
        self.n_mels = int(c["n_mels"])
        self.fmin = float(c.get("fmin", 0.0))
        self.fmax = float(c["fmax"]) if c.get("fmax") is not None else self.sample_rate / 2.0
        self.clip_val = float(clip_val)
        if self.n_fft not in N_FFT:
            raise ValueError(f"MelFrontEnd: n_fft must be one of {N_FFT}, got {self.n_fft}")
        if not 1 <= self.hop <= self.n_fft:
            raise ValueError(f"MelFrontEnd: hop_length must be in [1, n_fft] (hop_length {self.hop}, n_fft {self.n_fft})")
        if not 1 <= self.win_length <= self.n_fft:
            raise ValueError(f"MelFrontEnd: win_length must be in [1, n_fft] (win_length {self.win_length}, n_fft {self.n_fft})")
        self.filterbank = mel_filterbank(self.sample_rate, self.n_fft, self.n_mels, self.fmin, self.fmax)
        self.tables_host, self.nnz = build_tables(self.n_fft, self.win_length, self.filterbank)
        lib = _lib.load()
        nbytes = self.tables_host.nbytes
        if lib.ttts_audio_tables_bytes(self.n_fft, self.n_mels, self.nnz) != nbytes:
            raise RuntimeError("MelFrontEnd: the table layout disagrees with the library")
        _lib.check(lib.ttts_audio_tables_check(self.tables_host.ctypes.data, nbytes, self.n_fft, self.win_length, self.n_mels, self.nnz),
                   "ttts_audio_tables_check")
        if not torch.cuda.is_available():
            raise RuntimeError("MelFrontEnd needs the HIP device (no CPU fallback)")
        self.device = torch.device(device if device is not None else "cuda")
        self.tables = torch.from_numpy(self.tables_host).to(self.device)
        self.mean_std = None
        if (mean is None) != (std is None):
            raise ValueError("MelFrontEnd: give both `mean` and `std`, or neither")
        if mean is not None:
            self.set_stats(mean, std)

    # ------------------------------------------------------------------ statistics
    def set_stats(self, mean, std) -> None:
        """normalise from now on with (x - mean) / (std + 1e-8); floats, or device scalars (then nothing is read back).  The two
        values live in one device buffer that is overwritten in place, so a captured call follows them.  None, None: stop."""
        import torch
        if mean is None and std is None:
            self.mean_std = None
            return
        if self.mean_std is None:
            self.mean_std = torch.empty(2, dtype=torch.float32, device=self.device)
        for i, v in enumerate((mean, std)):
            if isinstance(v, torch.Tensor):
                self.mean_std[i].copy_(v.reshape(()).to(torch.float32))
            else:
                self.mean_std[i] = float(v)

    def stats(self, melspec, melspec_lens):
        """-> (sum, sum of squares, count) of the valid rows of an UNNORMALISED log-mel batch: fp64, fp64, int64 device scalars.
        Per utterance in a fixed order on the device (ttts_logmel_stats), utterances added in fp64."""
        import torch
        from . import _lib
        from .ops import _p, _stream
        self._chk(melspec, "stats.melspec", torch.float32)
        if melspec.dim() != 3 or melspec.size(2) != self.n_mels or min(melspec.shape) < 1:
            raise ValueError(f"stats: melspec must be (B, T, {self.n_mels}), got {tuple(melspec.shape)}")
        B, T, _ = melspec.shape
        lens = self._lens(melspec_lens, B, "stats.melspec_lens")
        mel = melspec.detach().contiguous()
        sums = torch.empty(B, 2, dtype=torch.float64, device=mel.device)
        _lib.check(_lib.load().ttts_logmel_stats(_p(mel), _p(lens), B, T, self.n_mels, _p(sums), _stream()), "ttts_logmel_stats")
        total = sums.sum(0)
        return total[0], total[1], lens.clamp(0, T).sum() * self.n_mels

    @staticmethod
    def mean_std_from(total, total_sq, count):
        """preprocess.py:59-61: mean = S / n, std = sqrt(Q / n - mean^2 + 1e-8); works on floats and on device scalars"""
        mean = total / count
        var = total_sq / count - mean ** 2
        return mean, (var + 1e-8) ** 0.5

    # ------------------------------------------------------------------ the two calls
    def _chk(self, t, name, dtype):
        if not t.is_cuda:
            raise ValueError(f"MelFrontEnd.{name}: expected a CUDA/HIP tensor (the HIP path has no CPU fallback), got {t.device}")
        if t.dtype != dtype:
            raise ValueError(f"MelFrontEnd.{name}: expected dtype {dtype}, got {t.dtype}")

    def _lens(self, lens, B, name):
        import torch
        if tuple(lens.shape) != (B,):
            raise ValueError(f"MelFrontEnd.{name} must have shape ({B},), got {tuple(lens.shape)}")
        if lens.dtype.is_floating_point or lens.dtype == torch.bool:
            raise ValueError(f"MelFrontEnd.{name} must be integers, got {lens.dtype}")
        if not lens.is_cuda:                       # host lengths: the one place the unreflectable length can be refused
            if lens.numel() and int(lens.min()) <= self.n_fft // 2 and "wave" in name:
                raise ValueError(f"MelFrontEnd.{name}: an utterance of {int(lens.min())} samples cannot be reflected "
                                 f"(n_fft/2 + 1 = {self.n_fft // 2 + 1} at the least)")
            lens = lens.to(self.device)
        return lens.to(torch.int64).contiguous()

    def _run(self, wave, wave_lens, mode: str):
        import torch
        from . import _lib
        from .ops import _p, _stream
        if wave.dim() != 2 or min(wave.shape) < 1:
            raise ValueError(f"MelFrontEnd: wave must be (B, Nmax), got {tuple(wave.shape)}")
        self._chk(wave, "wave", torch.float32)
        B, Nmax = wave.shape
        lens = self._lens(wave_lens, B, "wave_lens")
        wave = wave.detach()
        if (Nmax > 1 and wave.stride(1) != 1) or (B > 1 and wave.stride(0) < Nmax):
            wave = wave.contiguous()
        ld = wave.stride(0) if B > 1 else Nmax
        Tmax = 1 + Nmax // self.hop
        width = self.n_mels if mode == "logmel" else self.n_fft // 2 + 1
        out = torch.empty(B, Tmax, width, dtype=torch.float32, device=wave.device)
        mel_lens = torch.empty(B, dtype=torch.int64, device=wave.device)
        _lib.check(_lib.load().ttts_logmel(_p(wave), ld, _p(lens), B, Nmax, self.n_fft, self.hop, self.n_mels, self.nnz, _p(self.tables),
                                           self.clip_val, _p(self.mean_std), _p(out), _p(mel_lens), MODES[mode], _stream()),
                   "ttts_logmel")
        return out, mel_lens

    def __call__(self, wave, wave_lens):
        mel, lens = self._run(wave, wave_lens, "logmel")
        return {"melspec": mel, "melspec_lens": lens}

    def spectrogram(self, wave, wave_lens):
        mag, lens = self._run(wave, wave_lens, "magnitude")
        return {"spectrogram": mag, "melspec_lens": lens}


class Vocoder:
    """Griffin-Lim on the front end's tables; a call is one magnitude launch and 2 n_iter + 1 transform launches, nothing is read
    back.  With an explicit `init` the whole call captures into a HIP graph (the default init draws from a torch.Generator)."""

    def __init__(self, audio_config: Dict, device=None, mean=None, std=None, n_iter: int = 32, momentum: float = 0.99,
                 floor: float = 1e-10):
        import torch
        from . import _lib
        self.n_iter, self.momentum, self.floor = int(n_iter), float(momentum), float(floor)
        if self.n_iter < 0:
            raise ValueError(f"Vocoder: n_iter must be >= 0, got {n_iter}")
        if not 0.0 <= self.momentum < 1.0:
            raise ValueError(f"Vocoder: momentum must be in [0, 1), got {momentum}")
        if not self.floor > 0.0:
            raise ValueError(f"Vocoder: floor must be positive, got {floor}")
        if int(audio_config["n_mels"]) > MAX_MELS:
            raise ValueError(f"Vocoder: at most {MAX_MELS} mel filters, got {audio_config['n_mels']}")
        self.front_end = MelFrontEnd(audio_config, device=device, mean=mean, std=std)
        fe = self.front_end
        self.n_fft, self.hop, self.n_mels, self.bins, self.device = fe.n_fft, fe.hop, fe.n_mels, fe.n_fft // 2 + 1, fe.device
        self.sample_rate = fe.sample_rate
        self.span = SPAN_MULT * self.n_fft
        self.pinv_host = inverse_mel_basis(fe.filterbank)
        _lib.check(_lib.load().ttts_vocoder_pinv_check(self.pinv_host.ctypes.data, self.pinv_host.nbytes, self.n_fft, self.n_mels),
                   "ttts_vocoder_pinv_check")
        self.pinv = torch.from_numpy(self.pinv_host).to(self.device)

    def set_stats(self, mean, std) -> None:
        """the front end's statistics: one buffer, seen by both directions"""
        self.front_end.set_stats(mean, std)

    @property
    def mean_std(self):
        return self.front_end.mean_std

    # ------------------------------------------------------------------ checks
    def _chk(self, t, name, dtype):
        if not t.is_cuda:
            raise ValueError(f"Vocoder.{name}: expected a CUDA/HIP tensor (the HIP path has no CPU fallback), got {t.device}")
        if t.dtype != dtype:
            raise ValueError(f"Vocoder.{name}: expected dtype {dtype}, got {t.dtype}")

    def _lens(self, lens, B, name):
        import torch
        if tuple(lens.shape) != (B,):
            raise ValueError(f"Vocoder.{name} must have shape ({B},), got {tuple(lens.shape)}")
        if lens.dtype.is_floating_point or lens.dtype == torch.bool:
            raise ValueError(f"Vocoder.{name} must be integers, got {lens.dtype}")
        return lens.to(self.device).to(torch.int64).contiguous()

    def _frames3(self, x, width, what, name):
        if x.dim() != 3 or x.size(2) != width or min(x.shape) < 1:
            raise ValueError(f"Vocoder: {name} must be (B, Tmax, {width}) {what}, got {tuple(x.shape)}")
        if x.size(1) < 2:
            raise ValueError(f"Vocoder: {name} needs Tmax >= 2 rows, got {tuple(x.shape)}")

    # ------------------------------------------------------------------ the steps
    def magnitude(self, melspec, melspec_lens):
        """(normalised) log-mel -> linear magnitudes max(pinv @ exp(mel), floor) and the effective frames (0 for a row that
        cannot be vocoded)"""
        import torch
        from . import _lib
        from .ops import _p, _stream
        self._frames3(melspec, self.n_mels, "log-mels", "melspec")
        self._chk(melspec, "melspec", torch.float32)
        B, Tmax, _ = melspec.shape
        lens = self._lens(melspec_lens, B, "melspec_lens")
        mel = melspec.detach()
        if mel.stride(2) != 1 or mel.stride(1) < self.n_mels or (B > 1 and mel.stride(0) < (Tmax - 1) * mel.stride(1) + self.n_mels):
            mel = mel.contiguous()
        mag = torch.empty(B, Tmax, self.bins, dtype=torch.float32, device=mel.device)
        frames = torch.empty(B, dtype=torch.int64, device=mel.device)
        _lib.check(_lib.load().ttts_mel_to_magnitude(_p(mel), mel.stride(1), mel.stride(0), _p(lens), B, Tmax, self.n_fft, self.hop,
                                                     self.n_mels, _p(self.pinv), _p(self.mean_std), self.floor, _p(mag), _p(frames),
                                                     _stream()), "ttts_mel_to_magnitude")
        return {"spectrogram": mag, "melspec_lens": frames}

    def _istft(self, spec, frames, B, Tmax):
        """spec: (B, Tmax, bins, 2) fp32 contiguous"""
        import torch
        from . import _lib
        from .ops import _p, _stream
        wave = torch.empty(B, (Tmax - 1) * self.hop, dtype=torch.float32, device=spec.device)
        wave_lens = torch.empty(B, dtype=torch.int64, device=spec.device)
        _lib.check(_lib.load().ttts_istft(_p(spec), _p(frames), B, Tmax, self.n_fft, self.hop, _p(self.front_end.tables), _p(wave),
                                          _p(wave_lens), _stream()), "ttts_istft")
        return wave, wave_lens

    def istft(self, spectrum, frames):
        """complex64 (B, Tmax, bins) and the rows' frames -> {'wave': (B, (Tmax-1)*hop), 'wave_lens': (frames - 1) * hop};
        least-squares overlap-add with the front end's window, the n_fft/2 samples of centring removed"""
        import torch
        self._frames3(spectrum, self.bins, "complex64", "spectrum")
        self._chk(spectrum, "spectrum", torch.complex64)
        B, Tmax, _ = spectrum.shape
        frames = self._lens(frames, B, "frames")
        spec = torch.view_as_real(spectrum.detach().contiguous())
        wave, wave_lens = self._istft(spec, frames, B, Tmax)
        return {"wave": wave, "wave_lens": wave_lens}

    def stft(self, wave, wave_lens):
        """(B, Nmax) fp32 -> {'spectrum': complex64 (B, 1 + Nmax // hop, bins), 'melspec_lens'}: the front end's transform with
        its phases (framing, reflection, window and frame count as MelFrontEnd)"""
        import torch
        from . import _lib
        from .ops import _p, _stream
        if wave.dim() != 2 or min(wave.shape) < 1:
            raise ValueError(f"Vocoder: wave must be (B, Nmax), got {tuple(wave.shape)}")
        if wave.size(1) < self.hop:
            raise ValueError(f"Vocoder: wave needs Nmax >= hop_length = {self.hop} samples (two frames), got {tuple(wave.shape)}")
        self._chk(wave, "wave", torch.float32)
        B, Nmax = wave.shape
        lens = self._lens(wave_lens, B, "wave_lens")
        wave = wave.detach()
        if (Nmax > 1 and wave.stride(1) != 1) or (B > 1 and wave.stride(0) < Nmax):
            wave = wave.contiguous()
        ld = wave.stride(0) if B > 1 else Nmax
        Tmax = 1 + Nmax // self.hop
        spec = torch.empty(B, Tmax, self.bins, 2, dtype=torch.float32, device=wave.device)
        frames = torch.empty(B, dtype=torch.int64, device=wave.device)
        _lib.check(_lib.load().ttts_stft_project(_p(wave), ld, _p(lens), None, B, Nmax, self.n_fft, self.hop, _p(self.front_end.tables),
                                                 None, None, 0.0, _p(spec), _p(frames), _stream()), "ttts_stft_project")
        return {"spectrum": torch.view_as_complex(spec), "melspec_lens": frames}

    def _init(self, init, B, Tmax, seed):
        import torch
        if init is None:
            gen = torch.Generator(device=self.device)
            gen.manual_seed(int(seed))
            angle = torch.rand(B, Tmax, self.bins, generator=gen, dtype=torch.float32, device=self.device) * (2.0 * math.pi)
            return torch.polar(torch.ones_like(angle), angle)
        if tuple(init.shape) != (B, Tmax, self.bins):
            raise ValueError(f"Vocoder: init must be (B, Tmax, bins) = ({B}, {Tmax}, {self.bins}), got {tuple(init.shape)}")
        self._chk(init, "init", torch.complex64)
        return init.detach()

    def _griffin_lim(self, mag, frames, init, seed):
        """mag: (B, Tmax, bins) fp32 contiguous; frames: the EFFECTIVE frames (int64, device)"""
        import torch
        from . import _lib
        from .ops import _p, _stream
        B, Tmax, _ = mag.shape
        init = self._init(init, B, Tmax, seed)
        spec = torch.view_as_real(init * mag).contiguous()            # unit phases times the magnitudes, once per call
        prev = torch.zeros_like(spec) if self.momentum > 0.0 and self.n_iter > 0 else None
        lib, tables = _lib.load(), self.front_end.tables
        Nmax = (Tmax - 1) * self.hop
        for _ in range(self.n_iter):
            wave, _lens = self._istft(spec, frames, B, Tmax)
            _lib.check(lib.ttts_stft_project(_p(wave), Nmax, None, _p(frames), B, Nmax, self.n_fft, self.hop, _p(tables), _p(mag),
                                             _p(prev), self.momentum if prev is not None else 0.0, _p(spec), None, _stream()),
                       "ttts_stft_project")
        wave, wave_lens = self._istft(spec, frames, B, Tmax)
        return {"wave": wave, "wave_lens": wave_lens}

    def griffin_lim(self, magnitude, frames, init=None, seed: int = 0):
        """linear magnitudes (B, Tmax, bins) fp32 and the rows' frames -> {'wave', 'wave_lens'}; rows that cannot be vocoded
        ((frames - 1) * hop <= n_fft/2) come back as 0 samples"""
        import torch
        self._frames3(magnitude, self.bins, "magnitudes", "magnitude")
        self._chk(magnitude, "magnitude", torch.float32)
        B, Tmax, _ = magnitude.shape
        frames = self._lens(frames, B, "frames").clamp(0, Tmax)
        frames = torch.where((frames - 1) * self.hop > self.n_fft // 2, frames, torch.zeros_like(frames))
        return self._griffin_lim(magnitude.detach().contiguous(), frames, init, seed)

    def __call__(self, melspec, melspec_lens, init=None, seed: int = 0):
        m = self.magnitude(melspec, melspec_lens)
        return self._griffin_lim(m["spectrogram"], m["melspec_lens"], init, seed)


PITCH_MAX_FRAME = 4096                          # pitch.hip PITCH_MAX_F


def pitch_lags(sample_rate: float, fmin: float, fmax: float) -> Tuple[int, int]:
    """-> (tau_min, tau_max) = (floor(sr / fmax), ceil(sr / fmin)): the lags YIN searches"""
    if not 0.0 < fmin < fmax:
        raise ValueError(f"PitchEnergy: need 0 < fmin < fmax (fmin {fmin}, fmax {fmax})")
    return int(math.floor(sample_rate / fmax)), int(math.ceil(sample_rate / fmin))


class PitchEnergy:
    """YIN F0, voicing, aperiodicity and the STFT frame energy of a ragged batch on the device: one launch of csrc/pitch.hip a
    call, nothing read back, capturable into a HIP graph.

        pe = PitchEnergy(config['audio'], device='cuda')   # or front_end=fe: shares that MelFrontEnd's window table
        out = pe(wave, wave_lens)                          # {'f0', 'voiced' (bool), 'aperiodicity', 'energy': (B, Tmax); 'frames': (B,)}

    `wave`, `wave_lens` exactly as MelFrontEnd takes them; frame t is mel frame t (centred at t * hop, reflected ends), frames =
    1 + len // hop, 0 for len <= max(frame_length, n_fft) / 2, rows at or beyond a row's frames are zeros.  d(tau) = sum_{j < window}
    (x_j - x_{j+tau})^2 as differences squared, d' = d tau / running sum, the first lag in [tau_min, tau_max] under `threshold`
    followed down its dip, a parabola through its neighbours; unvoiced frames carry f0 = 0 and the minimum of d' as aperiodicity.
    energy is the L2 norm of the front end's STFT frame (FastSpeech 2's)."""

    def __init__(self, audio_config: Dict, fmin: float = 65.0, fmax: float = 600.0, frame_length: Optional[int] = None,
                 window: Optional[int] = None, threshold: float = 0.1, device=None, front_end: Optional["MelFrontEnd"] = None):
        import torch
        c = audio_config
        self.sample_rate = int(c["sample_rate"])
        self.n_fft, self.hop = int(c["n_fft"]), int(c["hop_length"])
        self.win_length = int(c.get("win_length") or self.n_fft)
        self.fmin, self.fmax, self.threshold = float(fmin), float(fmax), float(threshold)
        self.frame_length = self.n_fft if frame_length is None else int(frame_length)
        self.window = self.frame_length // 2 if window is None else int(window)
        F, W = self.frame_length, self.window
        if self.n_fft not in N_FFT:
            raise ValueError(f"PitchEnergy: n_fft must be one of {N_FFT}, got {self.n_fft}")
        if not 1 <= self.win_length <= self.n_fft:
            raise ValueError(f"PitchEnergy: win_length must be in [1, n_fft] (win_length {self.win_length}, n_fft {self.n_fft})")
        if F < 2 or F % 2 or F > PITCH_MAX_FRAME:
            raise ValueError(f"PitchEnergy: frame_length must be even and in [2, {PITCH_MAX_FRAME}], got {F}")
        if not 1 <= self.hop <= F:
            raise ValueError(f"PitchEnergy: hop_length must be in [1, frame_length] (hop_length {self.hop}, frame_length {F})")
        if W < 1:
            raise ValueError(f"PitchEnergy: window must be positive, got {W}")
        self.tau_min, self.tau_max = pitch_lags(self.sample_rate, self.fmin, self.fmax)
        if self.tau_min < 2:
            raise ValueError(f"PitchEnergy: tau_min = floor(sample_rate / fmax) must be at least 2, got {self.tau_min} "
                             f"(sample_rate {self.sample_rate}, fmax {self.fmax})")
        if self.tau_min >= self.tau_max:
            raise ValueError(f"PitchEnergy: tau_min must be below tau_max (tau_min {self.tau_min}, tau_max {self.tau_max})")
        if W + self.tau_max > F:
            raise ValueError(f"PitchEnergy: window + tau_max must fit the frame (window {W}, tau_max = ceil(sample_rate / fmin) = "
                             f"{self.tau_max}, frame_length {F})")
        if not 0.0 < self.threshold < 1.0:
            raise ValueError(f"PitchEnergy: threshold must be in (0, 1), got {threshold}")
        if front_end is not None:
            if (front_end.n_fft, front_end.win_length, front_end.hop, front_end.sample_rate) != (self.n_fft, self.win_length, self.hop,
                                                                                               self.sample_rate):
                raise ValueError("PitchEnergy: front_end was built for another audio config (n_fft, win_length, hop_length, "
                                 f"sample_rate {front_end.n_fft}, {front_end.win_length}, {front_end.hop}, {front_end.sample_rate})")
            if device is not None and torch.device(device).type != front_end.device.type:
                raise ValueError(f"PitchEnergy: front_end lives on {front_end.device}, device is {device}")
            self.front_end, self.device = front_end, front_end.device
            self.hann = front_end.tables[HEADER:HEADER + self.n_fft].view(torch.float32)      # the window section, not a copy
        else:
            if not torch.cuda.is_available():
                raise RuntimeError("PitchEnergy needs the HIP device (no CPU fallback)")
            self.front_end, self.device = None, torch.device(device if device is not None else "cuda")
            self.hann = torch.from_numpy(hann_window(self.win_length, self.n_fft).astype(np.float32)).to(self.device)

    def _chk(self, t, name, dtype):
        if not t.is_cuda:
            raise ValueError(f"PitchEnergy.{name}: expected a CUDA/HIP tensor (the HIP path has no CPU fallback), got {t.device}")
        if t.dtype != dtype:
            raise ValueError(f"PitchEnergy.{name}: expected dtype {dtype}, got {t.dtype}")

    def _lens(self, lens, B, name):
        import torch
        if tuple(lens.shape) != (B,):
            raise ValueError(f"PitchEnergy.{name} must have shape ({B},), got {tuple(lens.shape)}")
        if lens.dtype.is_floating_point or lens.dtype == torch.bool:
            raise ValueError(f"PitchEnergy.{name} must be integers, got {lens.dtype}")
        if not lens.is_cuda:                       # host lengths: the one place the unreflectable length can be refused
            half = max(self.frame_length, self.n_fft) // 2
            if lens.numel() and int(lens.min()) <= half:
                raise ValueError(f"PitchEnergy.{name}: an utterance of {int(lens.min())} samples cannot be reflected "
                                 f"(max(frame_length, n_fft)/2 + 1 = {half + 1} at the least)")
            lens = lens.to(self.device)
        return lens.to(torch.int64).contiguous()

    def __call__(self, wave, wave_lens):
        import torch
        from . import _lib
        from .ops import _p, _stream
        if wave.dim() != 2 or min(wave.shape) < 1:
            raise ValueError(f"PitchEnergy: wave must be (B, Nmax), got {tuple(wave.shape)}")
        self._chk(wave, "wave", torch.float32)
        B, Nmax = wave.shape
        lens = self._lens(wave_lens, B, "wave_lens")
        wave = wave.detach()
        if (Nmax > 1 and wave.stride(1) != 1) or (B > 1 and wave.stride(0) < Nmax):
            wave = wave.contiguous()
        ld = wave.stride(0) if B > 1 else Nmax
        Tmax = 1 + Nmax // self.hop
        f0, aper, energy = (torch.empty(B, Tmax, dtype=torch.float32, device=wave.device) for _ in range(3))
        voiced = torch.empty(B, Tmax, dtype=torch.uint8, device=wave.device)
        frames = torch.empty(B, dtype=torch.int64, device=wave.device)
        _lib.check(_lib.load().ttts_pitch_energy(_p(wave), ld, _p(lens), B, Nmax, self.n_fft, self.win_length, self.hop, self.frame_length,
                                                 self.window, self.tau_min, self.tau_max, float(self.sample_rate), self.threshold,
                                                 _p(self.hann), _p(f0), _p(voiced), _p(aper), _p(energy), _p(frames), _stream()),
                   "ttts_pitch_energy")
        return {"f0": f0, "voiced": voiced.view(torch.bool), "aperiodicity": aper, "energy": energy, "frames": frames}


def phoneme_average(values, durations, phoneme_lens, frames, mask=None):
    """frame values -> phoneme means (csrc/pitch.hip ttts_segment_mean, one launch, nothing read back).  values (B, Tmax) fp32,
    durations (B, Pmax) int64 as `extract_durations` returns them, phoneme_lens and frames (B,) integers, mask (B, Tmax) bool or
    uint8 or None -> {'mean': (B, Pmax) fp32, 'count': (B, Pmax) int32}.  Phoneme p covers frames [c_p, c_p + dur_p), c the
    exclusive prefix sum, clipped to frames[b]; the mean is over the frames the mask keeps, 0 when there is none.
    phoneme_average(f0, ..., mask=voiced) is FastSpeech 2's phoneme pitch, phoneme_average(energy, ...) its phoneme energy."""
    import torch
    from . import _lib
    from .ops import _p, _stream
    if values.dim() != 2 or min(values.shape) < 1:
        raise ValueError(f"phoneme_average: values must be (B, Tmax), got {tuple(values.shape)}")
    if not values.is_cuda:
        raise ValueError(f"phoneme_average.values: expected a CUDA/HIP tensor (the HIP path has no CPU fallback), got {values.device}")
    if values.dtype != torch.float32:
        raise ValueError(f"phoneme_average.values: expected dtype {torch.float32}, got {values.dtype}")
    B, Tmax = values.shape
    if durations.dim() != 2 or durations.size(0) != B or durations.size(1) < 1:
        raise ValueError(f"phoneme_average: durations must be ({B}, Pmax), got {tuple(durations.shape)}")
    if durations.dtype != torch.int64:
        raise ValueError(f"phoneme_average.durations: expected dtype {torch.int64}, got {durations.dtype}")
    Pmax = durations.size(1)
    for t, name in ((phoneme_lens, "phoneme_lens"), (frames, "frames")):
        if tuple(t.shape) != (B,):
            raise ValueError(f"phoneme_average.{name} must have shape ({B},), got {tuple(t.shape)}")
        if t.dtype.is_floating_point or t.dtype == torch.bool:
            raise ValueError(f"phoneme_average.{name} must be integers, got {t.dtype}")
    if mask is not None:
        if tuple(mask.shape) != (B, Tmax):
            raise ValueError(f"phoneme_average: mask must be ({B}, {Tmax}) like values, got {tuple(mask.shape)}")
        if mask.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"phoneme_average.mask: expected dtype {torch.bool} or {torch.uint8}, got {mask.dtype}")
        mask = mask.to(values.device).contiguous().view(torch.uint8)
    lens = [t.to(values.device).to(torch.int64).contiguous() for t in (phoneme_lens, frames)]
    values = values.detach()
    if (Tmax > 1 and values.stride(1) != 1) or (B > 1 and values.stride(0) < Tmax):
        values = values.contiguous()
    ld = values.stride(0) if B > 1 else Tmax
    dur = durations.to(values.device).contiguous()
    mean = torch.empty(B, Pmax, dtype=torch.float32, device=values.device)
    count = torch.empty(B, Pmax, dtype=torch.int32, device=values.device)
    _lib.check(_lib.load().ttts_segment_mean(_p(values), ld, _p(dur), _p(lens[0]), _p(lens[1]), _p(mask), Tmax, B, Tmax, Pmax, _p(mean),
                                             _p(count), _stream()), "ttts_segment_mean")
    return {"mean": mean, "count": count}
