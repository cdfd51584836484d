"""Griffin-Lim vocoder (ABI v24, csrc/vocoder.hip, transformertts_amd/audio.py): the entry points are declared, bound and exported,
ctypes and the header agree, every refusal comes with its message before any launch; the pseudo-inverse mel basis; the fp64
oracle the GPU tests use against itself (inverse of the forward oracle), against torch.istft in fp64 and in its descent; and
tools/vocode_mel.py's file handling.  Host logic only, no GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from audio_reference import CONFIG_A, CONFIG_B, magnitude_ref, make_signal, mel_filterbank_ref, ragged_batch, stft_ref, window_ref
from vocoder_reference import (envelope_zero_count, griffin_lim_ref, istft_ref, mel_to_magnitude_ref, pinv_ref, spectral_convergence,
                               unit_phases, vocodable)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ttts_vocoder_pinv_check", "ttts_mel_to_magnitude", "ttts_istft", "ttts_stft_project")
CONFIGS = (CONFIG_A, CONFIG_B)


def test_abi_version_and_the_header_declares_the_new_entry_points():
    from transformertts_amd import _lib, audio
    lib = _lib.load()
    assert lib.ttts_abi_version() >= 24
    hdr = open(os.path.join(REPO, "include", "ttts_hip.h")).read()
    declared = set(re.findall(r"\b(ttts_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, f"{name} is not declared in ttts_hip.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name), f"{name} is not exported / bound"
        decl = re.search(r"^(?:int|size_t) " + name + r"\s*\(([^;]*)\)\s*;", hdr, re.M).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name      # ctypes and the header agree on the argument count
    P, I, L, F, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_size_t
    assert _lib.SIGNATURES[NEW[0]] == (I, [P, Z, I, I])
    assert _lib.SIGNATURES[NEW[1]] == (I, [P, L, L, P, I, I, I, I, I, P, P, F, P, P, P])
    assert _lib.SIGNATURES[NEW[2]] == (I, [P, P, I, I, I, I, P, P, P, P])
    assert _lib.SIGNATURES[NEW[3]] == (I, [P, L, P, P, I, I, I, I, P, P, P, F, P, P, P])
    assert hdr.index("ABI v24; vocoder.hip") > hdr.index("int ttts_logmel_stats(")       # the block follows the v23 declarations
    block = hdr[hdr.index("ABI v24; vocoder.hip"):hdr.index("int ttts_vocoder_pinv_check")]
    for needle in ("x * (std + 1e-8) + mean", "expf(x[f])", "max(sum_f pinv[k, f] * m[f], floor)", "(frames_b - 1) * hop > n_fft/2",
                   "irfft(spec[b, t], n_fft)", "env > 1.17549435e-38f ? y / env : y", "g' = g + n_fft/2", "Nmax = (Tmax - 1) * hop",
                   "ascending", "(momentum / (1 + momentum)) * prev", "a2 > 1e-30f ? t * rsqrt(a2) : (1, 0)", "momentum in [0, 1)",
                   "{256, 512, 1024, 2048}", "Tmax < 2", "hop < 1 or", "floor <= 0", "misaligned pointers", "no atomics"):
        assert needle in block, needle
    src = open(os.path.join(REPO, "transformertts_amd", "csrc", "vocoder.hip")).read()
    assert "fft_lds<M, FFT_INVERSE, THREADS>" in src and '#include "audio_common.h"' in src
    assert "sincos" not in src and "atomic" not in src.replace("no atomics", "")
    assert '#include "audio_common.h"' in open(os.path.join(REPO, "transformertts_amd", "csrc", "audio.hip")).read()
    m = re.search(r"#define TTTS_VOCODER_SPAN_MULT (\d+)", src)
    assert int(m.group(1)) == audio.SPAN_MULT                         # the span constant the GPU tests size their joins by
    import transformertts_amd
    for name in ("Vocoder", "write_wav_pcm16"):
        assert getattr(transformertts_amd, name) is getattr(audio, name) and name in transformertts_amd.__all__


def test_entry_points_refuse_bad_arguments_with_a_message():
    from transformertts_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096 + 16)
    a = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)          # a 16-byte aligned host address (never dereferenced)
    a2, a4 = ctypes.c_void_p(a.value + 2), ctypes.c_void_p(a.value + 4)

    def bad(rc, needle):
        assert rc == -1, rc
        assert needle in _lib.last_error(), _lib.last_error()

    def caller(fn, names, defaults):
        def call(**kw):
            assert not set(kw) - set(names)
            return fn(*[kw.get(n, defaults[n]) for n in names])
        return call

    def common(call, e, tmax_kw):
        bad(call(B=0), e + ": sizes must be positive (B 0)")
        bad(call(B=-2), e + ": sizes must be positive (B -2)")
        for n in (0, 128, 1000, 4096):
            bad(call(n_fft=n), e + f": n_fft must be one of 256, 512, 1024, 2048, got {n}")
        bad(call(hop=0), e + ": hop must be in [1, n_fft] (hop 0, n_fft 1024)")
        bad(call(hop=1025), e + ": hop must be in [1, n_fft] (hop 1025, n_fft 1024)")
        bad(call(B=65536), e + ": grid too large (B 65536, at most 65535 utterances a call)")
        bad(call(**tmax_kw), e + ": Tmax must be at least 2, got 1")

    e = "mel_to_magnitude"
    names = ["mel", "ld_row", "ld_batch", "melspec_lens", "B", "Tmax", "n_fft", "hop", "n_mels", "pinv", "mean_std", "floor", "mag",
             "frames", "stream"]
    m2m = caller(lib.ttts_mel_to_magnitude, names, dict(mel=a, ld_row=80, ld_batch=1280, melspec_lens=a, B=4, Tmax=16, n_fft=1024,
                                                        hop=256, n_mels=80, pinv=a, mean_std=None, floor=1e-10, mag=a, frames=a,
                                                        stream=None))
    for p in ("mel", "melspec_lens", "pinv", "mag", "frames"):
        bad(m2m(**{p: None}), e + ": null pointer")
    common(m2m, e, dict(Tmax=1))
    bad(m2m(Tmax=0), e + ": Tmax must be at least 2, got 0")
    bad(m2m(Tmax=(1 << 22) + 2), e + ": more than 2^30 samples per utterance are not supported")
    bad(m2m(n_mels=0), e + ": sizes must be positive (n_mels 0)")
    bad(m2m(n_mels=513, ld_row=513, ld_batch=513 * 16), e + ": at most 512 filters (n_mels 513)")
    bad(m2m(ld_row=79), e + ": the strides must cover a row and a batch (ld_row 79, ld_batch 1280, n_mels 80, Tmax 16)")
    bad(m2m(ld_batch=1279), e + ": the strides must cover a row and a batch (ld_row 80, ld_batch 1279,")
    bad(m2m(floor=0.0), e + ": floor must be positive")
    bad(m2m(floor=-1e-10), e + ": floor must be positive")
    for p in ("mel", "pinv", "mag", "mean_std"):
        bad(m2m(**{p: a2}), e + ": mel, pinv, mean_std and mag must be 4-byte aligned")
    for p in ("melspec_lens", "frames"):
        bad(m2m(**{p: a4}), e + ": melspec_lens and frames must be 8-byte aligned")

    e = "istft"
    names = ["spec", "frames", "B", "Tmax", "n_fft", "hop", "tables", "wave", "wave_lens", "stream"]
    ist = caller(lib.ttts_istft, names, dict(spec=a, frames=a, B=4, Tmax=16, n_fft=1024, hop=256, tables=a, wave=a, wave_lens=a,
                                             stream=None))
    for p in ("spec", "frames", "tables", "wave", "wave_lens"):
        bad(ist(**{p: None}), e + ": null pointer")
    common(ist, e, dict(Tmax=1))
    bad(ist(Tmax=(1 << 22) + 2), e + ": more than 2^30 samples per utterance are not supported")
    bad(ist(spec=a4), e + ": spec must be 8-byte aligned (complex pairs)")
    for p in ("tables", "wave"):
        bad(ist(**{p: a2}), e + ": tables and wave must be 4-byte aligned")
    for p in ("frames", "wave_lens"):
        bad(ist(**{p: a4}), e + ": frames and wave_lens must be 8-byte aligned")

    e = "stft_project"
    names = ["wave", "ld_batch", "wave_lens", "frames", "B", "Nmax", "n_fft", "hop", "tables", "mag", "prev", "momentum", "spec",
             "frames_out", "stream"]
    prj = caller(lib.ttts_stft_project, names, dict(wave=a, ld_batch=3840, wave_lens=None, frames=a, B=4, Nmax=3840, n_fft=1024, hop=256,
                                                    tables=a, mag=a, prev=a, momentum=0.99, spec=a, frames_out=None, stream=None))
    for p in ("wave", "tables", "spec"):
        bad(prj(**{p: None}), e + ": null pointer")
    bad(prj(frames=None), e + ": give wave_lens or frames, one of them")
    bad(prj(wave_lens=a), e + ": give wave_lens or frames, one of them")
    common(prj, e, dict(Nmax=255, ld_batch=255))
    bad(prj(Nmax=0, ld_batch=0), e + ": sizes must be positive (Nmax 0)")
    bad(prj(Nmax=(1 << 30) + 1, ld_batch=1 << 31), e + ": more than 2^30 samples per utterance are not supported (Nmax 1073741825)")
    bad(prj(ld_batch=3839), e + ": the batch stride must be >= Nmax (ld_batch 3839, Nmax 3840)")
    bad(prj(momentum=1.0), e + ": momentum must be in [0, 1), got 1")
    bad(prj(momentum=-0.5), e + ": momentum must be in [0, 1), got -0.5")
    bad(prj(momentum=float("nan")), e + ": momentum must be in [0, 1)")
    bad(prj(prev=None), e + ": momentum 0.99 needs prev")
    bad(prj(mag=None), e + ": prev and momentum need mag (the projection)")
    bad(prj(mag=None, prev=None), e + ": prev and momentum need mag (the projection)")
    for p in ("spec", "prev"):
        bad(prj(**{p: a4}), e + ": spec and prev must be 8-byte aligned (complex pairs)")
    for p in ("wave", "tables", "mag"):
        bad(prj(**{p: a2}), e + ": wave, tables and mag must be 4-byte aligned")
    for p in ("frames", "frames_out"):
        bad(prj(**{p: a4}), e + ": wave_lens, frames and frames_out must be 8-byte aligned")
    bad(prj(wave_lens=a4, frames=None), e + ": wave_lens, frames and frames_out must be 8-byte aligned")

    # the pseudo-inverse: a host copy is checked before it is uploaded
    e = "vocoder_pinv_check"
    pinv = np.zeros((257, 40), dtype=np.float32)
    chk = lambda p=pinv, nbytes=None, n_fft=512, n_mels=40: lib.ttts_vocoder_pinv_check(p.ctypes.data, p.nbytes if nbytes is None else nbytes,
                                                                                        n_fft, n_mels)
    assert chk() == 0
    assert lib.ttts_vocoder_pinv_check(None, 4, 512, 40) == -1 and e + ": null pointer" in _lib.last_error()
    bad(chk(n_fft=500), e + ": n_fft must be one of 256, 512, 1024, 2048, got 500")
    bad(chk(n_mels=0), e + ": sizes must be positive (n_mels 0)")
    bad(chk(n_mels=513), e + ": at most 512 filters (n_mels 513)")
    bad(chk(nbytes=pinv.nbytes - 4), e + f": the matrix holds {pinv.nbytes - 4} bytes, {pinv.nbytes} expected")
    bad(chk(n_fft=1024), e + f": the matrix holds {pinv.nbytes} bytes, {513 * 40 * 4} expected")
    bad(lib.ttts_vocoder_pinv_check(ctypes.c_void_p(pinv.ctypes.data + 2), pinv.nbytes, 512, 40), e + ": the matrix must be 4-byte aligned")
    p = pinv.copy()
    p[3, 7] = np.inf
    bad(chk(p=p), e + ": element (3, 7) is not finite")
    p[3, 7], p[256, 39] = 0.0, np.nan
    bad(chk(p=p), e + ": element (256, 39) is not finite")


def test_the_inverse_mel_basis_is_the_pseudo_inverse_rounded_once():
    from transformertts_amd.audio import inverse_mel_basis, mel_filterbank
    for cfg in CONFIGS:
        fb = mel_filterbank(cfg["sample_rate"], cfg["n_fft"], cfg["n_mels"], cfg["fmin"], cfg["fmax"])
        pinv = inverse_mel_basis(fb)
        assert pinv.dtype == np.float32 and pinv.shape == (cfg["n_fft"] // 2 + 1, cfg["n_mels"]) and pinv.flags["C_CONTIGUOUS"]
        assert np.array_equal(pinv, np.linalg.pinv(fb).astype(np.float32))           # fp64, rounded once
        back = fb @ pinv.astype(np.float64) @ fb
        assert np.abs(back - fb).max() <= 1e-6 * np.abs(fb).max(), np.abs(back - fb).max()
        assert np.abs(fb @ np.linalg.pinv(fb) @ fb - fb).max() <= 1e-12 * np.abs(fb).max()
        ref = pinv_ref(cfg)                                                          # the oracle's own, from its own basis
        assert np.abs(ref - pinv).max() <= 1e-6 * np.abs(ref).max()
    with pytest.raises(ValueError, match="must be \\(n_mels, bins\\)"):
        inverse_mel_basis(np.ones(5))


ROUND_TRIPS = [(CONFIG_A, 256), (CONFIG_B, 128), (CONFIG_B, 256), (CONFIG_B, 200), (CONFIG_B, 96)]


def test_the_oracle_inverts_the_forward_oracle():
    worst = 0.0
    for cfg, hop in ROUND_TRIPS:
        n_fft, win = cfg["n_fft"], cfg["win_length"]
        for i, n in enumerate((n_fft // 2 + 1 + hop, 5 * hop, 8 * hop - 1, 4000)):
            x = make_signal(n, cfg["sample_rate"], 60 + i).astype(np.float64)
            spec = stft_ref(x, n_fft, hop, win)
            T = spec.shape[0]
            back = istft_ref(spec, n_fft, hop, win)
            assert back.shape == ((T - 1) * hop,)
            err = float(np.abs(back - x[:(T - 1) * hop]).max())
            worst = max(worst, err)
            assert err <= 1e-12, (n_fft, hop, n, err)
    print(f"vocoder oracle: istft_ref(stft_ref(x)) - x max-abs {worst:.2e}")


def test_the_oracle_istft_is_torch_istft_in_fp64():
    rng = np.random.default_rng(11)
    for cfg, hop in ROUND_TRIPS:
        n_fft, win = cfg["n_fft"], cfg["win_length"]
        T = 12
        spec = rng.standard_normal((T, n_fft // 2 + 1)) + 1j * rng.standard_normal((T, n_fft // 2 + 1))     # not a consistent STFT
        try:
            want = torch.istft(torch.from_numpy(spec.T.copy()), n_fft, hop_length=hop, win_length=win, center=True, length=(T - 1) * hop,
                               window=torch.hann_window(win, periodic=True, dtype=torch.float64)).numpy()
        except RuntimeError as e:                                                    # torch refuses windows whose overlap-add has zeros
            assert "window overlap add" in str(e), e
            continue
        got = istft_ref(spec, n_fft, hop, win)
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (n_fft, hop, np.abs(got - want).max())
    # a window that leaves gaps: 520 samples no window reaches, and those come out as exact zeros
    assert envelope_zero_count(9, 256, 128, 64) == 520
    spec = rng.standard_normal((9, 129)) + 1j * rng.standard_normal((9, 129))
    out = istft_ref(spec, 256, 128, 64)
    assert int((out == 0).sum()) == 520 and np.isfinite(out).all()


def test_plain_griffin_lim_descends_in_the_oracle():
    for ci, cfg in enumerate(CONFIGS):
        n_fft, hop, win = cfg["n_fft"], cfg["hop_length"], cfg["win_length"]
        _, lens, sigs = ragged_batch(cfg)
        for b, x in enumerate(sigs):
            mag = magnitude_ref(x, cfg)
            if not vocodable(mag.shape[0], cfg):
                assert b == 0                                                        # the n_fft/2 + 1 sample utterance: 3 frames
                continue
            trace = []
            wave = griffin_lim_ref(mag, unit_phases(mag.shape, 100 * ci + b), n_fft, hop, win, 32, 0.0, trace)
            assert wave.shape == ((mag.shape[0] - 1) * hop,) and len(trace) == 33
            assert all(trace[i + 1] <= trace[i] * (1 + 1e-12) for i in range(32)), trace
            assert trace[-1] < trace[0]
            assert abs(spectral_convergence(wave, mag, n_fft, hop, win) - trace[-1]) == 0.0


def test_mel_to_magnitude_oracle_undoes_the_mel_projection_before_the_floor():
    for cfg in CONFIGS:
        fb = mel_filterbank_ref(cfg["sample_rate"], cfg["n_fft"], cfg["n_mels"], cfg["fmin"], cfg["fmax"])
        pinv = pinv_ref(cfg)
        x = make_signal(4000, cfg["sample_rate"], 9)
        mel = np.log(np.maximum(magnitude_ref(x, cfg) @ fb.T, 1e-5))
        mag = mel_to_magnitude_ref(mel, pinv)
        assert mag.shape == (1 + 4000 // cfg["hop_length"], cfg["n_fft"] // 2 + 1) and (mag >= 1e-10).all()
        again = mel_to_magnitude_ref((mel - 1.5) / (2.0 + 1e-8), pinv, mean=1.5, std=2.0)
        assert np.abs(again - mag).max() <= 1e-9 * mag.max()
        # before the floor the pseudo-inverse gives back a spectrum with the mel spectrum that went in (the basis has full row
        # rank), and the floor is element-wise
        raw = np.exp(mel) @ pinv.T
        assert np.abs(raw @ fb.T - np.exp(mel)).max() <= 1e-5 * np.exp(mel).max()
        assert np.array_equal(mag, np.maximum(raw, 1e-10)) and (raw < 1e-10).any()


def test_vocode_mel_reads_what_preprocess_mel_writes(tmp_path):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import vocode_mel as tool
    finally:
        sys.path.pop(0)
    from transformertts_amd.audio import read_wav

    class OracleVocoder:
        """Vocoder's surface on the fp64 oracle, on the CPU"""

        def __init__(self, cfg, mean=None, std=None):
            self.cfg, self.mean, self.std, self.device, self.sample_rate = cfg, mean, std, torch.device("cpu"), cfg["sample_rate"]

        def __call__(self, mel, lens):
            c = self.cfg
            T = int(lens[0])
            mag = mel_to_magnitude_ref(mel[0, :T].numpy(), pinv_ref(c), mean=self.mean, std=self.std)
            wave = griffin_lim_ref(mag, unit_phases(mag.shape, 0), c["n_fft"], c["hop_length"], c["win_length"], 2, 0.99)
            return {"wave": torch.from_numpy(wave).float()[None], "wave_lens": torch.tensor([wave.size])}

    made = []

    def make(cfg, mean=None, std=None):
        made.append((mean, std))
        return OracleVocoder(cfg, mean, std)

    cfg = dict(CONFIG_B, normalize_mel=True)
    fb = mel_filterbank_ref(16000, 512, 40, 50.0, 8000.0)
    x = make_signal(2000, 16000, 5)
    mel = np.log(np.maximum(magnitude_ref(x, CONFIG_B) @ fb.T, 1e-5))
    npz, stats, out = tmp_path / "a.npz", tmp_path / "stats.json", tmp_path / "a.wav"
    np.savez(str(npz), melspec=np.ascontiguousarray(((mel + 5.0) / (2.0 + 1e-8)).T.astype(np.float32)))      # (n_mels, T) as the tool writes
    stats.write_text('{"mean": -5.0, "std": 2.0}')
    n = tool.run({"audio": cfg}, str(npz), str(out), stats_path=str(stats), make_vocoder=make, log=lambda s: None)
    assert made == [(-5.0, 2.0)]
    y = read_wav(str(out), 16000)
    assert n == y.size == (mel.shape[0] - 1) * 128 and np.abs(y).max() > 0.01
    with pytest.raises(ValueError, match="normalize_mel"):
        tool.run({"audio": cfg}, str(npz), str(out), stats_path=None, make_vocoder=make, log=lambda s: None)
    np.savez(str(tmp_path / "b.npz"), melspec=np.zeros((41, 9), np.float32))
    with pytest.raises(ValueError, match="melspec must be \\(40, T\\)"):
        tool.run({"audio": cfg}, str(tmp_path / "b.npz"), str(out), stats_path=str(stats), make_vocoder=make, log=lambda s: None)
