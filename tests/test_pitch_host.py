"""Frame pitch and energy (csrc/pitch.hip, transformertts_amd/audio.py): what the fp64 oracle of tests/pitch_reference.py
delivers on pure sines, the identity the kernel takes the energy from against the rfft, d' of silent and constant frames, the
oracle's frame count against the front end's, every refusal of the two entry points and of the Python checks with its message,
before any launch; tools/preprocess_mel.py with `prosody=True` on oracles; and the exports.  Host logic only, no GPU."""
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

from audio_reference import CLIP, CONFIG_A, frames_ref, logmel_ref, make_signal, mel_filterbank_ref, stft_ref
from pitch_reference import (LONG_LAGS, ODD_WINDOW, SHIPPED, SHORT_FRAME, SMALL, block_ref, cents, energy_frames_ref, energy_identity, energy_ref,
                             frame_count_ref, glide_signal, lags_ref, pitch_frames_ref, pitch_ref, pitch_stock, segment_mean_ref)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ttts_pitch_lags", "ttts_pitch_frames", "ttts_pitch_block", "ttts_pitch_energy", "ttts_segment_mean")


def test_the_header_declares_each_entry_point_once_and_the_exports_agree():
    from transformertts_amd import _lib, audio
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
    for name in ("PitchEnergy", "phoneme_average"):
        assert getattr(transformertts_amd, name) is getattr(audio, name) and name in transformertts_amd.__all__
    assert 1 <= lib.ttts_pitch_lags() <= 8
    # a workgroup owns 8 frames at the shipped shape and fewer when the lags no longer fit its LDS; 0 for a shape the entry refuses
    assert lib.ttts_pitch_frames(1024, 256, 1024, 512, 340) == 8 and lib.ttts_pitch_frames(256, 64, 256, 128, 100) == 8
    assert 1 <= lib.ttts_pitch_frames(2048, 1, 4096, 1, 4095) < 8 and lib.ttts_pitch_frames(1024, 256, 1024, 512, 513) == 0
    for p, frames in ((SMALL, 8), (SHIPPED, 8), (ODD_WINDOW, 8), (SHORT_FRAME, 8), (LONG_LAGS, 2)):      # the stock form's block order is the kernel's
        a = (p["n_fft"], p["hop_length"], p["frame_length"], p["window"], lags_ref(p)[1])
        assert (lib.ttts_pitch_frames(*a), lib.ttts_pitch_block(*a)) == (frames, block_ref(p)), p
    assert lib.ttts_pitch_block(1024, 256, 1024, 512, 513) == 0
    src = open(os.path.join(REPO, "transformertts_amd", "csrc", "pitch.hip")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert "atomic" not in code.replace("__ATOMIC_", "") and "hipMalloc" not in code and "hipMemcpy" not in code
    assert re.search(r"PITCH_MAX_F = (\d+)", src).group(1) == str(audio.PITCH_MAX_FRAME)


@pytest.mark.parametrize("freq,bound", [(70, 0.013), (110, 0.010), (220, 0.084), (440, 0.37), (590, 0.42)])
def test_the_oracle_on_pure_sines(freq, bound):
    x = np.sin(2 * np.pi * freq * np.arange(6000) / 22050.0)
    r = pitch_ref(x, SHIPPED)
    mid = slice(3, r["frames"] - 3)                                   # (the end frames are half reflection)
    err = float(cents(r["f0"][mid], freq).max())
    print(f"YIN oracle on a {freq} Hz sine at 22050 Hz: {err:.4f} cent")
    assert r["voiced"][mid].all() and err <= 0.5
    assert err <= 1.05 * bound                                        # the figures of DESIGN.md 25


@pytest.mark.parametrize("p", [SMALL, SHIPPED, SHORT_FRAME, ODD_WINDOW], ids=["small", "shipped", "short_frame", "odd_window"])
def test_the_energy_identity_is_parsevals(p):
    x = glide_signal(3000, p, 3)
    y = energy_frames_ref(x, p)
    want = energy_ref(x, p)
    assert np.abs(energy_identity(y) / want - 1.0).max() <= 1e-13
    cfg = dict(n_fft=p["n_fft"], hop_length=p["hop_length"], win_length=p["win_length"])
    if p["frame_length"] <= p["n_fft"]:                               # ... and the rows are the front end's STFT rows
        spec = stft_ref(x, cfg["n_fft"], cfg["hop_length"], cfg["win_length"])
        assert np.abs(np.sqrt((np.abs(spec) ** 2).sum(axis=1)) / want - 1.0).max() <= 1e-13


def test_silent_and_constant_frames():
    for x in (np.zeros(2000), np.full(2000, 0.37)):
        for fn in (pitch_ref, pitch_stock):
            r = fn(x, SMALL)
            assert r["frames"] == 32 and (r["dprime"] == 1).all()
            assert not r["voiced"].any() and (r["f0"] == 0).all() and (r["aperiodicity"] == 1).all()
            assert np.allclose(r["margin"], 0.9) and (r["lag"] == lags_ref(SMALL)[0]).all()       # the first argmin of a flat d'


def test_the_oracle_frames_like_the_front_end():
    for p in (SMALL, SHIPPED, ODD_WINDOW):
        for n in (p["n_fft"] // 2 + 1, 5 * p["hop_length"], 8 * p["hop_length"] - 1, 3000):
            x = make_signal(n, p["sample_rate"], n)
            want = frames_ref(x, p["n_fft"], p["hop_length"])
            got = pitch_frames_ref(x, p)
            assert frame_count_ref(n, p) == want.shape[0] == got.shape[0] == pitch_ref(x, p)["frames"]
            assert np.array_equal(got, want)                          # F == n_fft: the very frames
        assert frame_count_ref(p["n_fft"] // 2, p) == 0 and pitch_ref(np.ones(p["n_fft"] // 2), p)["frames"] == 0
    p = SHORT_FRAME                                                   # F < n_fft: the middle F samples of the front end's frames
    x = make_signal(3000, 8000, 1)
    lo = (p["n_fft"] - p["frame_length"]) // 2
    assert np.array_equal(pitch_frames_ref(x, p), frames_ref(x, p["n_fft"], p["hop_length"])[:, lo:lo + p["frame_length"]])
    assert frame_count_ref(256, p) == 0 and frame_count_ref(257, p) == 5
    assert (lags_ref(SHIPPED), lags_ref(SMALL)) == ((36, 340), (16, 100))
    assert (block_ref(SHIPPED), block_ref(SMALL), block_ref(ODD_WINDOW)) == (256, 64, 100)


def test_the_stock_form_follows_the_oracle():
    x = glide_signal(4000, SMALL, 10)
    r, s = pitch_ref(x, SMALL), pitch_stock(x, SMALL)
    err = float(np.abs(s["dprime"] - r["dprime"]).max())
    ok = r["margin"] > 8 * err
    print(f"stock fp32 |d'| error {err:.2e}; {int((~ok).sum())} of {ok.size} frames undecided")
    assert err <= 1e-5 and (~ok).sum() <= 0.05 * ok.size
    assert (s["voiced"][ok] == r["voiced"][ok]).all() and (s["lag"][ok & r["voiced"]] == r["lag"][ok & r["voiced"]]).all()
    assert np.abs(s["energy"] / energy_ref(x, SMALL) - 1.0).max() <= 1e-5


# ------------------------------------------------------------------------------------------------ refusals of the C entries
PITCH_POINTERS = ("wave", "wave_lens", "hann", "f0", "voiced", "aperiodicity", "energy", "frames")


def _pitch(lib, **kw):
    """ttts_pitch_energy on a host buffer: every case below is refused before a launch, so nothing dereferences it.  A pointer
    argument is None or a byte offset into the buffer."""
    buf = np.zeros(64, dtype=np.int64)
    a = dict(wave=0, ld_batch=4000, wave_lens=0, B=2, Nmax=4000, n_fft=1024, win_length=1024, hop=256, frame_length=1024, window=512,
             tau_min=36, tau_max=340, sample_rate=22050.0, threshold=0.1, hann=0, f0=0, voiced=0, aperiodicity=0, energy=0, frames=0)
    a.update(kw)
    for name in PITCH_POINTERS:
        a[name] = None if a[name] is None else buf.ctypes.data + a[name]
    return lib.ttts_pitch_energy(a["wave"], a["ld_batch"], a["wave_lens"], a["B"], a["Nmax"], a["n_fft"], a["win_length"], a["hop"],
                                 a["frame_length"], a["window"], a["tau_min"], a["tau_max"], a["sample_rate"], a["threshold"], a["hann"],
                                 a["f0"], a["voiced"], a["aperiodicity"], a["energy"], a["frames"], None)


PITCH_REFUSALS = [(dict([(name, None)]), "null pointer") for name in PITCH_POINTERS] + [
    (dict(B=0), "B must be in [1, 65535] (one grid row per utterance), got 0"), (dict(B=65536), "got 65536"),
    (dict(Nmax=0), "Nmax must be in [1, 2^30] samples per utterance, got 0"),
    (dict(Nmax=(1 << 30) + 1, ld_batch=1 << 31), f"got {(1 << 30) + 1}"),
    (dict(n_fft=1000), "n_fft must be one of 256, 512, 1024, 2048, got 1000"), (dict(n_fft=4096, frame_length=4096), "got 4096"),
    (dict(win_length=0), "win_length must be in [1, n_fft] (win_length 0, n_fft 1024)"),
    (dict(win_length=1025), "win_length must be in [1, n_fft] (win_length 1025, n_fft 1024)"),
    (dict(frame_length=1023), "frame_length must be even and in [2, 4096], got 1023"),
    (dict(frame_length=4098), "frame_length must be even and in [2, 4096], got 4098"),
    (dict(frame_length=0), "frame_length must be even and in [2, 4096], got 0"),
    (dict(hop=0), "hop must be in [1, frame_length] (hop 0, frame_length 1024)"),
    (dict(hop=1025), "hop must be in [1, frame_length] (hop 1025, frame_length 1024)"),
    (dict(window=0), "window must be positive, got 0"),
    (dict(tau_min=1), "tau_min must be at least 2 (fmax too high for the sample rate), got 1"),
    (dict(tau_min=340), "tau_min must be below tau_max (tau_min 340, tau_max 340)"),
    (dict(tau_max=30), "tau_min must be below tau_max (tau_min 36, tau_max 30)"),
    (dict(tau_max=513), "window + tau_max must fit the frame (window 512, tau_max 513, frame_length 1024)"),
    (dict(window=700), "window + tau_max must fit the frame (window 700, tau_max 340, frame_length 1024)"),
    (dict(threshold=0.0), "threshold must be in (0, 1), got 0"), (dict(threshold=1.0), "threshold must be in (0, 1), got 1"),
    (dict(threshold=float("nan")), "threshold must be in (0, 1), got nan"),
    (dict(sample_rate=0.0), "sample_rate must be positive and finite, got 0"),
    (dict(sample_rate=float("inf")), "sample_rate must be positive and finite, got inf"),
    (dict(ld_batch=3999), "the batch stride must be >= Nmax (ld_batch 3999, Nmax 4000)"),
    (dict(wave=2), "wave, hann, f0, aperiodicity and energy must be 4-byte aligned"),
    (dict(hann=2), "wave, hann, f0, aperiodicity and energy must be 4-byte aligned"),
    (dict(f0=6), "4-byte aligned"), (dict(aperiodicity=1), "4-byte aligned"), (dict(energy=3), "4-byte aligned"),
    (dict(wave_lens=4), "wave_lens and frames must be 8-byte aligned"), (dict(frames=12), "wave_lens and frames must be 8-byte aligned"),
]

MEAN_POINTERS = ("values", "durations", "phoneme_lens", "frames", "mask", "mean", "counts")


def _mean(lib, **kw):
    buf = np.zeros(64, dtype=np.int64)
    a = dict(values=0, ld_values=40, durations=0, phoneme_lens=0, frames=0, mask=0, ld_mask=40, B=3, Tmax=40, Pmax=12, mean=0, counts=0)
    a.update(kw)
    for name in MEAN_POINTERS:
        a[name] = None if a[name] is None else buf.ctypes.data + a[name]
    return lib.ttts_segment_mean(a["values"], a["ld_values"], a["durations"], a["phoneme_lens"], a["frames"], a["mask"], a["ld_mask"],
                                 a["B"], a["Tmax"], a["Pmax"], a["mean"], a["counts"], None)


MEAN_REFUSALS = [(dict([(name, None)]), "null pointer") for name in MEAN_POINTERS if name != "mask"] + [
    (dict(B=0), "B must be in [1, 65535] (one workgroup per utterance), got 0"), (dict(B=65536), "got 65536"),
    (dict(Tmax=0, ld_values=0, ld_mask=0), "Tmax must be in [1, 2^30] frames, got 0"),
    (dict(Pmax=0), "Pmax must be in [1, 2^20] phonemes, got 0"), (dict(Pmax=(1 << 20) + 1), f"got {(1 << 20) + 1}"),
    (dict(ld_values=39), "the value stride must be >= Tmax (ld_values 39, Tmax 40)"),
    (dict(ld_mask=39), "the mask stride must be >= Tmax (ld_mask 39, Tmax 40)"),
    (dict(values=2), "values, mean and counts must be 4-byte aligned"), (dict(mean=6), "values, mean and counts must be 4-byte aligned"),
    (dict(counts=1), "values, mean and counts must be 4-byte aligned"),
    (dict(durations=4), "durations, phoneme_lens and frames must be 8-byte aligned"),
    (dict(phoneme_lens=12), "durations, phoneme_lens and frames must be 8-byte aligned"),
    (dict(frames=4), "durations, phoneme_lens and frames must be 8-byte aligned"),
]


@pytest.mark.parametrize("case", range(len(PITCH_REFUSALS)))
def test_every_refusal_of_pitch_energy_names_its_value_before_any_launch(case):
    from transformertts_amd import _lib
    lib = _lib.load()
    kw, needle = PITCH_REFUSALS[case]
    rc = _pitch(lib, **kw)
    assert rc != 0 and needle in _lib.last_error(), _lib.last_error()
    with pytest.raises(RuntimeError, match=re.escape(needle)):       # ... and reaches Python through _lib.check
        _lib.check(rc, "ttts_pitch_energy")


@pytest.mark.parametrize("case", range(len(MEAN_REFUSALS)))
def test_every_refusal_of_segment_mean_names_its_value_before_any_launch(case):
    from transformertts_amd import _lib
    lib = _lib.load()
    kw, needle = MEAN_REFUSALS[case]
    rc = _mean(lib, **kw)
    assert rc != 0 and needle in _lib.last_error(), _lib.last_error()
    with pytest.raises(RuntimeError, match=re.escape(needle)):
        _lib.check(rc, "ttts_segment_mean")


# ------------------------------------------------------------------------------------------------ refusals of the Python checks
def _fake_front_end(cfg):
    """what PitchEnergy reads of a MelFrontEnd, on the CPU: the checks in front of the launch can be reached without a device"""
    return types.SimpleNamespace(n_fft=cfg["n_fft"], win_length=cfg["win_length"], hop=cfg["hop_length"], sample_rate=cfg["sample_rate"],
                                 device=torch.device("cpu"), tables=torch.zeros(8 + cfg["n_fft"], dtype=torch.int32))


def test_the_constructor_refuses():
    from transformertts_amd.audio import PitchEnergy
    fe = _fake_front_end(CONFIG_A)
    pe = PitchEnergy(CONFIG_A, front_end=fe)
    assert (pe.frame_length, pe.window, pe.tau_min, pe.tau_max, pe.threshold) == (1024, 512, 36, 340, 0.1)
    assert (pe.fmin, pe.fmax, pe.hop, pe.n_fft, pe.win_length, pe.sample_rate) == (65.0, 600.0, 256, 1024, 1024, 22050)
    assert pe.hann.dtype == torch.float32 and pe.hann.data_ptr() == fe.tables.data_ptr() + 32 and pe.hann.numel() == 1024
    for kw, needle in (
            (dict(frame_length=1023), "frame_length must be even and in [2, 4096], got 1023"),
            (dict(frame_length=4098), "frame_length must be even and in [2, 4096], got 4098"),
            (dict(frame_length=200, window=10, fmin=200.0), "hop_length must be in [1, frame_length] (hop_length 256, frame_length 200)"),
            (dict(window=0), "window must be positive, got 0"),
            (dict(fmax=12000.0), "tau_min = floor(sample_rate / fmax) must be at least 2, got 1"),
            (dict(fmin=600.0, fmax=600.0), "need 0 < fmin < fmax (fmin 600.0, fmax 600.0)"),
            (dict(fmin=0.0), "need 0 < fmin < fmax (fmin 0.0, fmax 600.0)"),
            (dict(fmin=40.0), "window + tau_max must fit the frame (window 512, tau_max = ceil(sample_rate / fmin) = 552, frame_length 1024)"),
            (dict(window=700), "window + tau_max must fit the frame (window 700"),
            (dict(threshold=0.0), "threshold must be in (0, 1), got 0.0"), (dict(threshold=1.0), "threshold must be in (0, 1), got 1.0")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            PitchEnergy(CONFIG_A, front_end=fe, **kw)
    with pytest.raises(ValueError, match=re.escape("n_fft must be one of (256, 512, 1024, 2048), got 1000")):
        PitchEnergy(dict(CONFIG_A, n_fft=1000), front_end=fe)
    with pytest.raises(ValueError, match=re.escape("win_length must be in [1, n_fft] (win_length 2000, n_fft 1024)")):
        PitchEnergy(dict(CONFIG_A, win_length=2000), front_end=fe)
    with pytest.raises(ValueError, match="front_end was built for another audio config"):
        PitchEnergy(dict(CONFIG_A, hop_length=128), front_end=fe)
    with pytest.raises(ValueError, match="front_end lives on cpu, device is cuda"):
        PitchEnergy(CONFIG_A, front_end=fe, device="cuda")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match=re.escape("PitchEnergy needs the HIP device (no CPU fallback)")):
            PitchEnergy(CONFIG_A)


def test_the_call_checks_like_the_front_end_in_the_same_order():
    from transformertts_amd.audio import PitchEnergy
    pe = PitchEnergy(CONFIG_A, front_end=_fake_front_end(CONFIG_A))
    lens = torch.tensor([3000, 2000])
    for wave, wl, needle in (
            (torch.zeros(3000), lens, "PitchEnergy: wave must be (B, Nmax), got (3000,)"),
            (torch.zeros(2, 0), lens, "PitchEnergy: wave must be (B, Nmax), got (2, 0)"),
            (torch.zeros(2, 3000), lens, "PitchEnergy.wave: expected a CUDA/HIP tensor (the HIP path has no CPU fallback), got cpu"),
            (torch.zeros(2, 3000, dtype=torch.float64), torch.zeros(3), "PitchEnergy.wave: expected a CUDA/HIP tensor")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            pe(wave, wl)
    for wl, needle in ((torch.tensor([3000]), "PitchEnergy.wave_lens must have shape (2,), got (1,)"),
                       (torch.tensor([3000.0, 2.0]), "PitchEnergy.wave_lens must be integers, got torch.float32"),
                       (torch.tensor([True, False]), "PitchEnergy.wave_lens must be integers, got torch.bool"),
                       (torch.tensor([3000, 512]), "an utterance of 512 samples cannot be reflected (max(frame_length, n_fft)/2 + 1 = 513")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            pe._lens(wl, 2, "wave_lens")
    with pytest.raises(ValueError, match=re.escape("PitchEnergy.wave: expected dtype torch.float32, got torch.float64")):
        pe._chk(types.SimpleNamespace(is_cuda=True, dtype=torch.float64, device="cuda:0"), "wave", torch.float32)


def test_phoneme_average_refuses():
    from transformertts_amd.audio import phoneme_average
    v, d, pl, fr = torch.zeros(3, 40), torch.zeros(3, 12, dtype=torch.int64), torch.tensor([12, 3, 1]), torch.tensor([40, 20, 5])
    cuda = types.SimpleNamespace(dim=lambda: 2, shape=(3, 40), is_cuda=True, dtype=torch.float32, device="cuda:0")
    for args, kw, needle in (
            ((torch.zeros(40), d, pl, fr), {}, "phoneme_average: values must be (B, Tmax), got (40,)"),
            ((torch.zeros(0, 40), d, pl, fr), {}, "phoneme_average: values must be (B, Tmax), got (0, 40)"),
            ((v, d, pl, fr), {}, "phoneme_average.values: expected a CUDA/HIP tensor (the HIP path has no CPU fallback), got cpu"),
            ((types.SimpleNamespace(**dict(vars(cuda), dtype=torch.float64)), d, pl, fr), {},
             "phoneme_average.values: expected dtype torch.float32, got torch.float64"),
            ((cuda, torch.zeros(2, 12, dtype=torch.int64), pl, fr), {}, "phoneme_average: durations must be (3, Pmax), got (2, 12)"),
            ((cuda, torch.zeros(3, dtype=torch.int64), pl, fr), {}, "phoneme_average: durations must be (3, Pmax), got (3,)"),
            ((cuda, torch.zeros(3, 0, dtype=torch.int64), pl, fr), {}, "phoneme_average: durations must be (3, Pmax), got (3, 0)"),
            ((cuda, d.to(torch.int32), pl, fr), {}, "phoneme_average.durations: expected dtype torch.int64, got torch.int32"),
            ((cuda, d, pl[:2], fr), {}, "phoneme_average.phoneme_lens must have shape (3,), got (2,)"),
            ((cuda, d, pl.float(), fr), {}, "phoneme_average.phoneme_lens must be integers, got torch.float32"),
            ((cuda, d, pl, fr[:1]), {}, "phoneme_average.frames must have shape (3,), got (1,)"),
            ((cuda, d, pl, fr > 3), {}, "phoneme_average.frames must be integers, got torch.bool"),
            ((cuda, d, pl, fr), dict(mask=torch.zeros(3, 39, dtype=torch.bool)), "phoneme_average: mask must be (3, 40) like values, got (3, 39)"),
            ((cuda, d, pl, fr), dict(mask=torch.zeros(3, 40)), "phoneme_average.mask: expected dtype torch.bool or torch.uint8, got torch.float32")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            phoneme_average(*args, **kw)


def test_the_segment_mean_reference():
    v = np.arange(20, dtype=np.float32).reshape(2, 10)
    d = np.array([[2, 0, 3, 9], [4, 4, 4, 4]])
    mask = (np.arange(20).reshape(2, 10) % 2 == 0)
    m, c = segment_mean_ref(v, d, [4, 3], [8, 10])
    assert c.tolist() == [[2, 0, 3, 3], [4, 4, 2, 0]] and m.tolist() == [[0.5, 0.0, 3.0, 6.0], [11.5, 15.5, 18.5, 0.0]]
    m, c = segment_mean_ref(v, d, [4, 3], [8, 10], mask)
    assert c.tolist() == [[1, 0, 2, 1], [2, 2, 1, 0]] and m.tolist() == [[0.0, 0.0, 3.0, 6.0], [11.0, 15.0, 18.0, 0.0]]


# ------------------------------------------------------------------------------------------------ the tool
class OracleFrontEnd:
    """MelFrontEnd's surface on the fp64 oracle, on the CPU"""

    def __init__(self, cfg):
        self.cfg, self.device = cfg, torch.device("cpu")
        self.fb = mel_filterbank_ref(cfg["sample_rate"], cfg["n_fft"], cfg["n_mels"], cfg["fmin"], cfg["fmax"])

    def __call__(self, wave, wave_lens):
        B, Nmax = wave.shape
        out = torch.zeros(B, 1 + Nmax // self.cfg["hop_length"], self.cfg["n_mels"])
        lens = torch.zeros(B, dtype=torch.int64)
        for b in range(B):
            m = logmel_ref(wave[b, :int(wave_lens[b])].numpy(), self.cfg, self.fb, CLIP)
            out[b, :len(m)] = torch.from_numpy(m).float()
            lens[b] = len(m)
        return {"melspec": out, "melspec_lens": lens}


class OraclePitchEnergy:
    """PitchEnergy's surface on the fp64 oracle, on the CPU; counts what the tool makes and calls"""
    made, calls = [], []

    def __init__(self, cfg, front_end):
        assert isinstance(front_end, OracleFrontEnd)                  # the tool hands over its front end (one window table)
        self.p = dict(SHIPPED, **{k: cfg[k] for k in ("sample_rate", "n_fft", "hop_length", "win_length")})
        OraclePitchEnergy.made.append(cfg["sample_rate"])

    def __call__(self, wave, wave_lens):
        OraclePitchEnergy.calls.append(tuple(wave.shape))
        B, Tmax = wave.size(0), 1 + wave.size(1) // self.p["hop_length"]
        out = {"f0": torch.zeros(B, Tmax), "voiced": torch.zeros(B, Tmax, dtype=torch.bool), "aperiodicity": torch.zeros(B, Tmax),
               "energy": torch.zeros(B, Tmax), "frames": torch.zeros(B, dtype=torch.int64)}
        for b, n in enumerate(wave_lens.tolist()):
            x = wave[b, :n].numpy()
            r, e = pitch_ref(x, self.p), energy_ref(x, self.p)
            T = r["frames"]
            out["frames"][b] = T
            out["f0"][b, :T], out["voiced"][b, :T] = torch.from_numpy(r["f0"]).float(), torch.from_numpy(r["voiced"])
            out["aperiodicity"][b, :T], out["energy"][b, :T] = torch.from_numpy(r["aperiodicity"]).float(), torch.from_numpy(e).float()
        return out


def test_preprocess_mel_adds_the_prosody_targets(tmp_path, monkeypatch):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import preprocess_mel as tool
    finally:
        sys.path.pop(0)
    from transformertts_amd.audio import read_wav, write_wav_pcm16
    cfg = dict(CONFIG_A, normalize_mel=False)
    data, out = tmp_path / "data", tmp_path / "out"
    (data / "wavs").mkdir(parents=True)
    files = [("a", 3000), ("b", 2100), ("c", 300), ("d", 5000)]       # c is too short to frame: skipped as before
    for i, (name, n) in enumerate(files):
        write_wav_pcm16(str(data / "wavs" / (name + ".wav")), glide_signal(n, SHIPPED, 40 + i), 22050)
    monkeypatch.setattr(tool, "make_front_end", OracleFrontEnd)
    monkeypatch.setattr(tool, "make_pitch_energy", OraclePitchEnergy)
    OraclePitchEnergy.made, OraclePitchEnergy.calls = [], []
    config = {"audio": cfg, "path": {"data": str(data), "preprocessed": str(out)}}
    logs = []
    assert tool.run(config, batch=3, stats_path=str(tmp_path / "s.json"), log=logs.append) == 3      # without the flag: as before
    assert OraclePitchEnergy.made == [] and sorted(np.load(str(out / "a.npz")).files) == ["melspec"]
    plain = {name: np.load(str(out / (name + ".npz")))["melspec"] for name, n in files if n > 512}
    logs2 = []
    assert tool.run(config, batch=3, stats_path=str(tmp_path / "s.json"), log=logs2.append, prosody=True) == 3
    assert [m.replace(str(tmp_path), "") for m in logs] == [m.replace(str(tmp_path), "") for m in logs2]      # the log is as before
    assert OraclePitchEnergy.made == [22050] and OraclePitchEnergy.calls == [(2, 3000), (1, 5000)]
    assert not os.path.exists(str(out / "c.npz"))
    for name, n in files:
        if n <= 512:
            continue
        x = read_wav(str(data / "wavs" / (name + ".wav")), 22050)
        d = np.load(str(out / (name + ".npz")))
        T = 1 + n // 256
        assert sorted(d.files) == ["energy", "f0", "melspec", "voiced"] and np.array_equal(d["melspec"], plain[name])
        assert d["melspec"].shape == (80, T) and d["f0"].shape == d["voiced"].shape == d["energy"].shape == (T,)
        assert d["f0"].dtype == d["energy"].dtype == np.float32 and d["voiced"].dtype == np.bool_
        r = pitch_ref(x, SHIPPED)
        assert np.array_equal(d["voiced"], r["voiced"]) and d["voiced"].any() and not d["voiced"].all()
        assert np.array_equal(d["f0"], r["f0"].astype(np.float32)) and (d["f0"][~d["voiced"]] == 0).all()
        assert np.array_equal(d["energy"], energy_ref(x, SHIPPED).astype(np.float32))
    assert "--prosody" in open(os.path.join(REPO, "tools", "preprocess_mel.py")).read()
