"""Log-mel front end (ABI v23, csrc/audio.hip, transformertts_amd/audio.py): the entry points are declared, bound and exported,
ctypes and the header agree, every refusal comes with its message before any launch; the fp64 oracle the GPU tests use against
torch.stft; the slaney filter bank, its packed form and the host tables against their definitions; read_wav; and the files
tools/preprocess_mel.py writes, with the front end replaced by the oracle.  Host logic only, no GPU."""
import ctypes
import json
import math
import os
import re
import struct
import sys
import wave as wave_mod

import numpy as np
import pytest
import torch

from audio_reference import (CLIP, CONFIG_A, CONFIG_B, logmel_ref, make_signal, mel_filterbank_ref, stats_ref, stft_ref, window_ref)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ttts_audio_tables_bytes", "ttts_audio_tables_check", "ttts_logmel", "ttts_logmel_stats")
CONFIGS = (CONFIG_A, CONFIG_B)


def _fb(cfg):
    from transformertts_amd.audio import mel_filterbank
    return mel_filterbank(cfg["sample_rate"], cfg["n_fft"], cfg["n_mels"], cfg["fmin"], cfg["fmax"])


def test_abi_version_and_the_header_declares_the_new_entry_points():
    from transformertts_amd import _lib, audio
    lib = _lib.load()
    assert lib.ttts_abi_version() >= 23
    hdr = open(os.path.join(REPO, "include", "ttts_hip.h")).read()
    declared = set(re.findall(r"\b(ttts_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, f"{name} is not declared in ttts_hip.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name), f"{name} is not exported / bound"
        decl = re.search(r"^(?:int|size_t) " + name + r"\s*\(([^;]*)\)\s*;", hdr, re.M).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name      # ctypes and the header agree on the argument count
    P, I, L, F, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_size_t
    assert _lib.SIGNATURES[NEW[0]] == (Z, [I, I, I])
    assert _lib.SIGNATURES[NEW[1]] == (I, [P, Z, I, I, I, I])
    assert _lib.SIGNATURES[NEW[2]] == (I, [P, L, P, I, I, I, I, I, I, P, F, P, P, P, I, P])
    assert _lib.SIGNATURES[NEW[3]] == (I, [P, P, I, I, I, P, P])
    block = hdr[hdr.index("ABI v23; audio.hip"):hdr.index("size_t ttts_audio_tables_bytes")]
    for needle in ("g = t * hop - n_fft/2 + n", "g < 0 reads sample -g", "g >= len reads sample 2 * (len - 1) - g",
                   "frames = 1 + len / hop", "Tmax = 1 + Nmax / hop", "0.5 - 0.5 cos(2 pi n / win_length)",
                   "left pad (n_fft - win_length) / 2", "{256, 512, 1024, 2048}", "(x - mean) / (std + 1e-8)",
                   "len <= n_fft/2 cannot be reflected", "hop < 1 or hop > n_fft", "win_length > n_fft", "misaligned pointers",
                   "B < 1", "n_fft not in the supported set", "no atomics"):
        assert needle in block, needle
    assert [int(re.search(rf"#define TTTS_AUDIO_{m} (\d+)", hdr).group(1)) for m in ("LOGMEL", "MAGNITUDE")] == [0, 1]
    assert audio.MODES == {"logmel": 0, "magnitude": 1}
    src = open(os.path.join(REPO, "transformertts_amd", "csrc", "audio.hip")).read()
    assert '#include "fft_lds.h"' in src and "sincos" not in src.replace("No sincosf", "")
    fft = open(os.path.join(REPO, "transformertts_amd", "csrc", "fft_lds.h")).read()
    assert "template <int M, int DIR, int THREADS>" in fft and "FFT_INVERSE" in fft      # the direction is a template parameter
    import transformertts_amd
    for name in ("MelFrontEnd", "mel_filterbank", "read_wav", "normalize", "denormalize"):
        assert getattr(transformertts_amd, name) is getattr(audio, name)
    assert audio.normalize(3.0, 1.0, 2.0) == 2.0 / (2.0 + 1e-8) and audio.denormalize(audio.normalize(3.0, 1.0, 2.0), 1.0, 2.0) == 3.0


def test_entry_points_refuse_bad_arguments_with_a_message():
    from transformertts_amd import _lib, audio
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096 + 16)
    a = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)          # a 16-byte aligned host address (never dereferenced)
    a2, a4 = ctypes.c_void_p(a.value + 2), ctypes.c_void_p(a.value + 4)

    def bad(rc, needle):
        assert rc == -1, rc
        assert needle in _lib.last_error(), _lib.last_error()

    names = ["wave", "ld_batch", "wave_lens", "B", "Nmax", "n_fft", "hop", "n_mels", "nnz", "tables", "clip_val", "mean_std", "out",
             "mel_lens", "mode", "stream"]
    defaults = dict(wave=a, ld_batch=4037, wave_lens=a, B=4, Nmax=4037, n_fft=1024, hop=256, n_mels=80, nnz=727, tables=a,
                    clip_val=1e-5, mean_std=None, out=a, mel_lens=a, mode=0, stream=None)

    def logmel(**kw):
        assert not set(kw) - set(names)
        return lib.ttts_logmel(*[kw.get(n, defaults[n]) for n in names])

    e = "logmel"
    for p in ("wave", "wave_lens", "tables", "out", "mel_lens"):
        bad(logmel(**{p: None}), e + ": null pointer")
    bad(logmel(B=0), e + ": sizes must be positive (B 0, Nmax 4037)")
    bad(logmel(B=-3), e + ": sizes must be positive (B -3, Nmax 4037)")
    bad(logmel(Nmax=0, ld_batch=0), e + ": sizes must be positive (B 4, Nmax 0)")
    for n in (0, 128, 1000, 1023, 4096):
        bad(logmel(n_fft=n), e + f": n_fft must be one of 256, 512, 1024, 2048, got {n}")
    bad(logmel(hop=0), e + ": hop must be in [1, n_fft] (hop 0, n_fft 1024)")
    bad(logmel(hop=1025), e + ": hop must be in [1, n_fft] (hop 1025, n_fft 1024)")
    bad(logmel(n_mels=0), e + ": sizes must be positive (n_mels 0, nnz 727)")
    bad(logmel(nnz=0), e + ": sizes must be positive (n_mels 80, nnz 0)")
    bad(logmel(Nmax=(1 << 30) + 1, ld_batch=1 << 31), e + ": more than 2^30 samples per utterance are not supported (Nmax 1073741825)")
    bad(logmel(n_mels=513), e + ": at most 512 filters and 4096 weights (n_mels 513, nnz 727)")
    bad(logmel(nnz=4097), e + ": at most 512 filters and 4096 weights (n_mels 80, nnz 4097)")
    bad(logmel(mode=2), e + ": unknown mode 2")
    bad(logmel(mode=-1), e + ": unknown mode -1")
    bad(logmel(ld_batch=4036), e + ": the batch stride must be >= Nmax (ld_batch 4036, Nmax 4037)")
    bad(logmel(clip_val=0.0), e + ": clip_val must be positive")
    for p in ("wave", "tables", "out", "mean_std"):
        bad(logmel(**{p: a2}), e + ": wave, tables, mean_std and out must be 4-byte aligned")
    for p in ("wave_lens", "mel_lens"):
        bad(logmel(**{p: a4}), e + ": wave_lens and mel_lens must be 8-byte aligned")
    bad(logmel(B=65536), e + ": grid too large (B 65536, at most 65535 utterances a call)")

    e = "logmel_stats"
    stats = lambda mel=a, lens=a, B=4, T=16, C=80, sums=a: lib.ttts_logmel_stats(mel, lens, B, T, C, sums, None)
    bad(stats(mel=None), e + ": null pointer")
    bad(stats(lens=None), e + ": null pointer")
    bad(stats(sums=None), e + ": null pointer")
    bad(stats(B=0), e + ": sizes must be positive (B 0, Tmax 16, n_mels 80)")
    bad(stats(T=0), e + ": sizes must be positive (B 4, Tmax 0, n_mels 80)")
    bad(stats(C=-1), e + ": sizes must be positive (B 4, Tmax 16, n_mels -1)")
    bad(stats(mel=a2), e + ": mel must be 4-byte aligned")
    bad(stats(lens=a4), e + ": mel_lens and sums must be 8-byte aligned")
    bad(stats(sums=a4), e + ": mel_lens and sums must be 8-byte aligned")

    # the tables: size query and the check of a host copy
    assert lib.ttts_audio_tables_bytes(1000, 80, 727) == 0 and lib.ttts_audio_tables_bytes(1024, 0, 727) == 0
    assert lib.ttts_audio_tables_bytes(1024, 80, 0) == 0
    tables, nnz = audio.build_tables(512, 400, _fb(CONFIG_B))
    assert lib.ttts_audio_tables_bytes(512, 40, nnz) == tables.nbytes == 4 * audio.table_layout(512, 40, nnz)["words"]
    chk = lambda t=tables, nbytes=None, n_fft=512, win=400, n_mels=40, nz=nnz: lib.ttts_audio_tables_check(
        t.ctypes.data, t.nbytes if nbytes is None else nbytes, n_fft, win, n_mels, nz)
    e = "audio_tables_check"
    assert chk() == 0
    assert lib.ttts_audio_tables_check(None, 4, 512, 400, 40, nnz) == -1 and e + ": null pointer" in _lib.last_error()
    bad(chk(n_fft=500), e + ": n_fft must be one of 256, 512, 1024, 2048, got 500")
    bad(chk(win=513), e + ": win_length must be in [1, n_fft] (win_length 513, n_fft 512)")
    bad(chk(win=0), e + ": win_length must be in [1, n_fft] (win_length 0, n_fft 512)")
    bad(chk(n_mels=0), e + ": sizes must be positive (n_mels 0,")
    bad(chk(nbytes=tables.nbytes - 4), e + f": the tables hold {tables.nbytes - 4} bytes, {tables.nbytes} expected")
    bad(chk(win=401), e + ": the header does not match (n_fft 512, win_length 401, n_mels 40,")
    lay = audio.table_layout(512, 40, nnz)
    t = tables.copy()
    t[lay["first"] + 39] = 250                                        # the last filter would run past bin 256
    bad(chk(t=t), e + ": filter 39 leaves the 257 bins (first 250,")
    t = tables.copy()
    t[lay["offset"] + 5] += 1
    bad(chk(t=t), e + ": filter 5 starts at weight")
    t = tables.copy()
    t[lay["count"] + 39] -= 1
    bad(chk(t=t), e + ": the filters hold")
    with pytest.raises(ValueError, match="n_fft must be one of"):
        audio.build_tables(768, 768, np.ones((4, 385)))
    with pytest.raises(ValueError, match="win_length must be in \\[1, n_fft\\]"):
        audio.build_tables(512, 513, _fb(CONFIG_B))


LENGTHS = lambda cfg: [cfg["n_fft"] // 2 + 1, 5 * cfg["hop_length"], 8 * cfg["hop_length"] - 1, 4000]


def test_the_oracle_stft_is_torch_stft_in_fp64():
    for cfg in CONFIGS:
        n_fft, hop, win = cfg["n_fft"], cfg["hop_length"], cfg["win_length"]
        assert np.abs(window_ref(win, win) - torch.hann_window(win, periodic=True, dtype=torch.float64).numpy()).max() < 1e-15
        for i, n in enumerate(LENGTHS(cfg)):
            x = make_signal(n, cfg["sample_rate"], 40 + i).astype(np.float64)
            want = torch.stft(torch.from_numpy(x), n_fft, hop_length=hop, win_length=win, center=True, pad_mode="reflect",
                              window=torch.hann_window(win, periodic=True, dtype=torch.float64), return_complex=True).numpy().T
            got = stft_ref(x, n_fft, hop, win)
            assert got.shape == want.shape == (1 + n // hop, n_fft // 2 + 1)
            assert np.abs(got - want).max() <= 1e-12, (cfg["n_fft"], n, np.abs(got - want).max())


def test_the_filter_bank_is_the_definition_and_is_well_formed():
    for cfg, least in ((CONFIG_A, 3), (CONFIG_B, 4)):
        fb = _fb(cfg)
        ref = mel_filterbank_ref(cfg["sample_rate"], cfg["n_fft"], cfg["n_mels"], cfg["fmin"], cfg["fmax"])
        assert fb.dtype == np.float64 and fb.shape == ref.shape == (cfg["n_mels"], cfg["n_fft"] // 2 + 1)
        assert np.abs(fb - ref).max() <= 1e-12
        assert (fb >= 0).all()
        nz = (fb > 0).sum(1)
        assert nz.min() >= least, nz.min()                            # no empty row
        peaks = fb.argmax(1)
        assert (np.diff(peaks) > 0).all()                             # row peaks increase in frequency
        for row, p in zip(fb, peaks):                                 # unimodal: up to the peak, down after it
            assert (np.diff(row[:p + 1]) >= 0).all() and (np.diff(row[p:]) <= 0).all()
    with pytest.raises(ValueError, match="0 <= fmin < fmax"):
        from transformertts_amd.audio import mel_filterbank
        mel_filterbank(16000, 512, 40, 8000.0, 8000.0)


def test_the_packed_filters_and_the_host_tables():
    from transformertts_amd import audio
    for cfg in CONFIGS:
        n_fft, win, n_mels = cfg["n_fft"], cfg["win_length"], cfg["n_mels"]
        M = n_fft // 2
        fb = _fb(cfg)
        first, count, offset, weights = audio.pack_filters(fb)
        assert weights.dtype == np.float32 and first.dtype == count.dtype == offset.dtype == np.int32
        assert np.array_equal(audio.unpack_filters(first, count, offset, weights, M + 1), fb.astype(np.float32))
        assert int(count.sum()) == weights.size == int((fb > 0).sum())       # triangles: no zero inside a span
        assert np.array_equal(offset, np.cumsum(count) - count)
        tables, nnz = audio.build_tables(n_fft, win, fb)
        lay = audio.table_layout(n_fft, n_mels, nnz)
        assert tables.dtype == np.int32 and tables.size == lay["words"] and nnz == weights.size
        assert list(tables[:8]) == [audio.MAGIC, n_fft, win, n_mels, nnz, 0, 0, 0]
        f32 = tables.view(np.float32)
        sect = lambda name, n: f32[lay[name]:lay[name] + n]
        assert np.array_equal(sect("window", n_fft), window_ref(win, n_fft).astype(np.float32))
        left = (n_fft - win) // 2
        assert (sect("window", n_fft)[:left] == 0).all() and (sect("window", n_fft)[left + win:] == 0).all()
        k = np.arange(M, dtype=np.float64)
        assert np.array_equal(sect("tw_re", M), np.cos(2 * np.pi * k / M).astype(np.float32))
        assert np.array_equal(sect("tw_im", M), (-np.sin(2 * np.pi * k / M)).astype(np.float32))
        k = np.arange(M // 2 + 1, dtype=np.float64)
        assert np.array_equal(sect("pw_re", M // 2 + 1), np.cos(2 * np.pi * k / n_fft).astype(np.float32))
        assert np.array_equal(sect("pw_im", M // 2 + 1), (-np.sin(2 * np.pi * k / n_fft)).astype(np.float32))
        assert np.array_equal(tables[lay["first"]:lay["first"] + n_mels], first)
        assert np.array_equal(tables[lay["count"]:lay["count"] + n_mels], count)
        assert np.array_equal(tables[lay["offset"]:lay["offset"] + n_mels], offset)
        assert np.array_equal(sect("weights", nnz), weights)
    # a short window is centred: win 400 in 512 starts at 56
    assert np.flatnonzero(audio.hann_window(400, 512))[0] == 57 and audio.hann_window(400, 512)[56] == 0.0


def _riff(path, code, bits, channels, rate, payload):
    fmt = struct.pack("<HHIIHH", code, channels, rate, rate * channels * bits // 8, channels * bits // 8, bits)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"LIST" + struct.pack("<I", 3) + b"abc\0" + \
        b"data" + struct.pack("<I", len(payload)) + payload
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def test_read_wav_round_trips_and_refuses(tmp_path):
    from transformertts_amd.audio import read_wav, write_wav_pcm16
    rng = np.random.default_rng(3)
    pcm = rng.integers(-32768, 32768, 1001).astype("<i2")
    pcm[:3] = (-32768, 32767, 0)
    p16 = str(tmp_path / "a.wav")
    with wave_mod.open(p16, "wb") as w:                               # the standard library's writer
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(22050)
        w.writeframes(pcm.tobytes())
    x = read_wav(p16, 22050)
    assert x.dtype == np.float32 and x.shape == (1001,) and np.array_equal(x, pcm.astype(np.float32) / 32768.0)
    assert x.min() == -1.0 and x.max() < 1.0
    write_wav_pcm16(str(tmp_path / "b.wav"), x, 22050)
    assert np.array_equal(read_wav(str(tmp_path / "b.wav"), 22050), x)
    f32 = rng.standard_normal(333).astype("<f4") * 0.1
    _riff(str(tmp_path / "f.wav"), 3, 32, 1, 16000, f32.tobytes())     # with a LIST chunk of odd size in front of the data
    assert np.array_equal(read_wav(str(tmp_path / "f.wav"), 16000), f32)
    i24 = rng.integers(-(1 << 23), 1 << 23, 77)
    raw = b"".join(struct.pack("<i", int(v))[:3] for v in i24)
    _riff(str(tmp_path / "c.wav"), 1, 24, 1, 16000, raw)
    assert np.array_equal(read_wav(str(tmp_path / "c.wav"), 16000), (i24 / float(1 << 23)).astype(np.float32))
    i32 = rng.integers(-(1 << 31), 1 << 31, 55).astype("<i4")
    _riff(str(tmp_path / "d.wav"), 1, 32, 1, 16000, i32.tobytes())
    assert np.array_equal(read_wav(str(tmp_path / "d.wav"), 16000), (i32 / float(1 << 31)).astype(np.float32))
    with pytest.raises(ValueError, match="sampled at 22050 Hz, 16000 Hz expected"):
        read_wav(p16, 16000)
    _riff(str(tmp_path / "s.wav"), 1, 16, 2, 22050, pcm[:1000].tobytes())
    with pytest.raises(ValueError, match="has 2 channels, mono expected"):
        read_wav(str(tmp_path / "s.wav"), 22050)
    _riff(str(tmp_path / "u.wav"), 1, 8, 1, 22050, b"\x80" * 10)
    with pytest.raises(ValueError, match="format code 1 with 8 bits"):
        read_wav(str(tmp_path / "u.wav"), 22050)
    (tmp_path / "n.wav").write_bytes(b"not a wave file at all")
    with pytest.raises(ValueError, match="not a RIFF/WAVE file"):
        read_wav(str(tmp_path / "n.wav"), 22050)


class OracleFrontEnd:
    """MelFrontEnd's surface on the fp64 oracle, on the CPU"""

    def __init__(self, cfg):
        self.cfg, self.device, self.mean, self.std = cfg, torch.device("cpu"), None, None
        self.fb = mel_filterbank_ref(cfg["sample_rate"], cfg["n_fft"], cfg["n_mels"], cfg["fmin"], cfg["fmax"])

    def set_stats(self, mean, std):
        self.mean, self.std = mean, std

    def __call__(self, wave, wave_lens):
        B, Nmax = wave.shape
        Tmax = 1 + Nmax // self.cfg["hop_length"]
        out = torch.zeros(B, Tmax, self.cfg["n_mels"])
        lens = torch.zeros(B, dtype=torch.int64)
        for b in range(B):
            m = logmel_ref(wave[b, :int(wave_lens[b])].numpy(), self.cfg, self.fb, CLIP, self.mean, self.std)
            out[b, :len(m)] = torch.from_numpy(m).float()
            lens[b] = len(m)
        return {"melspec": out, "melspec_lens": lens}

    def stats(self, mel, lens):
        rows = [mel[b, :int(lens[b])].double() for b in range(mel.size(0))]
        return sum(r.sum() for r in rows), sum((r ** 2).sum() for r in rows), sum(r.numel() for r in rows)


def test_preprocess_mel_writes_what_the_dataset_reads(tmp_path, monkeypatch):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import preprocess_mel as tool
    finally:
        sys.path.pop(0)
    from transformertts_amd.audio import write_wav_pcm16, read_wav
    from transformertts_amd.dataset import TransformerTTSDataset, collate_fn
    cfg = dict(CONFIG_B, normalize_mel=True)
    data, seqs, out = tmp_path / "data", tmp_path / "seqs", tmp_path / "out"
    (data / "wavs").mkdir(parents=True)
    seqs.mkdir()
    names = ["LJ001-0001", "LJ004-0002", "LJ004-0003", "LJ004-0004"]
    lens = [700, 1500, 257, 100]                                      # the last one is too short to frame (n_fft/2 + 1 = 257)
    for i, (name, n) in enumerate(zip(names, lens)):
        write_wav_pcm16(str(data / "wavs" / (name + ".wav")), make_signal(n, 16000, 70 + i), 16000)
        np.savez(str(seqs / (name + ".npz")), melspec=np.zeros((40, 3), np.float32), transcript=f"text {i}",
                 phoneme=np.array(["AH", "B"]), sequence=np.arange(5 + i))
    monkeypatch.setattr(tool, "make_front_end", OracleFrontEnd)
    config = {"audio": cfg, "path": {"data": str(data), "preprocessed": str(out)}}
    said = []
    assert tool.run(config, batch=2, sequences=str(seqs), stats_path=str(tmp_path / "stats.json"), log=said.append) == 3
    assert sorted(os.listdir(out)) == [n + ".npz" for n in names[:3]]
    assert any("skipped" in s and "LJ004-0004" in s for s in said)
    fb = mel_filterbank_ref(16000, 512, 40, 50.0, 8000.0)
    sigs = [read_wav(str(data / "wavs" / (n + ".wav")), 16000) for n in names[:3]]
    raw = [logmel_ref(s, CONFIG_B, fb) for s in sigs]
    s, q, n, mean, std = stats_ref(raw)                               # preprocess.py:59-61
    stats = json.load(open(tmp_path / "stats.json"))
    assert sorted(stats) == ["mean", "std"]
    assert abs(stats["mean"] - mean) <= 1e-6 * abs(mean) and abs(stats["std"] - std) <= 1e-6 * std
    for i, name in enumerate(names[:3]):
        d = np.load(str(out / (name + ".npz")), allow_pickle=True)
        assert sorted(d.files) == ["melspec", "phoneme", "sequence", "transcript"]
        T = 1 + lens[i] // 128
        assert d["melspec"].dtype == np.float32 and d["melspec"].shape == (40, T) and d["melspec"].flags["C_CONTIGUOUS"]
        want = (raw[i] - mean) / (std + 1e-8)
        assert np.abs(d["melspec"].T - want).max() <= 1e-5
        assert str(d["transcript"]) == f"text {i}" and np.array_equal(d["sequence"], np.arange(5 + i))
    ds_train = TransformerTTSDataset(config, "train")
    ds_valid = TransformerTTSDataset(config, "valid")
    assert len(ds_train) == 2 and len(ds_valid) == 1
    batch = collate_fn([ds_train[0], ds_train[1]])
    assert tuple(batch["melspec"].shape) == (2, 1 + 1500 // 128, 40) and sorted(batch["melspec_lens"].tolist()) == [3, 12]
    # without --sequences: melspec only, and the tool says so; no statistics when the config does not ask for them
    out2 = tmp_path / "out2"
    config2 = {"audio": dict(CONFIG_B, normalize_mel=False), "path": {"data": str(data), "preprocessed": str(out2)}}
    said = []
    assert tool.run(config2, batch=64, stats_path=str(tmp_path / "none.json"), log=said.append) == 3
    assert any("melspec` only" in s for s in said) and not os.path.exists(tmp_path / "none.json")
    d = np.load(str(out2 / "LJ004-0002.npz"))
    assert d.files == ["melspec"] and np.abs(d["melspec"].T - raw[1]).max() <= 1e-5
