"""Band-limited resampler (csrc/resample.hip, transformertts_amd/audio.py): the fp64 oracle the GPU tests use against
scipy.signal.resample_poly; the host table against the oracle's weights; what the definition delivers (pass band, stop band);
lengths; every refusal of the entry point with its message, before any launch; read_wav_native; tools/preprocess_mel.py with
`resample=True` and tools/vocode_mel.py with `out_rate` on oracles; and the exports.  Host logic only, no GPU."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

from audio_reference import CLIP, CONFIG_A, logmel_ref, mel_filterbank_ref
from resample_reference import (BETA, PAIRS_SMALL, ROLLOFF, ZEROS, make_wave, out_len_ref, phase_weights_ref, prototype_ref, ratio_ref,
                                resample_ref)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ttts_resample_table_bytes", "ttts_resample_table_check", "ttts_resample_tile", "ttts_resample")
PAIRS = tuple((o, n, 6) for o, n in PAIRS_SMALL) + ((48000, 22050, ZEROS), (16000, 22050, ZEROS))
# (orig, new, zeros) -> (L, M, W, K), worked out by hand from s = rolloff * min(1, L / M), W = ceil(zeros / s), K = 2 W + 2
SHAPES = {(2, 1, 6): (1, 2, 13, 28), (1, 2, 6): (2, 1, 7, 16), (7, 5, 6): (5, 7, 9, 20), (5, 7, 6): (7, 5, 7, 16),
          (48000, 22050, 64): (147, 320, 148, 298), (16000, 22050, 64): (441, 320, 68, 138)}


def test_the_header_declares_each_entry_point_once_and_the_bindings_agree():
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
    P, I, L, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    assert _lib.SIGNATURES["ttts_resample_table_bytes"] == (Z, [I, I])
    assert _lib.SIGNATURES["ttts_resample_table_check"] == (I, [P, Z, I, I, I])
    assert _lib.SIGNATURES["ttts_resample_tile"] == (I, [])
    assert _lib.SIGNATURES["ttts_resample"] == (I, [P, L, P, I, I, I, I, I, P, P, L, P, P])
    for name in ("Resampler", "resample_table", "read_wav_native"):
        assert getattr(transformertts_amd, name) is getattr(audio, name) and name in transformertts_amd.__all__
    tile = lib.ttts_resample_tile()
    assert tile >= 64 and tile % 64 == 0
    src = open(os.path.join(REPO, "transformertts_amd", "csrc", "resample.hip")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert "sinf" not in code and "cosf" not in code and "atomic" not in code and "hipMalloc" not in code
    assert (audio.RESAMPLE_ZEROS, audio.RESAMPLE_ROLLOFF, audio.RESAMPLE_BETA) == (ZEROS, ROLLOFF, BETA)
    for const, name in ((audio.RESAMPLE_MAX_L, "RESAMPLE_MAX_L"), (audio.RESAMPLE_MAX_K, "RESAMPLE_MAX_K"),
                        (audio.RESAMPLE_MAX_RATIO, "RESAMPLE_MAX_RATIO")):
        assert re.search(name + r" = (\d+)", src).group(1) == str(const)


@pytest.mark.parametrize("orig,new,zeros", PAIRS)
def test_the_oracle_is_scipys_polyphase_filter_with_the_prototype_taps(orig, new, zeros):
    from scipy import signal
    L, M, s, W, K = ratio_ref(orig, new, zeros)
    x = make_wave(2500, 22050, orig + new).astype(np.float64)
    got = resample_ref(x, orig, new, zeros)
    want = signal.resample_poly(x, L, M, window=prototype_ref(orig, new, zeros) / L)      # scipy multiplies explicit taps by `up`
    assert got.shape == want.shape == (out_len_ref(x.size, L, M),)
    rel = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"resample oracle {orig} -> {new}: max |oracle - scipy| / max |scipy| = {rel:.2e}")
    assert rel <= 1e-12


def test_i0_by_its_series():
    from scipy import special
    from transformertts_amd.audio import bessel_i0
    x = np.concatenate([np.linspace(0.0, 20.0, 401), [BETA]])
    assert np.abs(bessel_i0(x) / special.i0(x) - 1.0).max() <= 1e-14
    assert np.abs(np.i0(x) / special.i0(x) - 1.0).max() <= 1e-14      # (the oracle's I0)
    assert float(bessel_i0(0.0)) == 1.0


@pytest.mark.parametrize("orig,new,zeros", PAIRS)
def test_the_table_is_the_oracles_weights_rounded_once(orig, new, zeros):
    from transformertts_amd import _lib
    from transformertts_amd.audio import resample_table
    table, L, M, K = resample_table(orig, new, zeros=zeros)
    _, _, _, W, _ = ratio_ref(orig, new, zeros)
    assert (L, M, W, K) == SHAPES[(orig, new, zeros)] and K == 2 * W + 2
    assert table.dtype == np.float32 and table.shape == (K, L) and table.flags["C_CONTIGUOUS"]      # tap-major: table[k * L + r]
    want = np.stack([phase_weights_ref(orig, new, r, zeros) for r in range(L)], axis=1)
    assert np.abs(table - want).max() <= 2.0 ** -25                   # |h| < 1: half an ulp of fp32 at the most
    # taps outside the window's support are exactly 0: tap 0 of every phase, the last tap of the phases with fraction 0
    assert (table[0] == 0).all() and table[K - 1, 0] == 0 and (table[1:K - 1] != 0).any(axis=0).all()
    dc = table.astype(np.float64).sum(axis=0)
    print(f"resample table {orig} -> {new}: DC gain of the phases {dc.min():.9f} .. {dc.max():.9f}")
    assert np.abs(dc - 1.0).max() <= 1e-3                             # measured: within 2.5e-7 of 1 for these six
    lib = _lib.load()
    assert lib.ttts_resample_table_bytes(L, K) == table.nbytes == 4 * L * K
    assert lib.ttts_resample_table_check(table.ctypes.data, table.nbytes, L, M, K) == 0, _lib.last_error()


def test_the_table_check_refuses():
    from transformertts_amd import _lib
    from transformertts_amd.audio import resample_table
    lib = _lib.load()
    table, L, M, K = resample_table(7, 5, zeros=6)

    def refused(buf, nbytes, l, m, k, needle):
        assert lib.ttts_resample_table_check(buf.ctypes.data if buf is not None else None, nbytes, l, m, k) != 0
        assert needle in _lib.last_error(), _lib.last_error()

    for bad in (np.nan, np.inf):
        t = table.copy()
        t[3, 2] = bad
        refused(t, t.nbytes, L, M, K, f"weight {3 * L + 2} (tap 3, phase 2) is not finite")
    refused(table, table.nbytes - 4, L, M, K, f"holds {table.nbytes - 4} bytes, {table.nbytes} expected")
    refused(table, table.nbytes, L, M, K + 1, f"K must be even and at least 4, got {K + 1}")
    refused(table, table.nbytes, L, M, 2, "K must be even and at least 4, got 2")
    refused(table, table.nbytes, 10, 4, K, "must be coprime (L 10, M 4, gcd 2)")
    refused(None, table.nbytes, L, M, K, "null pointer")
    assert lib.ttts_resample_table_bytes(L, K + 1) == 0 and lib.ttts_resample_table_bytes(0, K) == 0
    with pytest.raises(ValueError, match="the two rates are equal"):
        resample_table(22050, 22050)
    with pytest.raises(ValueError, match=r"needs L 1, M 16, K \d+; the kernel takes"):
        resample_table(16000, 1000)
    with pytest.raises(ValueError, match="needs L 22051, M 22050"):
        resample_table(22050, 22051)
    with pytest.raises(ValueError, match="positive integers"):
        resample_table(0, 22050)


@pytest.mark.parametrize("orig", [48000, 44100])
def test_what_the_definition_delivers_at_the_defaults(orig):
    """a sine at 0.85 of the new Nyquist comes back as itself, one at 1.1 times the new Nyquist does not come back"""
    new, n = 22050, 6000
    t_in, n_out = np.arange(n) / float(orig), out_len_ref(n, *ratio_ref(orig, new)[:2])
    t_out = np.arange(n_out) / float(new)
    mid = slice(n_out // 4, n_out - n_out // 4)
    f = 0.85 * new / 2.0
    err = float(np.abs(resample_ref(np.sin(2 * np.pi * f * t_in), orig, new) - np.sin(2 * np.pi * f * t_out))[mid].max())
    f = 1.1 * new / 2.0
    leak = float(np.abs(resample_ref(np.sin(2 * np.pi * f * t_in), orig, new))[mid].max())
    print(f"resample {orig} -> {new}: pass-band error {err:.2e}, stop-band {20 * math.log10(leak):.1f} dB")
    assert err <= 1e-6
    assert 20 * math.log10(leak) <= -120.0


def test_lengths():
    from transformertts_amd.audio import Resampler, resample_ratio
    for orig, new in ((48000, 22050), (16000, 22050), (2, 1), (5, 7)):
        L, M = resample_ratio(orig, new)
        for n in (0, 1, M - 1, M, M + 1):
            want = (n * L + M - 1) // M
            assert out_len_ref(n, L, M) == want == resample_ref(np.ones(n), orig, new, zeros=6).size
    rs = Resampler(22050, 22050)                                     # the identity needs no device
    assert (rs.L, rs.M, rs.table) == (1, 1, None) and rs.out_len(77) == 77


POINTERS = ("wave", "wave_lens", "table", "out", "out_lens")


def _call(lib, **kw):
    """ttts_resample on a host buffer: every case below is refused before a launch, so nothing dereferences it.  A pointer
    argument is None or a byte offset into the buffer."""
    buf = np.zeros(64, dtype=np.int64)
    a = dict(wave=0, ld_batch=4000, wave_lens=0, B=2, Nmax=4000, L=147, M=320, K=298, table=0, out=0, ld_out=1838, out_lens=0)
    a.update(kw)
    for name in POINTERS:
        a[name] = None if a[name] is None else buf.ctypes.data + a[name]
    return lib.ttts_resample(a["wave"], a["ld_batch"], a["wave_lens"], a["B"], a["Nmax"], a["L"], a["M"], a["K"], a["table"], a["out"],
                             a["ld_out"], a["out_lens"], None)


REFUSALS = [
    (dict(wave=None), "null pointer"), (dict(wave_lens=None), "null pointer"), (dict(table=None), "null pointer"),
    (dict(out=None), "null pointer"), (dict(out_lens=None), "null pointer"),
    (dict(B=0), "B must be in [1, 65535]"), (dict(B=0), "got 0"), (dict(B=65536), "got 65536"),
    (dict(Nmax=0), "Nmax must be in [1, 2^30]"), (dict(Nmax=0), "got 0"), (dict(Nmax=(1 << 30) + 1, ld_batch=1 << 31), f"got {(1 << 30) + 1}"),
    (dict(L=0), "rates must be positive (L 0, M 320)"), (dict(M=-1), "rates must be positive (L 147, M -1)"),
    (dict(L=320), "L == M (320) is the identity"),
    (dict(L=1025, M=1024), "at most 1024 phases, got L 1025"),
    (dict(L=9, M=1), "a factor of 8 at the most (L 9, M 1)"), (dict(L=1, M=9), "a factor of 8 at the most (L 1, M 9)"),
    (dict(K=1282), "at most 1280 taps, got K 1282"), (dict(K=297), "K must be even and at least 4, got 297"),
    (dict(K=2), "K must be even and at least 4, got 2"),
    (dict(ld_batch=3999), "the batch stride must be >= Nmax (ld_batch 3999, Nmax 4000)"),
    (dict(ld_out=1837), "the output stride must be >= Nout (ld_out 1837, Nout 1838)"),
    (dict(wave=2), "wave, table and out must be 4-byte aligned"), (dict(table=2), "wave, table and out must be 4-byte aligned"),
    (dict(out=6), "wave, table and out must be 4-byte aligned"),
    (dict(wave_lens=4), "wave_lens and out_lens must be 8-byte aligned"), (dict(out_lens=12), "wave_lens and out_lens must be 8-byte aligned"),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_every_refusal_names_its_value_before_any_launch(case):
    from transformertts_amd import _lib
    lib = _lib.load()
    kw, needle = REFUSALS[case]
    rc = _call(lib, **kw)
    assert rc != 0 and needle in _lib.last_error(), _lib.last_error()
    with pytest.raises(RuntimeError, match=re.escape(needle)):       # ... and reaches Python through _lib.check
        _lib.check(rc, "ttts_resample")


def test_read_wav_native_is_read_wav_without_the_rate_check(tmp_path):
    from transformertts_amd.audio import read_wav, read_wav_native, write_wav_pcm16
    x = make_wave(901, 16000, 4)
    p = str(tmp_path / "a.wav")
    write_wav_pcm16(p, x, 16000)
    got, rate = read_wav_native(p)
    assert rate == 16000 and isinstance(rate, int) and got.dtype == np.float32
    assert np.array_equal(got, read_wav(p, 16000)) and got.shape == (901,)
    with pytest.raises(ValueError, match=r"sampled at 16000 Hz, 22050 Hz expected \(there is no resampler\)"):
        read_wav(p, 22050)


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


class OracleResampler:
    """Resampler's surface on the fp64 oracle, on the CPU; counts what the tool makes and calls"""
    made, calls = [], []

    def __init__(self, orig, new):
        self.orig, self.new, self.device = orig, new, None
        OracleResampler.made.append((orig, new))

    def __call__(self, wave, wave_lens):
        OracleResampler.calls.append((self.orig, tuple(wave.shape)))
        rows = [resample_ref(wave[b, :int(n)].numpy(), self.orig, self.new) for b, n in enumerate(wave_lens.tolist())]
        out = torch.zeros(len(rows), out_len_ref(wave.size(1), *ratio_ref(self.orig, self.new)[:2]))
        for b, r in enumerate(rows):
            out[b, :r.size] = torch.from_numpy(r).float()
        return {"wave": out, "wave_lens": torch.tensor([r.size for r in rows], dtype=torch.int64)}


def test_preprocess_mel_resamples_a_directory_of_mixed_rates(tmp_path, monkeypatch):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import preprocess_mel as tool
    finally:
        sys.path.pop(0)
    from transformertts_amd.audio import read_wav_native, write_wav_pcm16
    cfg = dict(CONFIG_A, normalize_mel=False)
    data, out = tmp_path / "data", tmp_path / "out"
    (data / "wavs").mkdir(parents=True)
    files = [("a_native", 22050, 3000), ("b_16k", 16000, 2400), ("c_16k", 16000, 1700), ("d_native", 22050, 2100), ("e_48k", 48000, 5000)]
    for i, (name, rate, n) in enumerate(files):
        write_wav_pcm16(str(data / "wavs" / (name + ".wav")), make_wave(n, rate, 30 + i), rate)
    monkeypatch.setattr(tool, "make_front_end", OracleFrontEnd)
    monkeypatch.setattr(tool, "make_resampler", OracleResampler)
    OracleResampler.made, OracleResampler.calls = [], []
    config = {"audio": cfg, "path": {"data": str(data), "preprocessed": str(out)}}
    with pytest.raises(ValueError, match=r"sampled at 16000 Hz, 22050 Hz expected \(there is no resampler\)"):
        tool.run(config, batch=3, stats_path=str(tmp_path / "s.json"), log=lambda m: None)          # without the flag: as before
    assert tool.run(config, batch=3, stats_path=str(tmp_path / "s.json"), log=lambda m: None, resample=True) == 5
    assert sorted(OracleResampler.made) == [(16000, 22050), (48000, 22050)]                        # one per distinct rate
    assert OracleResampler.calls == [(16000, (2, 2400)), (48000, (1, 5000))]                       # grouped by rate within a batch
    fb = mel_filterbank_ref(22050, 1024, 80, 0.0, 8000.0)
    for name, rate, n in files:
        x, got_rate = read_wav_native(str(data / "wavs" / (name + ".wav")))
        assert got_rate == rate
        sig = x if rate == 22050 else resample_ref(x, rate, 22050).astype(np.float32)
        want = logmel_ref(sig, CONFIG_A, fb)
        d = np.load(str(out / (name + ".npz")))
        assert d["melspec"].shape == (80, 1 + sig.size // 256) and np.abs(d["melspec"].T - want).max() <= 1e-5
    # with the statistics pass the resamplers are shared by both passes
    OracleResampler.made = []

    class WithStats(OracleFrontEnd):
        def set_stats(self, mean, std):
            self.stats_set = (mean, std)

        def stats(self, mel, lens):
            rows = [mel[b, :int(lens[b])].double() for b in range(mel.size(0))]
            return sum(r.sum() for r in rows), sum((r ** 2).sum() for r in rows), sum(r.numel() for r in rows)

    monkeypatch.setattr(tool, "make_front_end", WithStats)
    config["audio"] = dict(CONFIG_A, normalize_mel=True)
    assert tool.run(config, batch=64, stats_path=str(tmp_path / "s.json"), log=lambda m: None, resample=True) == 5
    assert sorted(OracleResampler.made) == [(16000, 22050), (48000, 22050)]


def test_vocode_mel_writes_the_wave_at_another_rate(tmp_path, monkeypatch):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import vocode_mel as tool
    finally:
        sys.path.pop(0)
    from transformertts_amd.audio import read_wav_native
    cfg = dict(CONFIG_A, normalize_mel=False)
    T = 9
    x = make_wave((T - 1) * cfg["hop_length"], 22050, 8)

    class FixedVocoder:
        """a vocoder that returns one known wave: what is under test is what the tool does with it"""
        device = torch.device("cpu")

        def __call__(self, mel, lens):
            assert tuple(mel.shape) == (1, T, 80) and lens.tolist() == [T]
            return {"wave": torch.from_numpy(x)[None], "wave_lens": torch.tensor([x.size])}

    npz = tmp_path / "a.npz"
    np.savez(str(npz), melspec=np.zeros((80, T), np.float32))
    monkeypatch.setattr(tool, "make_resampler", OracleResampler)
    OracleResampler.made, OracleResampler.calls = [], []
    make = lambda audio_config, mean=None, std=None: FixedVocoder()
    for out_rate in (None, 22050):                                    # no flag, or the config's own rate: nothing is resampled
        n = tool.run({"audio": cfg}, str(npz), str(tmp_path / "same.wav"), make_vocoder=make, log=lambda s: None, out_rate=out_rate)
        y, rate = read_wav_native(str(tmp_path / "same.wav"))
        assert (n, rate) == (x.size, 22050) and np.abs(y - x).max() <= 1.0 / 32768 and OracleResampler.made == []
    n = tool.run({"audio": cfg}, str(npz), str(tmp_path / "16k.wav"), make_vocoder=make, log=lambda s: None, out_rate=16000)
    y, rate = read_wav_native(str(tmp_path / "16k.wav"))
    want = resample_ref(x, 22050, 16000)
    assert OracleResampler.made == [(22050, 16000)] and OracleResampler.calls == [(22050, (1, x.size))]
    assert rate == 16000 and n == y.size == want.size == out_len_ref(x.size, 320, 441)
    assert np.abs(y - want).max() <= 1.0 / 32768                      # PCM16 rounds to half a step


def test_the_tools_and_documents_no_longer_say_there_is_no_resampler():
    for rel in ("tools/preprocess_mel.py", "tools/vocode_mel.py", "README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(REPO, rel)).read()
        assert "no resampler" not in text, rel
    assert "--resample" in open(os.path.join(REPO, "tools", "preprocess_mel.py")).read()
    assert "--out-rate" in open(os.path.join(REPO, "tools", "vocode_mel.py")).read()
    assert "(there is no resampler)" in open(os.path.join(REPO, "transformertts_amd", "audio.py")).read()       # read_wav's message stays
