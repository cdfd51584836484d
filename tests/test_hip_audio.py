"""Log-mel front end on the GPU (csrc/audio.hip, csrc/fft_lds.h, transformertts_amd/audio.py, ABI v23) against the fp64 oracle of
tests/audio_reference.py: frame counts, reads inside the lengths (NaN behind them), zero rows, the clip, the accuracy of the
magnitude spectrogram and the log-mel (rel-L2 <= 1e-4, and the log-mel's largest error within 4 x that of the stock fp32 torch
restatement on the CPU: both are fp32 with O(log N) round-off and differ only in summation order), normalisation from device
statistics, the statistics, repeatability, graph capture, a strided input, the two radix depths the configs do not reach, and
the tiny model fed straight from the front end."""
import functools
import math

import numpy as np
import pytest
import torch

from audio_reference import CLIP, CONFIG_A, CONFIG_B, logmel_ref, magnitude_ref, make_signal, mel_filterbank_ref, ragged_batch, stats_ref
from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CONFIGS = {"A": CONFIG_A, "B": CONFIG_B}
FRAMES = {"A": [3, 6, 8, 16], "B": [3, 6, 8, 32]}
CLIPPED = {"A": 160, "B": 320}
LOG_CLIP = np.float32(math.log(float(np.float32(CLIP))))           # log of the fp32 clip value, rounded once


@functools.lru_cache(maxsize=None)
def _front_end(name):
    from transformertts_amd.audio import MelFrontEnd
    return MelFrontEnd(CONFIGS[name], device=DEV)


@functools.lru_cache(maxsize=None)
def _case(name, seed=0):
    """the ragged batch of a config, its oracle (computed once, never modified) and the stock fp32 restatement's error"""
    cfg = CONFIGS[name]
    wave, lens, sigs = ragged_batch(cfg, seed)
    fb = mel_filterbank_ref(cfg["sample_rate"], cfg["n_fft"], cfg["n_mels"], cfg["fmin"], cfg["fmax"])
    mags = [magnitude_ref(s, cfg) for s in sigs]
    mels = [logmel_ref(s, cfg, fb) for s in sigs]
    # stock torch in fp32 on the CPU: torch.stft, an fp32 filter-bank matmul, log
    win = torch.hann_window(cfg["win_length"], periodic=True, dtype=torch.float32)
    fb32 = torch.from_numpy(fb).float()
    stock_err, stock = 0.0, []
    for s, want in zip(sigs, mels):
        spec = torch.stft(torch.from_numpy(s), cfg["n_fft"], hop_length=cfg["hop_length"], win_length=cfg["win_length"], window=win,
                          center=True, pad_mode="reflect", return_complex=True).abs().T
        stock.append(torch.log(torch.clamp(spec @ fb32.T, min=CLIP)))
        stock_err = max(stock_err, float(np.abs(stock[-1].double().numpy() - want).max()))
    for a in mags + mels:
        a.setflags(write=False)
    return dict(cfg=cfg, wave=wave, lens=lens, sigs=sigs, fb=fb, mags=mags, mels=mels, stock=stock, stock_err=stock_err)


def _device_batch(case):
    return torch.from_numpy(case["wave"]).to(DEV), torch.tensor(case["lens"], device=DEV)


def _valid(out, lens):
    return np.concatenate([out[b, :n].reshape(-1) for b, n in enumerate(lens)])


def _errors(got, want_rows, lens):
    """rel-L2 and max-abs of the valid rows of a (B, T, C) device result against the per-utterance fp64 rows"""
    g = _valid(got.double().cpu().numpy(), lens)
    w = np.concatenate([r.reshape(-1) for r in want_rows])
    return float(np.linalg.norm(g - w) / np.linalg.norm(w)), float(np.abs(g - w).max())


@pytest.mark.parametrize("name", ["A", "B"])
def test_frames_lengths_zero_rows_and_the_clip(name):
    case, fe = _case(name), _front_end(name)
    cfg = case["cfg"]
    wave, lens = _device_batch(case)
    Tmax = 1 + wave.size(1) // cfg["hop_length"]
    for out, key, width in ((fe(wave, lens), "melspec", cfg["n_mels"]), (fe.spectrogram(wave, lens), "spectrogram", cfg["n_fft"] // 2 + 1)):
        x, frames = out[key], out["melspec_lens"]
        assert tuple(x.shape) == (4, Tmax, width) and x.dtype == torch.float32 and frames.dtype == torch.int64
        assert frames.tolist() == [1 + n // cfg["hop_length"] for n in case["lens"]] == FRAMES[name]
        assert not bool(torch.isnan(x).any()), "a sample behind a length was read"
        for b, n in enumerate(FRAMES[name]):
            assert bool((x[b, n:] == 0).all()), "rows beyond mel_lens must be exactly zero"
    mel = fe(wave, lens)["melspec"].cpu().numpy()
    want = case["mels"][3]
    at_clip = case["mags"][3] @ case["fb"].T <= CLIP
    assert (want[at_clip] == want[at_clip][0]).all() and abs(want[at_clip][0] - math.log(CLIP)) < 1e-12
    assert int(at_clip.sum()) == CLIPPED[name]                        # frames that lie wholly in the zeroed samples
    assert (mel[3, :FRAMES[name][3]][at_clip] == LOG_CLIP).all()
    assert int((mel[3, :FRAMES[name][3]] == LOG_CLIP).sum()) == CLIPPED[name]
    assert bool((fe.spectrogram(wave, lens)["spectrogram"][3, :FRAMES[name][3]].cpu().numpy()[at_clip.all(1)] == 0).all())


@pytest.mark.parametrize("name", ["A", "B"])
def test_accuracy_against_the_fp64_oracle(name):
    case, fe = _case(name), _front_end(name)
    wave, lens = _device_batch(case)
    mag_rel, mag_abs = _errors(fe.spectrogram(wave, lens)["spectrogram"], case["mags"], FRAMES[name])
    mel_rel, mel_abs = _errors(fe(wave, lens)["melspec"], case["mels"], FRAMES[name])
    print(f"audio accuracy config {name}: magnitude rel-L2 {mag_rel:.3e} max-abs {mag_abs:.3e}; log-mel rel-L2 {mel_rel:.3e} "
          f"max-abs {mel_abs:.3e}; stock fp32 torch (CPU) log-mel max-abs {case['stock_err']:.3e}")
    assert mag_rel <= 1e-4 and mel_rel <= 1e-4
    assert mel_abs <= 4 * case["stock_err"]


@pytest.mark.parametrize("name", ["A", "B"])
def test_statistics_and_normalisation_without_a_host_round_trip(name):
    from transformertts_amd.audio import MelFrontEnd
    case = _case(name)
    fe = MelFrontEnd(case["cfg"], device=DEV)
    wave, lens = _device_batch(case)
    raw = fe(wave, lens)
    s, q, n = fe.stats(raw["melspec"], raw["melspec_lens"])
    assert s.is_cuda and q.is_cuda and n.is_cuda and s.dtype == q.dtype == torch.float64
    ws, wq, wn, mean, std = stats_ref(case["mels"])
    assert int(n) == wn == sum(FRAMES[name]) * case["cfg"]["n_mels"]
    assert abs(float(s) - ws) <= 1e-4 * abs(ws) and abs(float(q) - wq) <= 1e-4 * abs(wq)
    s2, q2, _ = fe.stats(raw["melspec"], raw["melspec_lens"])
    assert float(s2) == float(s) and float(q2) == float(q)            # a fixed order: the same bits
    dmean, dstd = fe.mean_std_from(s, q, n)                           # device scalars
    assert dmean.is_cuda and dstd.is_cuda
    fe.set_stats(dmean, dstd)
    assert abs(float(fe.mean_std[0]) - mean) <= 1e-5 * abs(mean) and abs(float(fe.mean_std[1]) - std) <= 1e-5 * std
    out = fe(wave, lens)
    want = [(m - mean) / (std + 1e-8) for m in case["mels"]]
    rel, err = _errors(out["melspec"], want, FRAMES[name])
    # the same bounds: the stock fp32 restatement, normalised in fp32 with the same statistics, against the same oracle
    m32, s32 = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)
    stock_err = max(float(np.abs(((g - m32) / (s32 + 1e-8)).double().numpy() - w).max()) for g, w in zip(case["stock"], want))
    print(f"audio normalised config {name}: rel-L2 {rel:.3e} max-abs {err:.3e}; stock fp32 torch (CPU) max-abs {stock_err:.3e}")
    assert rel <= 1e-4
    assert err <= 4 * stock_err
    for b, t in enumerate(FRAMES[name]):
        assert bool((out["melspec"][b, t:] == 0).all())
    fe.set_stats(None, None)
    assert torch.equal(fe(wave, lens)["melspec"], raw["melspec"])
    fe2 = MelFrontEnd(case["cfg"], device=DEV, mean=mean, std=std)    # host floats at construction: the same values
    assert torch.allclose(fe2(wave, lens)["melspec"], out["melspec"], rtol=0, atol=1e-5)


@pytest.mark.parametrize("name", ["A", "B"])
def test_repeatable_strided_and_captured(name):
    case, fe = _case(name), _front_end(name)
    wave, lens = _device_batch(case)
    first = fe(wave, lens)
    again = fe(wave, lens)
    assert torch.equal(first["melspec"], again["melspec"]) and torch.equal(first["melspec_lens"], again["melspec_lens"])
    big = torch.full((4, wave.size(1) + 8), float("nan"), device=DEV)
    big[:, 3:3 + wave.size(1)] = wave
    view = big[:, 3:3 + wave.size(1)]
    assert view.stride(0) != wave.size(1)
    strided = fe(view, lens)
    assert torch.equal(strided["melspec"], first["melspec"])
    assert torch.equal(fe.spectrogram(view, lens)["spectrogram"], fe.spectrogram(wave, lens)["spectrogram"])
    # captured, then replayed on a second waveform copied into the same buffers
    other = _case(name, 1)
    wave2 = torch.from_numpy(np.ascontiguousarray(other["wave"][::-1])).to(DEV)          # the utterances in reverse order
    lens2 = torch.tensor(other["lens"][::-1], device=DEV)
    eager2 = fe(wave2, lens2)
    sw, sl = wave.clone(), lens.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fe(sw, sl)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out["melspec"], first["melspec"]) and torch.equal(out["melspec_lens"], first["melspec_lens"])
    sw.copy_(wave2)
    sl.copy_(lens2)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out["melspec"], eager2["melspec"]) and torch.equal(out["melspec_lens"], eager2["melspec_lens"])
    assert out["melspec_lens"].tolist() == FRAMES[name][::-1]


@pytest.mark.parametrize("n_fft", [256, 2048])
def test_the_other_radix_depths(n_fft):
    from transformertts_amd.audio import MelFrontEnd
    cfg = dict(sample_rate=22050, n_fft=n_fft, hop_length=n_fft // 4, win_length=n_fft, n_mels=20, fmin=0.0, fmax=8000.0)
    n = 3 * n_fft + 5
    x = make_signal(n, 22050, 7 + n_fft)
    wave = torch.full((1, n + 11), float("nan"))
    wave[0, :n] = torch.from_numpy(x)
    fe = MelFrontEnd(cfg, device=DEV)
    out = fe.spectrogram(wave.to(DEV), torch.tensor([n], device=DEV))
    T = 1 + n // cfg["hop_length"]
    assert out["melspec_lens"].tolist() == [T] and tuple(out["spectrogram"].shape) == (1, 1 + (n + 11) // cfg["hop_length"], n_fft // 2 + 1)
    rel = rel_l2(out["spectrogram"][0, :T], torch.from_numpy(magnitude_ref(x, cfg)))
    print(f"audio n_fft {n_fft}: magnitude rel-L2 {rel:.3e}")
    assert rel <= 1e-4
    assert not bool(torch.isnan(out["spectrogram"]).any()) and bool((out["spectrogram"][0, T:] == 0).all())


def test_an_utterance_too_short_to_reflect_gets_zero_frames():
    from transformertts_amd.audio import MelFrontEnd
    fe = _front_end("B")
    case = _case("B")
    wave, _ = _device_batch(case)
    lens = torch.tensor([256, 0, 257, -5], device=DEV)                # n_fft/2 = 256 cannot be reflected, 257 can
    out = fe(torch.full_like(wave, float("nan")).index_copy_(0, torch.tensor([2], device=DEV), wave[:1]), lens)
    assert out["melspec_lens"].tolist() == [0, 0, 3, 0]
    assert not bool(torch.isnan(out["melspec"]).any())
    assert bool((out["melspec"][[0, 1, 3]] == 0).all()) and bool((out["melspec"][2, 3:] == 0).all())
    assert torch.equal(out["melspec"][2, :3], fe(wave, torch.tensor(case["lens"], device=DEV))["melspec"][0, :3])
    with pytest.raises(ValueError, match="cannot be reflected"):       # host lengths: refused before any launch
        fe(wave, torch.tensor([256, 300, 257, 4000]))
    with pytest.raises(ValueError, match="wave must be \\(B, Nmax\\)"):
        fe(wave[0], lens)
    with pytest.raises(ValueError, match="expected a CUDA/HIP tensor"):
        fe(wave.cpu(), lens)
    with pytest.raises(ValueError, match="wave_lens must have shape"):
        fe(wave, lens[:3])
    with pytest.raises(ValueError, match="n_fft must be one of"):
        MelFrontEnd(dict(CONFIG_B, n_fft=768), device=DEV)
    with pytest.raises(ValueError, match="hop_length must be in"):
        MelFrontEnd(dict(CONFIG_B, hop_length=513), device=DEV)
    with pytest.raises(ValueError, match="win_length must be in"):
        MelFrontEnd(dict(CONFIG_B, win_length=513), device=DEV)


def test_the_front_end_feeds_the_tiny_model():
    from oracle import fill_state
    from transformertts_amd.audio import MelFrontEnd
    from transformertts_amd.model import TransformerTTS
    from transformertts_amd.workload import model_config
    mcfg = model_config("tiny")
    cfg = dict(CONFIG_B, n_mels=mcfg["n_mels"])
    case = _case("B")
    fe = MelFrontEnd(cfg, device=DEV)
    wave, lens = _device_batch(case)
    raw = fe(wave, lens)
    fe.set_stats(*fe.mean_std_from(*fe.stats(raw["melspec"], raw["melspec_lens"])))
    batch = fe(wave, lens)
    assert set(batch) == {"melspec", "melspec_lens"}                   # the keys DeviceStager hands the model
    assert tuple(batch["melspec"].shape) == (4, 1 + wave.size(1) // 128, mcfg["n_mels"]) and batch["melspec"].is_contiguous()
    m = TransformerTTS(**mcfg, device="cuda")
    m.load_state_dict(fill_state(mcfg, 3), strict=True)
    m = m.to(DEV).eval()
    g = torch.Generator().manual_seed(5)
    plens = torch.tensor([9, 7, 6, 4])
    phon = torch.zeros(4, 9, dtype=torch.long)
    for b, p in enumerate(plens.tolist()):
        phon[b, :p] = torch.randint(1, mcfg["n_phon"], (p,), generator=g)
    with torch.no_grad():
        out = m(phon.to(DEV), batch["melspec"], plens.to(DEV), batch["melspec_lens"])
    assert tuple(out["post_melspec"].shape) == tuple(batch["melspec"].shape)
    assert bool(torch.isfinite(out["post_melspec"]).all())
