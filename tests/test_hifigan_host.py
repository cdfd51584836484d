"""CPU checks of the HiFi-GAN generator's host side (transformertts_amd/hifigan.py): the weight-norm fold and the transposed
convolution's re-layout against torch in fp64, the presets' arithmetic, every refusal by name, the C entries' declarations, and the
reference generator of tests/hifigan_reference.py on a batch against itself on each utterance alone."""
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from hifigan_reference import Generator, dilated_conv_ref, fan_in_state, generate_per_utterance
from transformertts_amd.hifigan import HiFiGANConfig, HiFiGANGenerator, fold_weight_norm, transposed_as_conv

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(16, 8), (8, 4), (4, 2), (9, 5), (6, 4), (3, 3), (2, 2)]
TINY1 = dict(resblock="1", upsample_rates=(2, 2), upsample_kernel_sizes=(4, 4), upsample_initial_channel=128,
             resblock_kernel_sizes=(3, 5), resblock_dilation_sizes=((1, 3, 5), (1, 3, 5)), n_mels=8)
TINY2 = dict(TINY1, resblock="2", resblock_dilation_sizes=((1, 2), (2, 6)))


def test_the_entries_are_declared_once_and_bound():
    from transformertts_amd import _lib
    from transformertts_amd._lib import F as CF, I, P
    hdr = open(os.path.join(REPO, "include", "ttts_hip.h")).read()
    lib = _lib.load()
    for name in ("ttts_hifigan_max_operand_bytes", "ttts_hifigan_conv", "ttts_hifigan_post"):
        decls = re.findall(r"^(?:int|size_t) " + name + r"\(([^;]*)\);", hdr, re.M)
        assert len(decls) == 1, f"{name} must be declared exactly once in ttts_hip.h, found {len(decls)}"
        assert name in _lib.SIGNATURES and hasattr(lib, name), f"{name} is not exported / bound"
        n_args = 0 if decls[0].strip() == "void" else len(decls[0].split(","))
        assert n_args == len(_lib.SIGNATURES[name][1]), name
    assert _lib.SIGNATURES["ttts_hifigan_conv"] == (I, [P, P, P, P, P, P, P, I, I, I, I, I, I, CF, I, CF, P])
    assert _lib.SIGNATURES["ttts_hifigan_post"] == (I, [P, P, P, P, P, I, I, I, I, CF, P])
    assert lib.ttts_abi_version() == 24                                # additive: the version stays
    assert 0 < lib.ttts_hifigan_max_operand_bytes() < 1 << 32          # operands of 4 GiB or more are refused


@pytest.mark.parametrize("kind", ["conv", "transposed"])
@pytest.mark.parametrize("spelling", ["plain", "weight_g", "parametrizations"])
def test_fold_weight_norm_against_torchs_own_modules(kind, spelling):
    torch.manual_seed(3)
    layer = (nn.Conv1d(12, 20, 5) if kind == "conv" else nn.ConvTranspose1d(12, 20, 4, 2, padding=1)).double()
    if spelling == "weight_g":
        layer = torch.nn.utils.weight_norm(layer)
    elif spelling == "parametrizations":
        layer = torch.nn.utils.parametrizations.weight_norm(layer)
    with torch.no_grad():
        for p in layer.parameters():
            p.mul_(1 + 0.5 * torch.rand_like(p))                        # g is no longer ||v||: the fold is not the identity
    sd = {"l." + k: v for k, v in layer.state_dict().items()}
    if spelling != "plain":
        assert "l.weight" not in sd and len(sd) == 3
    folded = fold_weight_norm(sd)
    assert set(folded) == {"l.weight", "l.bias"}
    assert folded["l.weight"].dtype == torch.float64
    layer(torch.zeros(1, 12, 8, dtype=torch.float64))                   # (the hook form recomputes its weight in a forward)
    want = layer.weight.detach()
    assert float((folded["l.weight"] - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert torch.equal(folded["l.bias"], layer.bias.detach())
    if spelling != "plain":                                             # fp32 in, fp32 out; the arithmetic still in fp64
        f32 = fold_weight_norm({k: v.float() for k, v in sd.items()})
        assert f32["l.weight"].dtype == torch.float32
        assert float((f32["l.weight"].double() - want).abs().max()) <= 3e-7 * float(want.abs().max())


def test_fold_weight_norm_names_a_missing_partner():
    with pytest.raises(KeyError, match="ups.0.weight_v"):
        fold_weight_norm({"ups.0.weight_g": torch.ones(4, 1, 1), "ups.0.bias": torch.zeros(4)})
    with pytest.raises(KeyError, match="original0"):
        fold_weight_norm({"a.parametrizations.weight.original1": torch.ones(4, 2, 3)})


@pytest.mark.parametrize("k,u", PAIRS)
def test_transposed_as_conv_against_conv_transpose1d(k, u):
    torch.manual_seed(k * 31 + u)
    cin, cout, T = 6, 5, 9
    w = torch.randn(cin, cout, k, dtype=torch.float64)
    bias = torch.randn(cout, dtype=torch.float64)
    x = torch.randn(2, cin, T, dtype=torch.float64)
    want = F.conv_transpose1d(x, w, bias, stride=u, padding=(k - u) // 2)                   # (2, cout, T u)
    W = transposed_as_conv(w, u)
    assert W.shape == (u * cout, cin, 3) and W.dtype == torch.float64
    got = F.conv1d(x, W, bias.repeat(u), padding=1)                                          # (2, u cout, T)
    got = got.transpose(1, 2).reshape(2, T * u, cout).transpose(1, 2)                        # (B, T, u C) read as (B, T u, C)
    assert want.shape == got.shape
    assert float((got - want).abs().max()) <= 1e-12
    zeros = int((W == 0).sum())
    assert zeros == (3 * u - k) * cin * cout                                                 # the structural zeros: 3 u - k taps


def test_the_presets_channels_and_hop():
    v1, v3 = HiFiGANConfig.v1(), HiFiGANConfig.v3()
    assert v1.hop == 256 and v1.channels == (512, 256, 128, 64, 32) and v1.resblock == "1"
    assert v3.hop == 256 and v3.channels == (256, 128, 64, 32) and v3.resblock == "2"
    assert v1.n_mels == v3.n_mels == 80
    names = [n for n, _ in v1.layer_names()]
    assert names[0] == "conv_pre" and names[-1] == "conv_post" and len(names) == 2 + 4 + 4 * 3 * 3 * 2
    assert "resblocks.11.convs2.2" in names and "ups.3" in names
    names3 = [n for n, _ in v3.layer_names()]
    assert len(names3) == 2 + 3 + 3 * 3 * 2 and "resblocks.8.convs.1" in names3
    ref = Generator(v3)                                                                      # the reference carries the same keys
    assert {k.rsplit(".", 1)[0] for k in ref.state_dict()} == set(names3)
    tiny = HiFiGANConfig(**TINY1)
    assert tiny.hop == 4 and tiny.channels == (128, 64, 32)


def test_from_json_reads_the_usual_keys(tmp_path):
    c = dict(resblock="2", upsample_rates=[8, 8, 4], upsample_kernel_sizes=[16, 16, 8], upsample_initial_channel=256,
             resblock_kernel_sizes=[3, 5, 7], resblock_dilation_sizes=[[1, 2], [2, 6], [3, 12]], num_mels=80, sampling_rate=22050)
    p = tmp_path / "config.json"
    p.write_text(json.dumps(c))
    assert HiFiGANConfig.from_json(str(p)) == HiFiGANConfig.v3()
    del c["upsample_rates"]
    p.write_text(json.dumps(c))
    with pytest.raises(ValueError, match="upsample_rates"):
        HiFiGANConfig.from_json(str(p))


def test_every_refusal_is_named():
    with pytest.raises(ValueError, match="V2"):
        HiFiGANConfig.v2()
    with pytest.raises(ValueError, match="V2"):                         # V2's numbers through the constructor
        HiFiGANConfig("1", (8, 8, 2, 2), (16, 16, 4, 4), 128, (3, 7, 11), ((1, 3, 5),) * 3, 80)
    with pytest.raises(ValueError, match="resblock_kernel_sizes must be odd"):
        HiFiGANConfig(**dict(TINY1, resblock_kernel_sizes=(3, 4)))
    with pytest.raises(ValueError, match="resblock_kernel_sizes must be odd"):
        HiFiGANConfig(**dict(TINY1, resblock_kernel_sizes=(3, 13)))
    with pytest.raises(ValueError, match="must be even"):
        HiFiGANConfig(**dict(TINY1, upsample_kernel_sizes=(3, 4)))
    with pytest.raises(ValueError, match=r"\[stride, 2 stride\]"):
        HiFiGANConfig(**dict(TINY1, upsample_kernel_sizes=(6, 4)))
    with pytest.raises(ValueError, match=r"\[stride, 2 stride\]"):
        transposed_as_conv(torch.zeros(4, 4, 1), 2)
    with pytest.raises(ValueError, match="must be even"):
        transposed_as_conv(torch.zeros(4, 4, 5), 4)
    with pytest.raises(ValueError, match="resblock must be"):
        HiFiGANConfig(**dict(TINY1, resblock="3"))
    with pytest.raises(ValueError, match="resblock_dilation_sizes must be in"):
        HiFiGANConfig(**dict(TINY1, resblock_dilation_sizes=((1, 3, 13), (1, 3, 5))))
    with pytest.raises(ValueError, match="one entry per stage"):
        HiFiGANConfig(**dict(TINY1, upsample_kernel_sizes=(4,)))
    with pytest.raises(ValueError, match="one entry per resblock kernel size"):
        HiFiGANConfig(**dict(TINY1, resblock_dilation_sizes=((1, 3, 5),)))
    with pytest.raises(ValueError, match="n_mels"):
        HiFiGANConfig(**dict(TINY1, n_mels=6))
    cfg = HiFiGANConfig(**TINY1)
    sd = fan_in_state(cfg, 1)
    with pytest.raises(ValueError, match="CUDA/HIP device"):
        HiFiGANGenerator(cfg, sd, device="cpu")
    # a missing key is named before anything reaches the device (the device is not touched by the check itself)
    del sd["resblocks.2.convs1.1.bias"]
    with pytest.raises(KeyError, match=r"resblocks\.2\.convs1\.1\.bias"):
        HiFiGANGenerator(cfg, sd, device="cuda")


@pytest.mark.parametrize("cfg", [TINY1, TINY2], ids=["type1", "type2"])
def test_the_reference_on_a_batch_is_itself_on_each_utterance_alone(cfg):
    cfg = HiFiGANConfig(**cfg)
    model = Generator(cfg).double()
    model.load_state_dict({k: v.double() for k, v in fan_in_state(cfg, 5, post_gain=4.0).items()})
    torch.manual_seed(7)
    mel = torch.randn(3, 9, cfg.n_mels, dtype=torch.float64)
    with torch.no_grad():
        full = model(mel.transpose(1, 2))                               # equal lengths: the batch needs no padding
    assert full.shape == (3, 9 * cfg.hop)
    assert float((generate_per_utterance(model, mel, (9, 9, 9), cfg.hop) - full).abs().max()) <= 1e-12
    lens = (9, 4, 0)
    poisoned = mel.clone()
    for b, n in enumerate(lens):
        poisoned[b, n:] = float("nan")
    wave = generate_per_utterance(model, poisoned, lens, cfg.hop)
    assert not bool(torch.isnan(wave).any())
    with torch.no_grad():
        alone = model(mel[1:2, :4].transpose(1, 2))
    assert torch.equal(wave[1, :4 * cfg.hop], alone[0]) and bool((wave[1, 4 * cfg.hop:] == 0).all()) and bool((wave[2] == 0).all())
    # a padded batch is NOT this: the padding's bias leaks into the utterance's end
    with torch.no_grad():
        padded = model(torch.nan_to_num(poisoned).transpose(1, 2))
    assert float((padded[1, :4 * cfg.hop] - alone[0]).abs().max()) > 1e-6
    # the fp32 weight-norm spellings load into the reference and fold to the plain weights
    for spelling in ("weight_g", "parametrizations"):
        wn = fan_in_state(cfg, 5, post_gain=4.0, spelling=spelling)
        m2 = Generator(cfg, spelling)
        m2.load_state_dict(wn, strict=True)
        plain, folded = fan_in_state(cfg, 5, post_gain=4.0), fold_weight_norm(wn)
        assert set(folded) == set(plain)
        assert all(float((folded[k] - plain[k]).abs().max()) <= 3e-7 * float(plain[k].abs().max()) for k in plain)


def test_dilated_conv_ref_is_conv1d_on_each_utterance():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((2, 10, 8))
    w = rng.standard_normal((6, 8, 3))
    bias = rng.standard_normal(6)
    res = rng.standard_normal((2, 10, 6))
    got = dilated_conv_ref(x, (10, 3), w, bias, dilation=5, in_slope=0.1, residual=res)
    xt = F.leaky_relu(torch.from_numpy(x), 0.1)
    want = F.conv1d(xt[:1].transpose(1, 2), torch.from_numpy(w), torch.from_numpy(bias), dilation=5, padding=5).transpose(1, 2) + torch.from_numpy(res[:1])
    assert float((got[:1] - want).abs().max()) <= 1e-12
    assert bool((got[1, 3:] == 0).all()) and float(got[1, :3].abs().min()) > 0


def test_vocode_mel_takes_a_hifigan_checkpoint(tmp_path):
    import sys
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import vocode_mel as tool
    finally:
        sys.path.pop(0)
    from transformertts_amd.audio import read_wav
    cfg = HiFiGANConfig(**TINY2)
    model = Generator(cfg)
    model.load_state_dict(fan_in_state(cfg, 9, post_gain=2.0))

    class OracleGenerator:
        """HiFiGANGenerator's surface on the reference, on the CPU"""

        def __init__(self, mean, std):
            self.config, self.hop, self.device, self.mean, self.std = cfg, cfg.hop, torch.device("cpu"), mean, std

        def __call__(self, mel, lens):
            if self.mean is not None:
                mel = mel * (self.std + 1e-8) + self.mean
            return {"wave": generate_per_utterance(model, mel, lens.tolist(), cfg.hop), "wave_lens": lens * cfg.hop}

    made = []

    def make(ckpt, config_json, mean=None, std=None):
        made.append((ckpt, config_json, mean, std))
        return OracleGenerator(mean, std)

    audio = dict(sample_rate=22050, n_fft=16, hop_length=cfg.hop, win_length=16, n_mels=cfg.n_mels, normalize_mel=True)
    npz, stats, out = tmp_path / "a.npz", tmp_path / "stats.json", tmp_path / "a.wav"
    mel = np.random.default_rng(1).standard_normal((cfg.n_mels, 3)).astype(np.float32)      # 3 frames: too few for Griffin-Lim
    np.savez(str(npz), melspec=mel)
    stats.write_text('{"mean": -5.0, "std": 2.0}')
    n = tool.run({"audio": audio}, str(npz), str(out), stats_path=str(stats), hifigan="g.pt", hifigan_config="c.json", make_hifigan=make,
                 log=lambda s: None)
    assert made == [("g.pt", "c.json", -5.0, 2.0)]
    y = read_wav(str(out), 22050)
    assert n == y.size == 3 * cfg.hop and np.abs(y).max() > 0.01
    with pytest.raises(ValueError, match="go together"):
        tool.run({"audio": audio}, str(npz), str(out), stats_path=str(stats), hifigan="g.pt", make_hifigan=make, log=lambda s: None)
    with pytest.raises(ValueError, match="the audio config has"):
        tool.run({"audio": dict(audio, hop_length=8)}, str(npz), str(out), stats_path=str(stats), hifigan="g.pt", hifigan_config="c.json",
                 make_hifigan=make, log=lambda s: None)
    with pytest.raises(ValueError, match="too few to vocode"):           # without the options: Griffin-Lim's own rule, as before
        tool.run({"audio": audio}, str(npz), str(out), stats_path=str(stats), make_vocoder=lambda *a, **k: None, log=lambda s: None)
    assert "--hifigan-config" in open(os.path.join(REPO, "tools", "vocode_mel.py")).read()
