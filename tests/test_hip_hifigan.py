"""The HiFi-GAN generator on the device (csrc/hifigan.hip through transformertts_amd/hifigan.py) against the references of
tests/hifigan_reference.py.  The dilated convolution is held to the project's kernel bound (TOL of tests/test_hip_modes.py under
conftest.rel_l2: its products are exact fp32 MFMA, as the FFT sublayer's are), conv_post + tanh to the same bound; the whole
generator to twice the error of the stock-torch fp32 restatement from the same `state_dict` against the same fp64 per-utterance
reference, and to 1e-4 (the rule of `_held_to_stock` in tests/test_hip_fft.py; the stock fp32 restatement runs on the CPU).  NaN
sits behind every length of every input throughout.  The shapes are the smallest that reach every path: one row, row-tile joins
crossed with an empty utterance, an utterance shorter than the halo, every tap count crossed with the dilations, more than one
workgroup of rows at each of the four wave layouts (Cout 32, 64, 128, >= 256), partial column blocks, 80 mels into 512 columns, the
deepest reduction (11 x 512) over every column block, and the upsamplers through `transposed_as_conv`.
Measured values: parity_reports/hifigan_margin.txt (as measured on one MI355X: tests/reports/hifigan_margin.txt)."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from hifigan_reference import Generator, dilated_conv_ref, fan_in_state, generate_per_utterance, poison
from test_hip_dropout_parity import REPORT_DIR
from test_hip_modes import TOL
from transformertts_amd import _lib as _library
from transformertts_amd import hifigan as hg
from transformertts_amd.hifigan import (HiFiGANConfig, HiFiGANGenerator, fold_weight_norm, ragged_dilated_conv,  # noqa: F401 -- no feature, no tests
                                        transposed_as_conv)

_library.load()                                                       # raises when the library lacks the entries

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# name -> B, Nmax, Cin, Cout, taps, dilation, lens
CASES = {
    "one_row": (1, 1, 32, 32, 1, 1, (1,)),
    "tile_joins_empty": (4, 33, 32, 32, 3, 1, (31, 32, 33, 0)),
    "shorter_than_halo": (2, 40, 32, 32, 7, 12, (3, 40)),
    "two_blocks_c32": (1, 300, 32, 32, 3, 5, (290,)),                 # Cout 32: a workgroup owns 256 rows, a wave 64 x 32
    "two_blocks_c64": (2, 300, 64, 64, 5, 3, (300, 259)),             # Cout 64: 256 rows, a wave 64 x 64
    "two_blocks_c128": (2, 140, 32, 128, 3, 3, (140, 129)),           # Cout 128: 128 rows
    "two_blocks_c256": (2, 70, 32, 256, 3, 3, (70, 65)),              # Cout >= 256: 64 rows
    "partial_column_block": (1, 20, 32, 96, 3, 1, (20,)),             # the second block of 64 columns holds 32
    "idle_wave": (1, 20, 32, 192, 3, 1, (20,)),                       # the second block of 128 columns holds 64: a wave without columns
    "conv_pre": (2, 40, 80, 512, 7, 1, (40, 9)),
    "deepest": (2, 40, 512, 512, 11, 1, (40, 17)),
}
CASES.update({f"k{k}_d{d}": (2, 100, 32, 32, k, d, (100, 67)) for k in (3, 5, 7, 11) for d in (1, 3, 5, 12)})

TINY1 = dict(resblock="1", upsample_rates=(2, 2), upsample_kernel_sizes=(4, 4), upsample_initial_channel=128,
             resblock_kernel_sizes=(3, 5), resblock_dilation_sizes=((1, 3, 5), (1, 3, 5)), n_mels=8)
TINY2 = dict(TINY1, resblock="2", resblock_dilation_sizes=((1, 2), (2, 6)))
# name -> config, lens, conv_post gain (chosen on the CPU so that the fp64 output spreads over (-1, 1): see `_generator_case`)
GENERATORS = {
    "tiny1": (lambda: HiFiGANConfig(**TINY1), (9, 4, 0), 2.0),
    "tiny2": (lambda: HiFiGANConfig(**TINY2), (9, 4, 0), 2.0),
    "v1": (HiFiGANConfig.v1, (8, 5), 2.0),
    "v3": (HiFiGANConfig.v3, (8, 5), 2.0),
}


def _report(line):
    print(line)
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(f"{REPORT_DIR}/hifigan_margin.txt", "a") as f:
        f.write(line + "\n")


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _behind_are_zero(t, lens, per=1):
    return all(bool((t[b, max(int(n), 0) * per:] == 0).all()) for b, n in enumerate(lens))


@functools.lru_cache(maxsize=None)
def _case(name):
    """fp32 operands with NaN behind every length of x and of the residual (computed once, never modified)"""
    B, N, cin, cout, taps, dil, lens = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    x = rng.standard_normal((B, N, cin)).astype(np.float32)
    w = (rng.standard_normal((cout, cin, taps)) / np.sqrt(cin * taps)).astype(np.float32)
    bias = (0.3 * rng.standard_normal(cout)).astype(np.float32)
    res = rng.standard_normal((B, N, cout)).astype(np.float32)
    x, res = poison(lens, x, res)
    return dict(x=x, w=w, bias=bias, res=res, lens=np.array(lens, np.int64))


# ------------------------------------------------------------------------------------------------ the convolution
@pytest.mark.parametrize("name", list(CASES))
def test_the_dilated_convolution_against_fp64(name):
    B, N, cin, cout, taps, dil, lens = CASES[name]
    c = _case(name)
    x, w, bias, res, pl = _dev(c["x"]), _dev(c["w"]), _dev(c["bias"]), _dev(c["res"]), _dev(c["lens"])
    errs = {}
    # prologue, bias and residual, each on and off
    for tag, kw in (("plain", {}), ("bias", dict(bias=True)), ("lrelu", dict(in_slope=0.1)),
                    ("all", dict(bias=True, in_slope=0.1, residual=True))):
        y = ragged_dilated_conv(x, pl, w, bias if kw.get("bias") else None, dilation=dil, in_slope=kw.get("in_slope"),
                                residual=res if kw.get("residual") else None)
        ref = dilated_conv_ref(c["x"], lens, c["w"], c["bias"] if kw.get("bias") else None, dil, kw.get("in_slope"),
                               c["res"] if kw.get("residual") else None)
        assert y.shape == (B, N, cout) and not bool(torch.isnan(y).any()), tag      # nothing behind a length was used
        assert _behind_are_zero(y, lens), tag
        errs[tag] = rel_l2(y, ref)
        if tag == "all":
            again = ragged_dilated_conv(x, pl, w, bias, dilation=dil, in_slope=0.1, residual=res)
            assert _same_bits(again, y)                                             # the same bits on every call
            b = int(np.argmax(c["lens"]))                                           # an utterance alone: its bits in the batch
            n = int(c["lens"][b])
            alone = ragged_dilated_conv(x[b:b + 1, :n].contiguous(), pl[b:b + 1], w, bias, dilation=dil, in_slope=0.1,
                                        residual=res[b:b + 1, :n].contiguous())
            assert _same_bits(alone, y[b:b + 1, :n])
    _report(f"conv {name}: " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert all(v < TOL for v in errs.values()), errs


def test_the_accumulate_and_scale_epilogue():
    name = "two_blocks_c64"
    B, N, cin, cout, taps, dil, lens = CASES[name]
    c = _case(name)
    x, bias, res, pl = _dev(c["x"]), _dev(c["bias"]), _dev(c["res"]), _dev(c["lens"])
    w = hg._relaid(_dev(c["w"]))
    ref = dilated_conv_ref(c["x"], lens, c["w"], c["bias"], dil, 0.1, c["res"])
    y = ragged_dilated_conv(x, pl, _dev(c["w"]), bias, dilation=dil, in_slope=0.1, residual=res)
    nan = float("nan")
    acc = torch.full((B, N, cout), nan, device=DEV)
    y1 = torch.full((B, N, cout), nan, device=DEV)
    hg._conv(x, pl, w, bias, res, y1, acc, taps, dil, 0.1, 1, 1.0)                  # set: acc = v; y written too
    torch.cuda.synchronize()
    assert _same_bits(y1, y) and _same_bits(acc, y)
    hg._conv(x, pl, w, bias, res, None, acc, taps, dil, 0.1, 2, 1.0)                # add, y not wanted: acc = acc + v
    hg._conv(x, pl, w, bias, res, None, acc, taps, dil, 0.1, 2, 1.0 / 3.0)          # the last block carries 1 / n_blocks
    torch.cuda.synchronize()
    want = ((y + y) + y) * np.float32(1.0 / 3.0)                                    # fp32, in this order: bit for bit
    assert _same_bits(acc, want)
    assert not bool(torch.isnan(acc).any()) and _behind_are_zero(acc, lens)
    err = rel_l2(acc, ref)
    _report(f"conv {name}: mean of three through the accumulate epilogue {err:.3e}")
    assert err < TOL
    half = torch.full((B, N, cout), nan, device=DEV)
    hg._conv(x, pl, w, bias, res, None, half, taps, dil, 0.1, 1, 0.5)               # set with a scale
    torch.cuda.synchronize()
    assert _same_bits(half, y * 0.5)


def test_the_entries_refuse_bad_arguments_by_name():
    x, pl = torch.zeros(1, 8, 32, device=DEV), torch.tensor([8], device=DEV)
    with pytest.raises(ValueError, match="taps must be odd"):
        ragged_dilated_conv(x, pl, torch.zeros(32, 32, 4, device=DEV))
    with pytest.raises(ValueError, match="taps must be odd"):
        ragged_dilated_conv(x, pl, torch.zeros(32, 32, 13, device=DEV))
    with pytest.raises(ValueError, match="dilation"):
        ragged_dilated_conv(x, pl, torch.zeros(32, 32, 3, device=DEV), dilation=13)
    with pytest.raises(ValueError, match="Cout"):
        ragged_dilated_conv(x, pl, torch.zeros(48, 32, 3, device=DEV))
    with pytest.raises(ValueError, match="Cin"):
        ragged_dilated_conv(torch.zeros(1, 8, 136, device=DEV), pl, torch.zeros(32, 136, 3, device=DEV))
    with pytest.raises(ValueError, match="requires grad"):
        ragged_dilated_conv(x.clone().requires_grad_(True), pl, torch.zeros(32, 32, 3, device=DEV))
    from ctypes import c_void_p
    lib = _library.load()
    w, y = torch.zeros(3, 32, 32, device=DEV), torch.zeros(1, 8, 32, device=DEV)
    p = lambda t: c_void_p(t.data_ptr())
    for args, word in (((1, 8, 32, 32, 4, 1), "taps"), ((1, 8, 32, 32, 3, 0), "dilation"), ((1, 8, 32, 16, 3, 1), "Cout"),
                       ((1, 8, 544, 32, 3, 1), "Cin"), ((1, 8, 132, 32, 3, 1), "Cin"), ((1, 1 << 22, 32, 32, 3, 1), "Nmax"),
                       ((65535, 1 << 15, 32, 32, 3, 1), "split the batch")):     # (each is refused before any launch)
        rc = lib.ttts_hifigan_conv(p(x), p(pl), p(w), None, None, p(y), None, *args, 1.0, 0, 1.0, None)
        assert rc != 0 and word in _library.last_error(), (args, _library.last_error())
    rc = lib.ttts_hifigan_conv(p(x), p(pl), p(w), None, None, c_void_p(y.data_ptr() + 4), None, 1, 8, 32, 32, 3, 1, 1.0, 0, 1.0, None)
    assert rc != 0 and "aligned" in _library.last_error()
    rc = lib.ttts_hifigan_conv(p(x), p(pl), p(w), None, None, p(y), p(y), 1, 8, 32, 32, 3, 1, 1.0, 0, 1.0, None)
    assert rc != 0 and "acc_mode" in _library.last_error()
    rc = lib.ttts_hifigan_post(p(x), p(pl), p(w), p(w), p(y), 1, 8, 48, 7, 0.01, None)
    assert rc != 0 and "Cin" in _library.last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("k,u", [(16, 8), (4, 2), (8, 4)])
def test_the_upsampler_through_transposed_as_conv(k, u):
    cin, cout, B, T, lens = 64, 32, 3, 37, (37, 5, 0)
    rng = np.random.default_rng(k * 31 + u)
    x = poison(lens, rng.standard_normal((B, T, cin)).astype(np.float32))
    w = (rng.standard_normal((cin, cout, k)) / np.sqrt(cin * k / u)).astype(np.float32)
    bias = (0.3 * rng.standard_normal(cout)).astype(np.float32)
    W = transposed_as_conv(torch.from_numpy(w), u)
    y = ragged_dilated_conv(_dev(x), torch.tensor(lens, device=DEV), W.to(DEV), torch.from_numpy(bias).repeat(u).to(DEV), in_slope=0.1)
    y = y.view(B, T * u, cout)                                                       # (B, T, u C) row-major is (B, T u, C) row-major
    ref = torch.zeros(B, T * u, cout, dtype=torch.float64)
    for b, n in enumerate(lens):
        if n > 0:
            xb = F.leaky_relu(torch.from_numpy(x[b, :n]).double(), 0.1).t()[None]
            ref[b, :n * u] = F.conv_transpose1d(xb, torch.from_numpy(w).double(), torch.from_numpy(bias).double(), stride=u,
                                                padding=(k - u) // 2)[0].t()
    assert not bool(torch.isnan(y).any()) and _behind_are_zero(y, lens, u)
    err = rel_l2(y, ref)
    _report(f"upsampler k {k} u {u}: {err:.3e}")
    assert err < TOL


def test_conv_post_and_tanh_where_the_argument_reaches_ten():
    from transformertts_amd.ops import _p, _stream
    B, N, cin, lens = 3, 300, 32, (300, 257, 0)
    rng = np.random.default_rng(11)
    x = poison(lens, rng.standard_normal((B, N, cin)).astype(np.float32))
    w = (rng.standard_normal((1, cin, 7)) / np.sqrt(cin * 7)).astype(np.float32)
    bias = np.array([0.1], np.float32)
    pre = dilated_conv_ref(x, lens, w, bias, 1, 0.01)[:, :, 0]
    gain = np.float32(10.0 / float(pre.abs().max()))                                 # |pre-tanh| reaches 10
    w, bias = (w * gain).astype(np.float32), (bias * gain).astype(np.float32)
    pre = dilated_conv_ref(x, lens, w, bias, 1, 0.01)[:, :, 0]
    assert 9.9 < float(pre.abs().max()) < 10.1 and float((pre.abs() < 1).double().mean()) > 0.1
    valid = torch.arange(N)[None, :] < torch.tensor(lens)[:, None]
    ref = torch.where(valid, torch.tanh(pre), torch.zeros((), dtype=torch.float64))
    y = torch.full((B, N), float("nan"), device=DEV)
    xd, pl = _dev(x), torch.tensor(lens, device=DEV)
    wd, bd = hg._relaid(_dev(w)), _dev(bias)
    _library.check(_library.load().ttts_hifigan_post(_p(xd), _p(pl), _p(wd), _p(bd), _p(y), B, N, cin, 7, 0.01, _stream()), "post")
    torch.cuda.synchronize()
    assert not bool(torch.isnan(y).any()) and _behind_are_zero(y, lens)
    err = rel_l2(y, ref)
    worst = float((y.cpu().double() - ref).abs().max())
    _report(f"conv_post + tanh: rel-L2 {err:.3e} largest difference {worst:.3e} (|pre-tanh| up to {float(pre.abs().max()):.2f})")
    assert err < TOL and float(y.abs().max()) <= 1.0


# ------------------------------------------------------------------------------------------------ the generator
@functools.lru_cache(maxsize=None)
def _generator_case(name):
    """state dict (fan-in scaled), a poisoned mel batch, the fp64 per-utterance reference and the stock fp32 restatement's output
    (both on the CPU, computed once).  conv_post's gain makes the reference's output spread over (-1, 1) without being pinned at
    the ends: asserted here."""
    make, lens, gain = GENERATORS[name]
    cfg = make()
    sd = fan_in_state(cfg, sum(map(ord, name)), post_gain=gain)
    B, T = len(lens), max(lens)
    rng = np.random.default_rng(sum(map(ord, name)) + 1)
    mel = poison(lens, rng.standard_normal((B, T, cfg.n_mels)).astype(np.float32))
    out = {}
    for tag, dtype in (("ref", torch.float64), ("stock", torch.float32)):
        m = Generator(cfg).to(dtype)
        m.load_state_dict({k: v.to(dtype) for k, v in sd.items()})
        out[tag] = generate_per_utterance(m, torch.from_numpy(mel).to(dtype), lens, cfg.hop)
    live = torch.cat([out["ref"][b, :n * cfg.hop] for b, n in enumerate(lens)])
    spread = dict(std=float(live.std()), peak=float(live.abs().max()), pinned=float((live.abs() > 0.99).double().mean()))
    assert spread["std"] > 0.2 and spread["peak"] > 0.7 and spread["pinned"] < 0.05, (name, spread)
    return dict(cfg=cfg, sd=sd, mel=mel, lens=lens, ref=out["ref"], stock=out["stock"], spread=spread)


def _held_to_stock(tag, kernel, stock, ref):
    """the rule of tests/test_hip_fft.py: below twice the stock fp32 path's error against the same fp64, and below 1e-4"""
    e, e32 = rel_l2(kernel, ref), rel_l2(stock, ref)
    _report(f"{tag}: kernels {e:.3e} stock fp32 {e32:.3e}")
    assert e < 2.0 * e32 and e < 1e-4, (e, e32)


def _gen(name, sd=None, **kw):
    c = _generator_case(name)
    return HiFiGANGenerator(c["cfg"], c["sd"] if sd is None else sd, device=DEV, **kw)


@pytest.mark.parametrize("name", list(GENERATORS))
def test_the_generator_against_fp64_and_the_stock_fp32_path(name):
    c = _generator_case(name)
    gen = _gen(name)
    out = gen(_dev(c["mel"]), torch.tensor(c["lens"], device=DEV))
    torch.cuda.synchronize()
    wave, hop = out["wave"], c["cfg"].hop
    assert wave.shape == (len(c["lens"]), max(c["lens"]) * hop) and wave.dtype == torch.float32
    assert out["wave_lens"].tolist() == [n * hop for n in c["lens"]]
    assert not bool(torch.isnan(wave).any()) and _behind_are_zero(wave, c["lens"], hop)
    _report(f"generator {name}: reference spread " + " ".join(f"{k} {v:.3f}" for k, v in c["spread"].items()))
    _held_to_stock(f"generator {name}", wave, c["stock"], c["ref"])


def test_an_utterance_alone_and_a_second_call_have_the_same_bits():
    c = _generator_case("tiny1")
    gen = _gen("tiny1")
    mel, pl = _dev(c["mel"]), torch.tensor(c["lens"], device=DEV)
    wave = gen(mel, pl)["wave"]
    assert _same_bits(gen(mel, pl)["wave"], wave)
    hop = c["cfg"].hop
    for b, n in enumerate(c["lens"]):
        if n > 0:
            alone = gen(mel[b:b + 1, :n].contiguous(), pl[b:b + 1])["wave"]
            assert _same_bits(alone, wave[b:b + 1, :n * hop]), b
    long = gen(mel, pl + 100)                                                        # lengths are clamped to Tmax
    assert long["wave_lens"].tolist() == [max(c["lens"]) * hop] * len(c["lens"])


def test_a_captured_call_replays_to_the_eager_bits():
    c = _generator_case("tiny2")
    gen = _gen("tiny2")
    mels = [_dev(c["mel"]), _dev(poison(c["lens"], np.random.default_rng(3).standard_normal(c["mel"].shape).astype(np.float32)))]
    static, pl = mels[0].clone(), torch.tensor(c["lens"], device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                    # (warm-up: the library is loaded, the allocator primed)
        gen(static, pl)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = gen(static, pl)
    seen = []
    for mel in mels:
        static.copy_(mel)
        graph.replay()
        torch.cuda.synchronize()
        eager = gen(mel.clone(), pl)
        assert _same_bits(got["wave"], eager["wave"]) and torch.equal(got["wave_lens"], eager["wave_lens"])
        assert not bool(torch.isnan(got["wave"]).any())
        seen.append(got["wave"].clone())
    assert not torch.equal(seen[0], seen[1])                                         # the replay did follow the input


@pytest.mark.parametrize("spelling", ["weight_g", "parametrizations"])
def test_weight_norm_spellings_give_the_plain_state_dicts_bits(spelling):
    c = _generator_case("tiny1")
    wn = fan_in_state(c["cfg"], 77, post_gain=4.0, spelling=spelling)
    m = Generator(c["cfg"], spelling).double()                                       # torch's own fold, in fp64
    m.load_state_dict({k: v.double() for k, v in wn.items()})
    m(torch.zeros(1, c["cfg"].n_mels, 2, dtype=torch.float64))
    plain = {}
    for prefix, _ in c["cfg"].layer_names():
        mod = m.get_submodule(prefix)
        plain[prefix + ".weight"], plain[prefix + ".bias"] = mod.weight.detach().float(), mod.bias.detach().float()
    mel, pl = _dev(c["mel"]), torch.tensor(c["lens"], device=DEV)
    a = HiFiGANGenerator(c["cfg"], wn, device=DEV)(mel, pl)["wave"]
    b = HiFiGANGenerator(c["cfg"], plain, device=DEV)(mel, pl)["wave"]
    assert _same_bits(a, b) and float(a.abs().max()) > 0.1


def test_mean_and_std_denormalise_the_mel_first():
    c = _generator_case("tiny2")
    rng = np.random.default_rng(4)
    mean = rng.standard_normal(c["cfg"].n_mels).astype(np.float32)
    std = rng.uniform(0.5, 2.0, c["cfg"].n_mels).astype(np.float32)
    mel, pl = _dev(c["mel"]), torch.tensor(c["lens"], device=DEV)
    from transformertts_amd import denormalize
    want = _gen("tiny2")(denormalize(mel, _dev(mean), _dev(std)), pl)["wave"]
    got = _gen("tiny2", mean=mean, std=std)(mel, pl)["wave"]
    assert _same_bits(got, want) and not _same_bits(got, _gen("tiny2")(mel, pl)["wave"])


def test_the_batch_split_gives_the_unsplit_bits():
    c = _generator_case("tiny1")
    gen = _gen("tiny1")
    mel, pl = _dev(c["mel"]), torch.tensor(c["lens"], device=DEV)
    B, T = len(c["lens"]), max(c["lens"])
    whole = gen(mel, pl)["wave"]
    per = gen._widest(T) * 4
    assert gen._part(B, T, None) == B and gen._part(B, T, per) == 1 and gen._part(B, T, 2 * per + 1) == 2
    assert gen.peak_bytes(B, T) == 5 * B * per and gen.peak_bytes(B, T, per) == 5 * per
    for limit in (per, 2 * per + 1):
        assert _same_bits(gen(mel, pl, max_bytes=limit)["wave"], whole), limit
    with pytest.raises(ValueError, match="the limit is"):
        gen(mel, pl, max_bytes=per - 1)
