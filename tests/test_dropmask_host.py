"""Host checks of the dropout-mask restatement (oracle/dropmask.py) and of the mask injection of the fp64 oracle
(oracle.drop_masks).  No GPU: the restatement is pinned to the kernels by tests/test_hip_dropout_parity.py."""
import numpy as np
import pytest
import torch

from oracle import dropmask as dm


def test_masks_are_pure_functions_of_their_arguments():
    a, b = dm.keep_flat(0x1234ABCD5678, 4 * 70001, 0.1), dm.keep_flat(0x1234ABCD5678, 4 * 70001, 0.1)
    assert a.dtype == np.bool_ and a.shape == (4 * 70001,) and np.array_equal(a, b)
    # an index is hashed by its value: a window of the stream is that window of the whole stream (also across a quad boundary)
    assert np.array_equal(dm.keep_flat(0x1234ABCD5678, 1000, 0.1, start=4998), a[4998:5998])
    c, d = dm.keep_attn(77, 2 * 2 * 70, 23, 0.25), dm.keep_attn(77, 2 * 2 * 70, 23, 0.25)
    assert c.shape == (280, 23) and np.array_equal(c, d)
    # a row's decisions do not depend on how many rows or keys are asked for
    assert np.array_equal(dm.keep_attn(77, 300, 40, 0.25)[:280, :23], c)


@pytest.mark.parametrize("other", [0x1234ABCD5679, 0x1234ABCD5678 ^ (1 << 40), 0])
def test_another_seed_is_another_mask(other):
    """also a seed that differs in the HIGH word only (the hash folds both halves of the 64-bit seed)"""
    a, b = dm.keep_flat(0x1234ABCD5678, 200000, 0.5), dm.keep_flat(other, 200000, 0.5)
    assert 0.4 < float((a != b).mean()) < 0.6
    c, d = dm.keep_attn(0x1234ABCD5678, 2000, 100, 0.5), dm.keep_attn(other, 2000, 100, 0.5)
    assert 0.4 < float((c != d).mean()) < 0.6


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("seed", [0x5EED5EED, 0xD1B54A32D192ED03, 7])
def test_drop_rate_is_p(p, seed):
    """over >= 2e5 elements the drop rate is within 0.01 of p (the bound of test_dropout_masks_are_consistent_and_calibrated)"""
    flat = dm.keep_flat(seed, 262144, p)
    assert abs(float((~flat).mean()) - p) < 0.01
    attn = dm.keep_attn(seed, 2 * 4 * 300, 100, p)
    assert attn.size >= 200000 and abs(float((~attn).mean()) - p) < 0.01
    # every element of a quad takes its own decision (the four share one mixed word)
    for e in range(4):
        assert abs(float((~flat[e::4]).mean()) - p) < 0.015


def test_threshold_rounding_and_scale():
    """drop_threshold: round(p * 65536) clamped to [0, 65535] -- p is honoured to 1.5e-5 -- of the float32 p the C ABI receives;
    drop_scale: the float32 quotient the kernels multiply by"""
    assert dm.drop_threshold(0.0) == 0 and dm.drop_threshold(0.5) == 32768 and dm.drop_threshold(0.25) == 16384
    assert dm.drop_threshold(0.1) == 6554 and dm.drop_threshold(1.0) == 65535 and dm.drop_threshold(-0.3) == 0
    assert dm.drop_threshold(0.5 - 0.4 / 65536) == 32768 and dm.drop_threshold(0.5 - 0.6 / 65536) == 32767
    for p in (0.1, 0.25, 0.3, 0.5, 0.123456, 0.9):
        assert abs(dm.drop_threshold(p) / 65536.0 - p) < 1.5e-5
    # the keep test is `16-bit draw >= threshold`: threshold 0 keeps everything, and masks are nested in p
    assert dm.keep_flat(9, 4096, 0.0).all()
    lo, hi = dm.keep_flat(9, 65536, 0.1), dm.keep_flat(9, 65536, 0.5)
    assert not (hi & ~lo).any()
    assert dm.drop_scale(0.5) == 2.0 and dm.drop_scale(0.0) == 1.0
    assert dm.drop_scale(0.1) == float(np.float32(1.0) / (np.float32(1.0) - np.float32(0.1))) != 1.0 / 0.9
    assert abs(dm.drop_scale(0.1) - 1.0 / 0.9) < 2e-7


def test_site_seed_is_the_xor_with_the_step_word():
    assert dm.site_seed(0x1234, None) == 0x1234
    assert dm.site_seed(0x1234, 0) == 0x1234
    assert dm.site_seed(0xFFFF0000FFFF0000, 0xABCDEF0123456789) == 0xFFFF0000FFFF0000 ^ 0xABCDEF0123456789
    assert dm.site_seed(-1, 0) == 0xFFFFFFFFFFFFFFFF            # (seeds travel as unsigned 64-bit)


# ------------------------------------------------------------------------------------------------ mask injection in the oracle
def _tiny_case():
    from oracle import model_config, fill_state, synth_batch
    cfg = model_config("micro")
    batch = synth_batch(2, 7, 11, cfg["n_mels"], cfg["n_phon"], ragged=True, seed=3)
    return cfg, batch, lambda: _state(fill_state(cfg, 5))


def _state(sd):
    for k in list(sd):
        if sd[k].is_floating_point():
            sd[k] = sd[k].double()
            if "running" not in k and k != "pe.pe":
                sd[k].requires_grad_(True)
    return sd


def _run(cfg, batch, sd, **kw):
    from oracle import oracle_forward, oracle_loss
    out = oracle_forward(sd, cfg, batch["phoneme"], batch["melspec"].double(), batch["phoneme_lens"], batch["melspec_lens"],
                         training=True, **kw)
    oracle_loss(out, batch["melspec"].double(), batch["melspec_lens"])["total"].backward()
    return out


def _site_shapes(cfg, B, Tp, Tm):
    d, He, Hd = cfg["d_model"], cfg["encoder_n_head"], cfg["decoder_n_head"]
    shapes = {}
    for i in range(cfg["encoder_prenet_n_layers"]):
        shapes[f"enc_prenet.{i}"] = (B, Tp, cfg["encoder_prenet_out_channel"])
    shapes["enc.pe"] = (B, Tp, d)
    for i in range(cfg["encoder_n_layers"]):
        pre = f"encoder.layers.{i}"
        shapes.update({f"{pre}.attn": (B, He, Tp, Tp), f"{pre}.attn_out": (B, Tp, d), f"{pre}.ffn_h": (B, Tp, cfg["encoder_d_ffn"]),
                       f"{pre}.ffn_out": (B, Tp, d)})
    shapes.update({"dec_prenet.0": (B, Tm, d), "dec_prenet.1": (B, Tm, d), "dec.pe": (B, Tm, d)})
    for i in range(cfg["decoder_n_layers"]):
        pre = f"decoder.layers.{i}"
        shapes.update({f"{pre}.attn": (B, Hd, Tm, Tm), f"{pre}.attn_out": (B, Tm, d), f"{pre}.cross": (B, Hd, Tm, Tp),
                       f"{pre}.cross_out": (B, Tm, d), f"{pre}.ffn_h": (B, Tm, cfg["decoder_d_ffn"]), f"{pre}.ffn_out": (B, Tm, d)})
    n = cfg["postnet_n_layers"]
    for i in range(n):
        shapes[f"postnet.{i}"] = (B, Tm, cfg["n_mels"] if i == n - 1 else d)
    return shapes


def test_all_ones_masks_with_scale_one_are_the_dropout_off_forward():
    """bit for bit: outputs, BatchNorm buffers and every parameter gradient"""
    from oracle import drop_masks, drop_site_names
    cfg, batch, new_state = _tiny_case()
    shapes = _site_shapes(cfg, 2, batch["phoneme"].shape[1], batch["melspec"].shape[1])
    assert list(shapes) == drop_site_names(cfg)
    sd0, sd1 = new_state(), new_state()
    ref = _run(cfg, batch, sd0, dropout=False)
    with drop_masks({k: torch.ones(v, dtype=torch.bool) for k, v in shapes.items()}, scale=1.0) as rec:
        out = _run(cfg, batch, sd1, dropout=True)
    assert rec.used == drop_site_names(cfg)                     # every site drew, once, under its own name
    for k in ("pred_melspec", "post_melspec", "pred_stop"):
        assert torch.equal(out[k], ref[k]), k
    for a, r in zip(out["alignments"], ref["alignments"]):
        assert torch.equal(a, r)
    for k, v in sd0.items():
        assert torch.equal(sd1[k], v), k
        if v.requires_grad:
            assert torch.equal(sd1[k].grad, v.grad), k


def test_a_mask_zeroes_exactly_its_elements():
    """one cross-attention site: the returned (post-dropout) weights are zero exactly where the mask says, the kept ones are the
    undropped weights times float32 1 / (1 - p); a flat site through positional_encoding likewise"""
    from oracle import drop_masks
    from oracle.ref_model import multi_head_attention, positional_encoding
    from oracle import model_config, fill_state
    cfg = model_config("micro")
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in fill_state(cfg, 5).items()}
    g = torch.Generator().manual_seed(1)
    xq, mem = torch.randn(2, 9, 32, generator=g).double(), torch.randn(2, 6, 32, generator=g).double()
    lens = torch.tensor([6, 4])
    pre = "decoder.layers.0.multihead_attn"
    _, a0 = multi_head_attention(sd, pre, xq, mem, 2, lens, False, 0.25, False)
    keep = torch.from_numpy(dm.keep_attn(99, 2 * 2 * 9, 6, 0.25)).view(2, 2, 9, 6)
    with drop_masks({"s": keep}):
        o1, a1 = multi_head_attention(sd, pre, xq, mem, 2, lens, False, 0.25, True, "s")
    live = a0 > 0
    assert torch.equal((a1 == 0) & live, ~keep & live) and 0 < int((~keep & live).sum()) < int(live.sum())
    assert torch.equal(a1[keep], a0[keep] * dm.drop_scale(0.25))
    x = torch.randn(2, 9, 32, generator=g).double()
    keep = torch.from_numpy(dm.keep_flat(5, x.numel(), 0.1)).view(x.shape)
    y0 = positional_encoding(sd, x, 0.1, False)
    with drop_masks({"enc.pe": keep.flatten()}):                     # (any shape with the site's element count)
        y1 = positional_encoding(sd, x, 0.1, True, "enc.pe")
    assert torch.equal(y1, y0 * keep * dm.drop_scale(0.1)) and int((y1 == 0).sum()) == int((~keep).sum())


def test_a_site_without_a_mask_is_an_error():
    from oracle import drop_masks
    cfg, batch, new_state = _tiny_case()
    shapes = _site_shapes(cfg, 2, batch["phoneme"].shape[1], batch["melspec"].shape[1])
    masks = {k: torch.ones(v, dtype=torch.bool) for k, v in shapes.items()}
    del masks["decoder.layers.0.cross_out"]
    with drop_masks(masks), pytest.raises(KeyError, match="decoder.layers.0.cross_out"):
        _run(cfg, batch, new_state(), dropout=True)
    masks["decoder.layers.0.cross_out"] = torch.ones(3, dtype=torch.bool)
    with drop_masks(masks), pytest.raises(ValueError, match="elements"):
        _run(cfg, batch, new_state(), dropout=True)
    # with dropout off nothing draws, so nothing is asked for
    with drop_masks({}) as rec:
        _run(cfg, batch, new_state(), dropout=False)
    assert rec.used == []


def test_dropout_on_without_the_context_is_unchanged():
    """the plain `dropout=True` path still draws from torch's generator (F.dropout): same values as before under the same seed"""
    import torch.nn.functional as F
    from oracle.ref_model import _drop
    x = torch.randn(5, 7, generator=torch.Generator().manual_seed(2))
    torch.manual_seed(11)
    a = _drop(x, 0.3, True, "anything")
    torch.manual_seed(11)
    assert torch.equal(a, F.dropout(x, 0.3, training=True))
    assert _drop(x, 0.3, False) is x and _drop(x, 0.0, True) is x
    cfg, batch, new_state = _tiny_case()
    torch.manual_seed(12)
    o1 = _run(cfg, batch, new_state(), dropout=True)
    torch.manual_seed(12)
    o2 = _run(cfg, batch, new_state(), dropout=True)
    o0 = _run(cfg, batch, new_state(), dropout=False)
    assert torch.equal(o1["post_melspec"], o2["post_melspec"]) and not torch.equal(o1["post_melspec"], o0["post_melspec"])


def test_training_step_takes_one_mask_set_per_forward():
    """the two forwards of `oracle_training_step` run under their own masks: all-ones masks at scale 1 are the dropout-off
    step bit for bit (at the sites' own scale 1 / (1 - p) they are not); a zeroed site in the FIRST set changes the step, and
    does so through the scheduled-sampling mix"""
    from oracle import oracle_training_step
    from oracle.ref_model import drop_masks
    cfg, batch, new_state = _tiny_case()
    Tm = batch["melspec"].shape[1]
    shapes = _site_shapes(cfg, 2, batch["phoneme"].shape[1], Tm)
    ones = lambda: {k: torch.ones(v, dtype=torch.bool) for k, v in shapes.items()}
    u = torch.rand(2, 1, Tm, generator=torch.Generator().manual_seed(5)).double()
    b64 = dict(batch, melspec=batch["melspec"].double())
    sd0, sd1 = new_state(), new_state()
    l0, _, mixed0 = oracle_training_step(sd0, cfg, b64, epoch=120, seed_u=u)
    l1, _, mixed1 = oracle_training_step(sd1, cfg, b64, epoch=120, seed_u=u, masks=(ones(), ones()), mask_scale=1.0)
    assert drop_masks.active is None
    assert torch.equal(l1["total"], l0["total"]) and torch.equal(mixed1, mixed0) and bool((mixed0 != b64["melspec"]).any())
    l0["total"].backward()
    l1["total"].backward()
    for k, v in sd0.items():                # both BatchNorm updates and every gradient
        assert torch.equal(sd1[k], v), k
        if v.requires_grad:
            assert torch.equal(sd1[k].grad, v.grad), k
    l2, _, _ = oracle_training_step(new_state(), cfg, b64, epoch=120, seed_u=u, masks=(ones(), ones()))
    assert not torch.equal(l2["total"], l0["total"])
    first = ones()
    first["dec.pe"] = torch.zeros(shapes["dec.pe"], dtype=torch.bool)
    l3, _, mixed3 = oracle_training_step(new_state(), cfg, b64, epoch=120, seed_u=u, masks=(first, ones()), mask_scale=1.0)
    assert not torch.equal(mixed3, mixed0) and not torch.equal(l3["total"], l0["total"])
    # the same site zeroed in the SECOND set leaves the mix alone and changes the loss
    l4, _, mixed4 = oracle_training_step(new_state(), cfg, b64, epoch=120, seed_u=u, masks=(ones(), first), mask_scale=1.0)
    assert torch.equal(mixed4, mixed0) and not torch.equal(l4["total"], l0["total"])
