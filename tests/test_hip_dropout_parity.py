"""The dropout-ON training path against the fp64 oracle.

The dropout RNG of the kernels is a pure function of (site seed, element index) in 32-bit integer arithmetic
(csrc/ttts_common.h), restated on the host in oracle/dropmask.py.  Here that restatement is (A) pinned to the kernels element
for element, and (C) used to hand the fp64 oracle the very masks the HIP path drew (`oracle.drop_masks`, keyed by site name),
which makes a dropout-on forward / backward as continuous a comparison as the dropout-off one of tests/test_hip_model.py --
same quantities, same gates.  A mask that forward and backward index differently, a wrong 1 / (1 - p), a seed handed to the
wrong site: each fails these comparisons by orders of magnitude.  Per-site kernel tests with the same masks sit next to the
model tests, so that a red model test has a small neighbour that says where."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from test_hip_model import FLIP_FREE_GATE, GATE, GRAD_GATE, _build, _oracle64, _oracle_gated_grads
from test_hip_ops import TOL, _dev, _g, _rand, _ref_attention

from oracle import dropmask as dm

pytestmark = pytest.mark.gpu
# where the measured worst values of each case are written (one small text file per case)
REPORT_DIR = os.environ.get("TTTS_REPORT_DIR", "parity_reports")


def _t(keep: np.ndarray, *shape) -> torch.Tensor:
    return torch.from_numpy(keep).view(*shape)


# ============================================================================================ A. the restatement IS the kernels'
SEEDS = (0x5EED5EED, 0xD1B54A32D192ED03)          # (the second has a non-zero high word: the hash folds both halves)


@pytest.mark.parametrize("n,seed,p,word", [(4 * 70001, s, p, w) for s in SEEDS for p in (0.1, 0.5) for w in (None, 0xABCDEF0123456789)]
                         + [(2100004, SEEDS[1], 0.1, 0x1111222233334444)])
def test_flat_mask_restatement_equals_the_kernel(n, seed, p, word):
    """ttts_dropout_bwd on ones returns keep_flat * drop_scale EXACTLY.  n = 280 004: no multiple of the 256-thread block;
    n = 2 100 004: more than 2048 blocks x 256 threads x 4 elements, i.e. through the grid-stride loop.  `word`: under an active
    StepState whose seed word the kernel XORs into the site seed."""
    from transformertts_amd import _lib, ops
    from transformertts_amd.ops import _p, _stream
    lib, dev = _lib.load(), _dev()
    dy, dx = torch.ones(n, device=dev), torch.empty(n, device=dev)
    st = None
    if word is not None:
        st = ops.StepState(dev)
        st.push(seed=word, lr=0.0, p_tf=1.0, step=1)
    assert lib.ttts_dropout_bwd(_p(dy), _p(dx), n, p, seed, None if st is None else st.ptr, None, _stream()) == 0
    keep = dm.keep_flat(dm.site_seed(seed, word), n, p)
    want = torch.from_numpy(keep.astype(np.float32) * np.float32(dm.drop_scale(p)))
    got = dx.cpu()
    assert torch.equal(got, want), (int((got != want).sum()), int(((got != 0) != torch.from_numpy(keep)).sum()))
    assert abs(float((got == 0).float().mean()) - p) < 0.01
    if word is not None:          # and the word matters
        assert not np.array_equal(keep, dm.keep_flat(seed, n, p))


def test_attention_mask_restatement_equals_the_cross_attention_weights():
    """the post-dropout weights of ops.cross_attention(need_weights=True) are zero exactly where keep_attn says (row
    (b H + h) Tq + q, key k), and the kept ones are the undropped weights times drop_scale; on fp32 operands and on head images"""
    from transformertts_amd import ops
    dev = _dev()
    B, H, Tq, Tk, p, seed = 2, 2, 70, 23, 0.25, 0x0123456789ABCDEF
    d = H * 64
    q_, kv_ = _rand(B, Tq, d, seed=1), _rand(B, Tk, 2 * d, seed=2)
    lens = torch.tensor([23, 9], dtype=torch.int64)
    keep = _t(dm.keep_attn(seed, B * H * Tq, Tk, p), B, H, Tq, Tk)
    live = (torch.arange(Tk).view(1, 1, 1, Tk) < lens.view(B, 1, 1, 1)).expand(B, H, Tq, Tk)
    with torch.no_grad():
        _, a0 = ops.cross_attention(q_.to(dev), kv_.to(dev), lens.to(dev), H, 0.0, 0, True)
        _, a1 = ops.cross_attention(q_.to(dev), kv_.to(dev), lens.to(dev), H, p, seed, True)
    a0, a1 = a0.cpu(), a1.cpu()
    assert bool((a0[live] > 0).all())
    assert torch.equal(a1 != 0, keep & live), int(((a1 != 0) != (keep & live)).sum())
    assert rel_l2(a1, a0.double() * keep * dm.drop_scale(p)) < 1e-6
    # the head-image kernels (what the models with 64-column heads run): same rows, same keys
    x, mem = _rand(B, Tq, d, seed=3), _rand(B, Tk, d, seed=4)
    wq, wkv = _rand(d, d, seed=5, scale=d ** -0.5), _rand(2 * d, d, seed=6, scale=d ** -0.5)
    with torch.no_grad():
        qi = ops.linear(x.to(dev), wq.to(dev), None, head_image_sections=1)
        kvi = ops.linear(mem.to(dev), wkv.to(dev), None, head_image_sections=2)
        assert isinstance(qi, ops.HeadImage)
        _, b0 = ops.cross_attention(qi, kvi, lens.to(dev), H, 0.0, 0, True)
        _, b1 = ops.cross_attention(qi, kvi, lens.to(dev), H, p, seed, True)
    b0, b1 = b0.cpu(), b1.cpu()
    assert torch.equal(b1 != 0, keep & live & (b0 != 0)) and int((b0[live] == 0).sum()) == 0
    assert rel_l2(b1, b0.double() * keep * dm.drop_scale(p)) < 1e-6


@pytest.mark.parametrize("image", [False, True])
def test_self_attention_dropout_vs_fp64(image):
    """Self-attention dropout: its weights are never returned, so only output and dqkv can observe its mask -- against the fp64
    reference attention that drops by keep_attn (causal, ragged lengths).  On fp32 operands and through the in-projection that
    leaves a head image (what the models run)."""
    from transformertts_amd import ops
    dev = _dev()
    B, H, T, p, seed = 2, 2, 70, 0.25, 0xFEDCBA9876543210
    d = H * 64
    lens = torch.tensor([70, 31], dtype=torch.int64)
    do = _rand(B, T, d, seed=2)
    keep = _t(dm.keep_attn(seed, B * H * T, T, p), B, H, T, T).double() * dm.drop_scale(p)

    def ref_attn(qkv):
        q, k, v = [t.view(B, T, H, 64).transpose(1, 2) for t in qkv.split(d, dim=-1)]
        _, a = _ref_attention(q, k, v, lens, True)
        return ((a * keep) @ v).transpose(1, 2).reshape(B, T, d)

    if not image:
        qkv = _rand(B, T, 3 * d, seed=1)
        qd = qkv.double().requires_grad_()
        ref = ref_attn(qd)
        ref.backward(do.double())
        qg = _g(qkv)
        out = ops.self_attention(qg, lens.to(dev), H, True, p, seed)
        out.backward(do.to(dev))
        assert rel_l2(out, ref) < TOL and rel_l2(qg.grad, qd.grad) < TOL, (rel_l2(out, ref), rel_l2(qg.grad, qd.grad))
        return
    x, w, b = _rand(B, T, d, seed=3), _rand(3 * d, d, seed=4, scale=d ** -0.5), _rand(3 * d, seed=5, scale=0.1)
    xd, wd, bd = [t.double().requires_grad_() for t in (x, w, b)]
    ref = ref_attn(F.linear(xd, wd, bd))
    ref.backward(do.double())
    xg, wg, bg = _g(x), _g(w), _g(b)
    qkv = ops.linear(xg, wg, bg, head_image_sections=3)
    assert isinstance(qkv, ops.HeadImage)
    out = ops.self_attention(qkv, lens.to(dev), H, True, p, seed)
    out.backward(do.to(dev))
    errs = [rel_l2(out, ref), rel_l2(xg.grad, xd.grad), rel_l2(wg.grad, wd.grad), rel_l2(bg.grad, bd.grad)]
    assert max(errs) < TOL, errs


# ============================================================================================ per-site kernels under dropout
def test_posenc_dropout_vs_fp64():
    """ops.posenc at p = 0.1: y, dx and d alpha (a sum over the MASKED gradient: the backward regenerates the mask)"""
    from oracle.spec import sinusoid_table
    from transformertts_amd import ops
    dev = _dev()
    B, T, d, p, seed = 3, 21, 128, 0.1, 0x9E3779B97F4A7C15
    pe = sinusoid_table(100, d)
    x, alpha, dy = _rand(B, T, d, seed=4), torch.tensor([1.3]), _rand(B, T, d, seed=3)
    keep = _t(dm.keep_flat(seed, B * T * d, p), B, T, d).double() * dm.drop_scale(p)
    xd, ad = x.double().requires_grad_(), alpha.double().requires_grad_()
    ref = (xd + ad * pe[:T].double().unsqueeze(0)) * keep
    ref.backward(dy.double())
    xg, ag = _g(x), _g(alpha)
    y = ops.posenc(xg, pe.to(dev), ag, p, seed)
    y.backward(dy.to(dev))
    assert torch.equal(y.cpu() == 0, keep == 0)
    assert rel_l2(y, ref) < TOL and rel_l2(xg.grad, xd.grad) < TOL and rel_l2(ag.grad, ad.grad) < TOL


@pytest.mark.parametrize("B,T,cin,cout", [(3, 37, 128, 128), (2, 131, 80, 256)])
def test_conv_bn_tanh_dropout_vs_fp64(B, T, cin, cout):
    """ops.conv_bn with tanh and p = 0.5 (the post-net layers and, without tanh, the encoder pre-net): z, running statistics, dx,
    dw, d gamma, d beta -- the backward regenerates the mask in front of the tanh derivative, and d gamma / d beta are sums over
    masked gradients"""
    from transformertts_amd import ops
    k, p, seed = 5, 0.5, 0xC2B2AE3D27D4EB2F
    x = _rand(B, T, cin, seed=1)
    w = _rand(cout, cin, k, seed=2, scale=(cin * k) ** -0.5)
    b = _rand(cout, seed=3, scale=0.1)
    gamma = 0.8 + 0.4 * torch.rand(cout, generator=torch.Generator().manual_seed(4))
    beta = _rand(cout, seed=5, scale=0.1)
    rm, rv = _rand(cout, seed=6, scale=0.1), 0.5 + torch.rand(cout, generator=torch.Generator().manual_seed(7))
    dz = _rand(B, T, cout, seed=8)
    keep = _t(dm.keep_flat(seed, B * T * cout, p), B, T, cout).double() * dm.drop_scale(p)
    xd, wd, bd, gd, bed = [t.double().requires_grad_() for t in (x, w, b, gamma, beta)]
    rmd, rvd = rm.double().clone(), rv.double().clone()
    y = F.conv1d(xd.transpose(1, 2), wd, bd, padding=2)
    y = F.batch_norm(y, rmd, rvd, gd, bed, training=True, momentum=0.1, eps=1e-5).transpose(1, 2)
    ref = torch.tanh(y) * keep
    ref.backward(dz.double())
    xg, wg, bg, gg, beg = _g(x), _g(w), _g(b), _g(gamma), _g(beta)
    rmg, rvg = rm.to(_dev()), rv.to(_dev())
    nbt = torch.zeros((), dtype=torch.int64, device=_dev())
    z = ops.conv_bn(xg, wg, bg, gg, beg, rmg, rvg, nbt, True, 0.1, 1e-5, ops.ACT_TANH, p, seed)
    z.backward(dz.to(_dev()))
    assert int(nbt.item()) == 1
    errs = dict(z=rel_l2(z, ref), rm=rel_l2(rmg, rmd), rv=rel_l2(rvg, rvd), dx=rel_l2(xg.grad, xd.grad), dw=rel_l2(wg.grad, wd.grad),
                dgamma=rel_l2(gg.grad, gd.grad), dbeta=rel_l2(beg.grad, bed.grad))
    assert all(v < TOL for v in errs.values()), errs


def test_decoder_prenet_pair_dropout_vs_fp64():
    """The decoder pre-net: Linear(relu, p = 0.5) on the go-frame loader (row_shift = -1) feeding Linear(relu, p = 0.5) as its sole
    consumer -- the first mask is indexed by the OUTPUT row as stored (not by the shifted input row), and the first Linear's
    relu / dropout backward rides in the second one's data-gradient epilogue (the relu token)"""
    from transformertts_amd import ops
    dev = _dev()
    B, T, K, N, p, s1, s2 = 3, 37, 80, 256, 0.5, 0x1111111122222222, 0x3333333344444444
    x = _rand(B, T, K, seed=1)
    w1, b1 = _rand(N, K, seed=2, scale=K ** -0.5), _rand(N, seed=3, scale=0.1)
    w2, b2 = _rand(N, N, seed=4, scale=N ** -0.5), _rand(N, seed=5, scale=0.1)
    dy = _rand(B, T, N, seed=6)
    k1 = _t(dm.keep_flat(s1, B * T * N, p), B, T, N).double() * dm.drop_scale(p)
    k2 = _t(dm.keep_flat(s2, B * T * N, p), B, T, N).double() * dm.drop_scale(p)
    xs = torch.cat((torch.zeros(B, 1, K), x[:, :-1]), dim=1).double()
    ps = [t.double().requires_grad_() for t in (w1, b1, w2, b2)]
    h = F.relu(F.linear(xs, ps[0], ps[1])) * k1
    ref = F.relu(F.linear(h, ps[2], ps[3])) * k2
    ref.backward(dy.double())
    gs = [_g(t) for t in (w1, b1, w2, b2)]
    hg = ops.linear(x.to(dev), gs[0], gs[1], act=ops.ACT_RELU, drop_p=p, seed=s1, row_shift=-1, T=T, publish_amax=True)
    y = ops.linear(hg, gs[2], gs[3], act=ops.ACT_RELU, drop_p=p, seed=s2, sole_consumer=True)
    y.backward(dy.to(dev))
    assert rel_l2(hg, h) < TOL and rel_l2(y, ref) < TOL, (rel_l2(hg, h), rel_l2(y, ref))
    errs = {n: rel_l2(a.grad, r.grad) for n, a, r in zip(("dw1", "db1", "dw2", "db2"), gs, ps)}
    assert all(v < TOL for v in errs.values()), errs


@pytest.mark.parametrize("M,d", [(130, 256), (1100, 256), (130, 512), (1100, 512)])
def test_residual_dropout_handoff_to_layernorm_vs_fp64(M, d):
    """y = drop(x W + b) + r -> layer_norm(y, sole_consumer=True): the Linear's dropout backward is written by the LayerNorm's
    backward kernel (ttts_layernorm_bwd_drop) from the seed that travels on the drop token -- the two kernels must agree on
    seed, threshold and flat index.  Every gradient against fp64; M = 1100: past one pass of the backward's row loop."""
    from transformertts_amd import ops
    dev = _dev()
    p, seed = 0.1, 0x5555555566666666
    x, w, b, r = _rand(M, d, seed=1), _rand(d, d, seed=2, scale=d ** -0.5), _rand(d, seed=3, scale=0.1), _rand(M, d, seed=4)
    g, be, dz = 1 + _rand(d, seed=5, scale=0.2), _rand(d, seed=6, scale=0.1), _rand(M, d, seed=7)
    keep = _t(dm.keep_flat(seed, M * d, p), M, d).double() * dm.drop_scale(p)
    ps = [t.double().requires_grad_() for t in (x, w, b, r, g, be)]
    ref = F.layer_norm(F.linear(ps[0], ps[1], ps[2]) * keep + ps[3], (d,), ps[4], ps[5], 1e-5)
    ref.backward(dz.double())
    gs = [_g(t) for t in (x, w, b, r, g, be)]
    y = ops.linear(gs[0], gs[1], gs[2], residual=gs[3], drop_p=p, seed=seed)
    assert getattr(y, "_ttts_drop_token", None) is not None
    z = ops.layer_norm(y, gs[4], gs[5], 1e-5, sole_consumer=True)
    z.backward(dz.to(dev))
    errs = {"z": rel_l2(z, ref)}
    errs.update({n: rel_l2(a.grad, q.grad) for n, a, q in zip(("dx", "dw", "db", "dr", "dgamma", "dbeta"), gs, ps)})
    assert all(v < TOL for v in errs.values()), errs


# ============================================================================================ C. the model, dropout on
def _site_specs(cfg, B, Tp, Tm):
    """name -> (kind, p, rows, cols) of every dropout site of one forward, in the HIP path's launch order; rows x cols is the
    (rows, N) output of a flat site as stored, or the (B H Tq, Tk) weight matrix of an attention site"""
    d, He, Hd = cfg["d_model"], cfg["encoder_n_head"], cfg["decoder_n_head"]
    pe, pd = cfg["encoder_dropout"], cfg["decoder_dropout"]
    enc, dec, post = {}, {}, {}
    for i in range(cfg["encoder_prenet_n_layers"]):
        enc[f"enc_prenet.{i}"] = ("flat", cfg["encoder_prenet_dropout"], B * Tp, cfg["encoder_prenet_out_channel"])
    enc["enc.pe"] = ("flat", 0.1, B * Tp, d)
    for i in range(cfg["encoder_n_layers"]):
        n = f"encoder.layers.{i}"
        enc.update({f"{n}.attn": ("attn", pe, B * He * Tp, Tp), f"{n}.attn_out": ("flat", pe, B * Tp, d),
                    f"{n}.ffn_h": ("flat", pe, B * Tp, cfg["encoder_d_ffn"]), f"{n}.ffn_out": ("flat", pe, B * Tp, d)})
    dec.update({"dec_prenet.0": ("flat", 0.5, B * Tm, d), "dec_prenet.1": ("flat", 0.5, B * Tm, d), "dec.pe": ("flat", 0.1, B * Tm, d)})
    for i in range(cfg["decoder_n_layers"]):
        n = f"decoder.layers.{i}"
        dec.update({f"{n}.attn": ("attn", pd, B * Hd * Tm, Tm), f"{n}.attn_out": ("flat", pd, B * Tm, d),
                    f"{n}.cross": ("attn", pd, B * Hd * Tm, Tp), f"{n}.cross_out": ("flat", pd, B * Tm, d),
                    f"{n}.ffn_h": ("flat", pd, B * Tm, cfg["decoder_d_ffn"]), f"{n}.ffn_out": ("flat", pd, B * Tm, d)})
    n_post = cfg["postnet_n_layers"]
    for i in range(n_post):
        post[f"postnet.{i}"] = ("flat", cfg["postnet_dropout"], B * Tm, cfg["n_mels"] if i == n_post - 1 else d)
    return enc, dec, post


def _oracle_shape(name, cfg, B, Tp, Tm, rows, cols):
    """the shape the oracle's site has (attention weights: (B, H, Tq, Tk))"""
    if name.endswith((".attn", ".cross")):
        H = cfg["encoder_n_head"] if name.startswith("encoder") else cfg["decoder_n_head"]
        return (B, H, rows // (B * H), cols)
    return (B, rows // B, cols)


class _Recorder:
    """records the dropout launches (ops._drop_observer) and the relu outputs (ops._relu_observer) of what runs inside"""

    def __init__(self, seed):
        self.seed, self.drops, self.relus = seed, [], []

    def __enter__(self):
        from transformertts_amd import ops
        ops.seeds.manual_seed(self.seed)
        ops._drop_observer = lambda *rec: self.drops.append(rec)
        ops._relu_observer = lambda y: self.relus.append((y.detach() > 0).cpu())
        return self

    def __exit__(self, *exc):
        from transformertts_amd import ops
        ops._drop_observer = ops._relu_observer = None
        ops.seeds.follow_torch()


def _mask(kind, seed, p, rows, cols, word):
    seed = dm.site_seed(seed, word)
    return dm.keep_attn(seed, rows, cols, p) if kind == "attn" else dm.keep_flat(seed, rows * cols, p).reshape(rows, cols)


CASES = [("tiny", 3, 12, 40, 11, 21, None), ("micro", 3, 12, 40, 16, 26, None), ("base", 2, 60, 300, 12, 22, None),
         # 4350 rows: > 4096 (the row-dot backward's second row in flight), > 1024 (the LayerNorm backward's row loop), 2-D tile grids
         ("base", 5, 100, 870, 13, 23, None),
         # under an active StepState with a non-zero seed word: the masks come from site_seed(seed, word)
         ("tiny", 3, 12, 40, 11, 21, 0x0F1E2D3C4B5A6978)]


@pytest.mark.parametrize("cfg_name,B,Tp,Tm,w_seed,b_seed,word", CASES)
def test_dropout_on_forward_backward_vs_oracle(cfg_name, B, Tp, Tm, w_seed, b_seed, word):
    """What test_forward_backward_vs_oracle compares -- the three outputs, every alignment map, the loss, BatchNorm running
    statistics and counters, every parameter gradient -- with the configuration's dropout ON: the fp64 oracle runs under the
    masks the HIP path drew (rebuilt on the host from the recorded site seeds) and, for the gradients, under its ReLU gates.
    Gates: GATE (outputs), FLIP_FREE_GATE (gradients; above it the fallback rule of that test: at most twice stock fp32 torch
    under the same gates and masks, never above GATE).  Measured worst values: parity_dropout_*.txt in REPORT_DIR, and DESIGN.md."""
    import contextlib
    from oracle import drop_masks, drop_site_names, oracle_forward, oracle_loss, relu_gates, synth_batch
    from transformertts_amd import ops
    from transformertts_amd.loss import TransformerTTSLoss
    cfg, m = _build(cfg_name, w_seed, dropout=True)
    batch = synth_batch(B, Tp, Tm, cfg["n_mels"], cfg["n_phon"], ragged=True, seed=b_seed)
    Tp, Tm = batch["phoneme"].shape[1], batch["melspec"].shape[1]
    dev = torch.device("cuda")
    args = [batch[k].to(dev) for k in ("phoneme", "melspec", "phoneme_lens", "melspec_lens")]
    m.train()
    st = contextlib.nullcontext()
    if word is not None:
        st = ops.StepState(dev)
        st.push(seed=word, lr=0.0, p_tf=1.0, step=1)
    with _Recorder(0xD0D0 + w_seed) as rec, st:
        out = m(*args)
        loss = TransformerTTSLoss(8.0).to(dev)(out, args[1], args[3])
        loss["total"].backward()
    torch.cuda.synchronize()

    # every launch that drew is one named site, with the kind, p and geometry that site has; none is missing
    enc, dec, post = _site_specs(cfg, B, Tp, Tm)
    specs = {**enc, **dec, **post}
    assert len(rec.drops) == len(specs) == len(drop_site_names(cfg)) and sorted(specs) == sorted(drop_site_names(cfg))
    assert len({r[1] for r in rec.drops}) == len(rec.drops)             # one seed per site
    masks = {}
    for (name, (kind, p, rows, cols)), (rkind, seed, rp, shape, half) in zip(specs.items(), rec.drops):
        assert (rkind, shape, half) == (kind, (rows, cols), None) and abs(rp - p) < 1e-12, (name, rkind, rp, shape, half)
        masks[name] = _t(_mask(kind, seed, p, rows, cols, word), *_oracle_shape(name, cfg, B, Tp, Tm, rows, cols))

    sd = _oracle64(cfg, w_seed)
    with relu_gates() as pre, drop_masks(masks) as used:
        ref = oracle_forward(sd, cfg, batch["phoneme"], batch["melspec"].double(), batch["phoneme_lens"], batch["melspec_lens"],
                             training=True, dropout=True)
    rloss = oracle_loss(ref, batch["melspec"].double(), batch["melspec_lens"])
    assert sorted(used.used) == sorted(masks)                           # as many sites drew in the oracle, under the same names
    # The gate decisions, absolutely.  The observer sees relu AND dropout (y > 0 is gate AND keep), so: a dropped unit is never
    # "on", and among the KEPT units the HIP path may gate differently from exact arithmetic only within rounding distance of zero
    relu_sites = [f"encoder.layers.{i}.ffn_h" for i in range(cfg["encoder_n_layers"])] + ["dec_prenet.0", "dec_prenet.1"] + \
                 [f"decoder.layers.{i}.ffn_h" for i in range(cfg["decoder_n_layers"])]
    assert len(pre.pre) == len(rec.relus) == len(relu_sites)
    flips, units = 0, 0
    for name, x, gate in zip(relu_sites, pre.pre, rec.relus):
        keep, gate = masks[name].reshape(x.shape), gate.reshape(x.shape)
        assert not bool((gate & ~keep).any()), ("a dropped unit is on", name)
        diff = ((x > 0) != gate) & keep
        flips += int(diff.sum())
        units += x.numel()
        if diff.any():
            lim = 1e-5 * max(1.0, float(x.abs().max()) / 30.0)
            assert float(x[diff].abs().max()) < lim, ("a kept ReLU unit far from zero was gated differently", name, float(x[diff].abs().max()))
    assert flips <= max(20, units // 100000), (flips, units)

    errs = {k: rel_l2(out[k], ref[k]) for k in ("pred_melspec", "post_melspec", "pred_stop")}
    for i, (a, r) in enumerate(zip(out["alignments"], ref["alignments"])):
        errs[f"align{i}"] = rel_l2(a, r)
    errs["loss"] = abs(loss["total"].item() - rloss["total"].item()) / abs(rloss["total"].item())
    for name, buf in m.named_buffers():
        if "running_" in name:
            errs[name] = rel_l2(buf, sd[name])
        if "num_batches" in name:
            assert int(buf.item()) == int(sd[name]) == 1
    gated, _ = _oracle_gated_grads(cfg, w_seed, batch, rec.relus, masks=masks)
    gerrs = {}
    for name, p in m.named_parameters():
        rg = gated[name]
        if rg.norm().item() < 1e-7 * max(1.0, sd[name].detach().norm().item()):   # analytically-zero grads (conv bias before BN)
            assert p.grad.abs().max().item() < 1e-4, name
            continue
        gerrs[name] = rel_l2(p.grad, rg)
    bad = {k: v for k, v in errs.items() if not v < GATE}
    over = {k: v for k, v in gerrs.items() if not v < FLIP_FREE_GATE}
    fallback = {}
    if over:
        stock, _ = _oracle_gated_grads(cfg, w_seed, batch, rec.relus, dtype=torch.float32, masks=masks)
        for k, v in over.items():
            fallback[k] = (v, rel_l2(stock[k], gated[k]))
            if not (v < 2.0 * fallback[k][1] and v < GATE):
                bad[k] = fallback[k]
    os.makedirs(REPORT_DIR, exist_ok=True)
    tag = f"{cfg_name}_B{B}_Tm{Tm}" + ("_stepstate" if word is not None else "")
    with open(f"{REPORT_DIR}/parity_dropout_{tag}.txt", "w") as f:
        f.write(f"# dropout ON, {len(masks)} sites; {flips} of {units} kept ReLU units gated differently\n")
        wk, wg = max(errs, key=errs.get), max(gerrs, key=gerrs.get)
        f.write(f"# worst output / buffer / loss: {errs[wk]:.3e} {wk}  (gate {GATE:g})\n")
        f.write(f"# worst gradient: {gerrs[wg]:.3e} {wg}  (gate {FLIP_FREE_GATE:g})\n")
        for k, (v, e32) in fallback.items():
            f.write(f"# above the gradient gate: {k} {v:.3e}, stock fp32 under the same gates and masks {e32:.3e}\n")
        for k, v in sorted(errs.items(), key=lambda kv: -kv[1]):
            f.write(f"{v:.3e} {k}\n")
        for k, v in sorted(gerrs.items(), key=lambda kv: -kv[1]):
            f.write(f"{v:.3e} grad/{k}\n")
    assert not bad, bad


def _step_stream(cfg, B, Tp, Tm, twin_enc, twin_post):
    """the dropout launches of one training_step in launch order: (site, kind, p, rows, cols, half, forwards); `forwards`: which
    forward's mask the launch draws -- "ng" (the no-grad forward, which runs first), "g", or "both": one launch over the twin
    batch of 2 B utterances, the grad forward's first"""
    enc, dec, post = _site_specs(cfg, B, Tp, Tm)
    one = lambda sites, fw: [(n, k, p, r, c, None, fw) for n, (k, p, r, c) in sites.items()]
    s = []
    if twin_enc:       # BatchNorm stays per forward: the pre-net's conv blocks normalise (and drop) each half in a launch of its own
        for n, (k, p, r, c) in enc.items():
            s += [(n, k, p, r, c, 1, "ng"), (n, k, p, r, c, 0, "g")] if n.startswith("enc_prenet") else [(n, k, p, 2 * r, c, None, "both")]
    for fw in ("ng", "g"):
        if not twin_enc:
            s += one(enc, fw)
        s += one(dec, fw)
        if not twin_post:
            s += one(post, fw)
        elif fw == "g":            # one post-net pass over both predictions: per layer the no-grad half's launch, then the grad
            for i, (n, (k, p, r, c)) in enumerate(post.items()):         # half's; nobody reads the no-grad half of the last layer
                if i < len(post) - 1:
                    s.append((n, k, p, r, c, 1, "ng"))
                s.append((n, k, p, r, c, 0, "g"))
    return s


@pytest.mark.parametrize("twin_encoder", [True, False])
def test_dropout_on_training_step_vs_oracle(twin_encoder):
    """One LightningModule.training_step on tiny with dropout ON and p_tf < 1 (injected uniform draw), against
    oracle_training_step given the masks of each of its two forwards.  Default flags: the encoder of both forwards runs as ONE
    pass over 2 B utterances (encode_twin) and the post-net once over both predictions (PostnetTwin) -- each half must see the
    masks of its own forward: one launch hashes the whole 2 B-row buffer (the grad forward's rows first), the halves of the
    conv + BatchNorm blocks are launches of their own.  With the twin encoder switched off the step must agree with the oracle as well (the two
    variants draw different masks, so each is compared with the oracle, not with the other).  Loss and gradients at the gates of
    test_training_step_surface, BatchNorm running statistics -- updated twice, the no-grad forward's first -- at GATE."""
    import transformertts_amd.utils.util as U
    from oracle import model_config, fill_state, synth_batch, oracle_training_step
    from transformertts_amd import ops
    from transformertts_amd.lightning_module import LightningModule
    cfg = model_config("tiny")
    config = {"model": dict(cfg, device="cuda"), "loss": {"stop_weight": 8.0},
              "training": {"num_epochs": 300, "teacher_forcing_mode": "linear", "warmup_steps": 4000}}
    B = 3
    batch = synth_batch(B, 12, 40, cfg["n_mels"], cfg["n_phon"], ragged=True, seed=21)
    Tp, Tm = batch["phoneme"].shape[1], batch["melspec"].shape[1]
    u = torch.rand(B, 1, Tm, generator=torch.Generator().manual_seed(5))
    ops.TWIN_ENCODER = twin_encoder
    try:
        lm = LightningModule(config).to("cuda")
        lm.model.load_state_dict(fill_state(cfg, 11), strict=True)
        lm.train()
        lm.current_epoch = 120
        assert lm.model.twin_encode_ok(batch["phoneme"].to("cuda")) == twin_encoder and lm.model.twin_postnet_ok(batch["melspec"].to("cuda"))
        U._uniform_draw = lambda B_, T_, device: u.to(device)
        try:
            with _Recorder(0x7717 + int(twin_encoder)) as rec:
                loss = lm.training_step(dict(batch), 1)
                loss.backward()
        finally:
            U._uniform_draw = None
        torch.cuda.synchronize()
    finally:
        ops.TWIN_ENCODER = True
    stream = _step_stream(cfg, B, Tp, Tm, twin_encoder, True)
    assert len(rec.drops) == len(stream), (len(rec.drops), len(stream))
    sets = {"ng": {}, "g": {}}
    for (name, kind, p, rows, cols, half, fw), (rkind, seed, rp, shape, rhalf) in zip(stream, rec.drops):
        assert (rkind, shape, rhalf) == (kind, (rows, cols), half) and abs(rp - p) < 1e-12, (name, fw, rkind, rp, shape, rhalf)
        keep = _mask(kind, seed, p, rows, cols, None)
        if fw == "both":
            sets["g"][name] = _t(keep[:rows // 2].copy(), *_oracle_shape(name, cfg, B, Tp, Tm, rows // 2, cols))
            sets["ng"][name] = _t(keep[rows // 2:].copy(), *_oracle_shape(name, cfg, B, Tp, Tm, rows // 2, cols))
        else:
            assert name not in sets[fw]
            sets[fw][name] = _t(keep, *_oracle_shape(name, cfg, B, Tp, Tm, rows, cols))
    # the no-grad forward's output of the last post-net layer has no reader (its BatchNorm statistics precede its dropout): the
    # HIP path does not draw that mask, and whichever the oracle gets changes nothing that is compared
    last = f"postnet.{cfg['postnet_n_layers'] - 1}"
    assert last not in sets["ng"]
    sets["ng"][last] = torch.ones_like(sets["g"][last])
    assert sorted(sets["ng"]) == sorted(sets["g"])
    sd = _oracle64(cfg, 11)
    b64 = dict(batch, melspec=batch["melspec"].double())
    rloss, _, _ = oracle_training_step(sd, cfg, b64, epoch=120, seed_u=u.double(), masks=(sets["ng"], sets["g"]))
    rloss["total"].backward()
    lerr = abs(loss.item() - rloss["total"].item()) / abs(rloss["total"].item())
    gerrs = {n: rel_l2(p.grad, sd[n].grad) for n, p in lm.model.named_parameters() if sd[n].grad.norm().item() >= 1e-7}
    berrs = {}
    for name, buf in lm.model.named_buffers():
        if "num_batches" in name:
            assert int(buf.item()) == int(sd[name]) == 2
        elif "running_" in name:
            berrs[name] = rel_l2(buf, sd[name])
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(f"{REPORT_DIR}/parity_dropout_training_step_twin_encoder_{int(twin_encoder)}.txt", "w") as f:
        f.write(f"# training_step, dropout ON, twin encoder {twin_encoder}, twin post-net True; {len(rec.drops)} mask launches\n")
        f.write(f"# loss {lerr:.3e} (gate 1e-4); worst gradient {max(gerrs.values()):.3e} {max(gerrs, key=gerrs.get)} (gate {GRAD_GATE:g}); "
                f"worst running statistic {max(berrs.values()):.3e} {max(berrs, key=berrs.get)} (gate {GATE:g})\n")
        for k, v in sorted(gerrs.items(), key=lambda kv: -kv[1]):
            f.write(f"{v:.3e} grad/{k}\n")
        for k, v in sorted(berrs.items(), key=lambda kv: -kv[1]):
            f.write(f"{v:.3e} {k}\n")
    assert lerr < 1e-4, lerr
    assert all(v < GRAD_GATE for v in gerrs.values()), {k: v for k, v in gerrs.items() if not v < GRAD_GATE}
    assert all(v < GATE for v in berrs.values()), {k: v for k, v in berrs.items() if not v < GATE}
