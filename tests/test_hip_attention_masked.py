"""Attention under masks that are tensors -- a key-padding mask with holes, a `memory_mask`, a `tgt_mask` / `mask` that is not
the causal one -- on the masked forms of the 128-column kernels (csrc/attention_wide.hip; ttts_attention_fwd_wide_masked /
ttts_attention_bwd_wide_masked; ops.self_attention / ops.cross_attention with `dead` / `add_mask`): the kernels through the C ABI
and through ops against fp64, peaked softmaxes against stock fp32 torch, the dropout mask against its host restatement, the
layers, a captured forward + backward against the eager call, and what a forward + backward allocates.
Measured worst errors: attention_masked_*.txt in REPORT_DIR, and DESIGN.md 15."""
import contextlib
import functools
import os
import types

import pytest
import torch

from conftest import rel_l2
import test_hip_masks as masks            # (modules, not names: an imported test_* function would be collected here again)
from test_hip_dropout_parity import REPORT_DIR, _t
from test_hip_ops import TOL, _dev, _g, _rand

from oracle import dropmask as dm

pytestmark = pytest.mark.gpu
NEG_INF = float("-inf")

# The shapes sit on the edges of the 128-row query block (200 = 128 + 72, 161 = 128 + 33, 150), of the 32-row stages (70, 161) and
# of the mask-row padding (Tk 70 and 161 and 1 are no multiples of 4).  `mask`: "bh" a float mask per (batch, head), "2d" one
# shared float mask, "band" one shared bool band of half-width 20; float masks hold U(-4, 4) with `forbid` of the entries -inf and
# query row 7 forbidden altogether.  `dead`: share of dead keys per utterance; `last_dead`: the last utterance's keys all dead as
# well; `tail_dead`: its keys from that index on (the queries whose band lies behind it have no key).
CASES = {
    "self200": dict(B=2, H=2, Tq=200, Tk=200, hd=128, causal=True, packed=True, weights=False, mask="bh", forbid=0.3, dead=0.3),
    "cross150x70": dict(B=2, H=2, Tq=150, Tk=70, hd=96, causal=False, packed=False, weights=True, mask="2d", forbid=0.3, dead=0.3),
    "band200": dict(B=2, H=2, Tq=200, Tk=200, hd=64, causal=False, packed=True, weights=True, mask="band", dead=0.1, tail_dead=150),
    "self161": dict(B=3, H=2, Tq=161, Tk=161, hd=16, causal=True, packed=True, weights=False, mask=None, dead=0.3, last_dead=True),
    "self1": dict(B=2, H=2, Tq=1, Tk=1, hd=128, causal=True, packed=True, weights=False, mask=None, dead=0.0, last_dead=True),
    "cross5x1": dict(B=2, H=2, Tq=5, Tk=1, hd=128, causal=False, packed=False, weights=True, mask="2d", forbid=0.0, dead=0.0,
                     last_dead=True),
}


def _report(name, lines):
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(f"{REPORT_DIR}/attention_masked_{name}.txt", "w") as f:
        f.write("\n".join(lines) + "\n")


def _masks(c, seed=3):
    """-> (dead (B, Tk) bool or None, add_mask as a caller would pass it or None, allowed (B, H, Tq, Tk) bool, add (B, H, Tq, Tk)
    fp64: what is added to the allowed scores)"""
    B, H, Tq, Tk = c["B"], c["H"], c["Tq"], c["Tk"]
    g = torch.Generator().manual_seed(seed)
    dead = torch.rand(B, Tk, generator=g) < c["dead"]
    if c.get("last_dead"):
        dead[-1] = True
    if c.get("tail_dead"):
        dead[-1, c["tail_dead"]:] = True
    allowed = ~dead[:, None, None, :].expand(B, H, Tq, Tk).clone()
    add = torch.zeros(B, H, Tq, Tk, dtype=torch.float64)
    add_mask = None
    if c["mask"] == "band":
        add_mask = (torch.arange(Tq)[:, None] - torch.arange(Tk)[None, :]).abs() > 20
        allowed &= ~add_mask
    elif c["mask"] is not None:
        shape = (B * H, Tq, Tk) if c["mask"] == "bh" else (Tq, Tk)
        add_mask = torch.rand(shape, generator=g) * 8 - 4
        add_mask = add_mask.masked_fill(torch.rand(shape, generator=g) < c["forbid"], NEG_INF)
        add_mask[..., min(7, Tq - 1), :] = NEG_INF
        full = add_mask.reshape(B, H, Tq, Tk) if c["mask"] == "bh" else add_mask.expand(B, H, Tq, Tk)
        allowed &= ~torch.isneginf(full)
        add = full.masked_fill(torch.isneginf(full), 0).double()
    if c["causal"]:
        allowed &= ~torch.triu(torch.ones(Tq, Tk, dtype=torch.bool), diagonal=1)
    return (dead if bool(dead.any()) else None), add_mask, allowed, add


def _ref(q_, kv_, do, H, allowed, add, keep=None):
    """fp64 on the CPU: softmax over the allowed keys of q.k / sqrt(head_dim) + add; a row without an allowed key gives zeros (the
    reference softmax has no answer there).  `keep`: a (B, H, Tq, Tk) multiplier of the weights (dropout), or None."""
    B, Tq, d = q_.shape
    Tk, hd = kv_.shape[1], d // H
    qd, kvd = q_.double().requires_grad_(), kv_.double().requires_grad_()
    q = qd.view(B, Tq, H, hd).transpose(1, 2)
    k, v = [t.view(B, Tk, H, hd).transpose(1, 2) for t in kvd.split(d, dim=-1)]
    has_key = allowed.any(dim=-1, keepdim=True)
    s = ((q * hd ** -0.5) @ k.transpose(-1, -2) + add).masked_fill(~allowed, NEG_INF)
    a = torch.softmax(torch.where(has_key, s, torch.zeros_like(s)), dim=-1) * has_key
    if keep is not None:
        a = a * keep
    o = (a @ v).transpose(1, 2).reshape(B, Tq, d)
    o.backward(do.double())
    return types.SimpleNamespace(o=o.detach(), a=a.detach(), dq=qd.grad, dkv=kvd.grad)


@functools.lru_cache(maxsize=None)
def _case(name, hd=None, qk_scale=1.0):
    """inputs (CPU fp32), masks and the fp64 reference of one case, computed once and shared (read-only)"""
    c = dict(CASES[name])
    c["hd"] = hd or c["hd"]
    B, H, Tq, Tk, d = c["B"], c["H"], c["Tq"], c["Tk"], c["H"] * c["hd"]
    s = 1000 * sorted(CASES).index(name) + c["hd"]
    q_, kv_, do = _rand(B, Tq, d, seed=s + 1), _rand(B, Tk, 2 * d, seed=s + 2), _rand(B, Tq, d, seed=s + 3)
    q_ = q_ * qk_scale
    kv_ = torch.cat([kv_[..., :d] * qk_scale, kv_[..., d:]], dim=-1)
    if c["packed"]:                     # self-attention: one packed projection, do over the same rows
        assert Tq == Tk
    dead, add_mask, allowed, add = _masks(c)
    # no case passes on an empty mask: a share of the entries is allowed, and at least one row has no key at all
    share = allowed.float().mean().item()
    no_key = ~allowed.any(dim=-1)
    assert 0.1 <= share <= 0.6, (name, share)
    assert int(no_key.sum()) >= 1, name
    return types.SimpleNamespace(q=q_, kv=kv_, do=do, dead=dead, add_mask=add_mask, allowed=allowed, add=add, no_key=no_key,
                                 share=share, d=d, ref=_ref(q_, kv_, do, H, allowed, add),
                                 **{k: v for k, v in c.items() if k != "dead"})


def _lens(c, dev):
    return torch.full((c.B,), c.Tk, dtype=torch.int64, device=dev)


def _errors(got, c, ref=None):
    """worst-case figures of one run against the fp64 reference; asserts what is exact: rows without a key, dead keys"""
    ref = ref or c.ref
    o, attn, dq, dkv = got
    for t in (o, dq, dkv) + (() if attn is None else (attn,)):
        assert bool(torch.isfinite(t).all())
    errs = {"o": rel_l2(o, ref.o), "dkv": rel_l2(dkv, ref.dkv)}
    if attn is not None:
        errs["attn"] = rel_l2(attn, ref.a)
        assert float(attn[~c.allowed].abs().sum()) == 0.0                       # zero mass where the masks forbid
        assert float(attn[c.no_key].abs().sum()) == 0.0
    if c.Tk == 1:        # one key: the weights are constant 0 / 1 and dq is exactly zero in fp64 -- absolute bound instead
        assert dq.abs().max().item() < 1e-6 * c.do.abs().max().item()
    else:
        errs["dq"] = rel_l2(dq, ref.dq)
    # a row without an allowed key: exact zeros in o and dq (every head's columns of that row)
    rows = c.no_key.transpose(1, 2)[..., None].expand(c.B, c.Tq, c.H, c.hd).reshape(c.B, c.Tq, c.d)
    assert float(o[rows].abs().sum()) == 0.0 and float(dq[rows].abs().sum()) == 0.0
    # a key no query is allowed to see: exact zeros in dk and dv
    unseen = ~c.allowed.any(dim=2)                                              # (B, H, Tk)
    cols = unseen.transpose(1, 2)[..., None].expand(c.B, c.Tk, c.H, c.hd).reshape(c.B, c.Tk, c.d)
    assert float(dkv[..., :c.d][cols].abs().sum()) == 0.0 and float(dkv[..., c.d:][cols].abs().sum()) == 0.0
    return errs


def _mask_abi(c, dev):
    """the six mask arguments of the C ABI for case c, and the tensors that own the memory"""
    from transformertts_amd import ops
    dead = None if c.dead is None else c.dead.to(dev)
    m4 = None if c.add_mask is None else ops._mask_operand(c.add_mask.to(dev), c.B, c.H, c.Tq, c.Tk)
    args = ops._mask_args(dead, m4, c.Tk)
    if m4 is not None:
        assert args[1] % 4 == 0 and args[1] >= c.Tk and m4.data_ptr() % 16 == 0
    return args, (dead, m4)


def _abi(c, need_w, p=0.0, seed=0, ss=None):
    """head_dim 128 in place through ttts_attention_fwd_wide_masked / ttts_attention_bwd_wide_masked -> (o, attn or None, dq, dkv)
    on the CPU.  `packed`: one (B, T, 3d) buffer read and one gradient buffer written with row stride 3d.  Every output starts
    as NaN."""
    from transformertts_amd import _lib
    from transformertts_amd.ops import _off, _p, _stream
    lib, dev = _lib.load(), _dev()
    B, H, Tq, Tk, d = c.B, c.H, c.Tq, c.Tk, c.d
    assert c.hd == 128
    nan = float("nan")
    if c.packed:
        buf = torch.cat([c.q, c.kv], dim=-1).to(dev)
        g = torch.full_like(buf, nan)
        ins, lds = [_off(buf, 0), _off(buf, d), _off(buf, 2 * d)], [3 * d] * 3
        outs, dq, dkv = [_off(g, 0), _off(g, d), _off(g, 2 * d)], g[..., :d], g[..., d:]
    else:
        q, kv = c.q.to(dev), c.kv.to(dev)
        dq, dkv = torch.full_like(q, nan), torch.full_like(kv, nan)
        ins, lds = [_p(q), _off(kv, 0), _off(kv, d)], [d, 2 * d, 2 * d]
        outs = [_p(dq), _off(dkv, 0), _off(dkv, d)]
    o = torch.full((B, Tq, d), nan, device=dev)
    stat = torch.full((2, B, H, Tq), nan, device=dev)
    attn = torch.full((B, H, Tq, Tk), nan, device=dev) if need_w else None
    delta = torch.empty(B, H, Tq, device=dev)
    lens_d, do_d = _lens(c, dev), c.do.to(dev)
    margs, owners = _mask_abi(c, dev)
    scale, cz = 128 ** -0.5, 1 if c.causal else 0
    _lib.check(lib.ttts_attention_fwd_wide_masked(*ins, _p(o), _p(stat), _p(attn), _p(lens_d), B, H, Tq, Tk, *lds, d, cz, scale, p,
                                                  seed, ss, *margs, _stream()), "ttts_attention_fwd_wide_masked")
    _lib.check(lib.ttts_attention_bwd_wide_masked(*ins, _p(o), _p(do_d), _p(stat), _p(delta), *outs, _p(lens_d), B, H, Tq, Tk, *lds,
                                                  d, *lds, cz, scale, p, seed, ss, *margs, _stream()),
               "ttts_attention_bwd_wide_masked")
    torch.cuda.synchronize()
    # rows without a key: m = 0 and l = 0 in the row statistics
    stat = stat.cpu()
    assert float(stat[0][c.no_key].abs().sum()) == 0.0 and float(stat[1][c.no_key].abs().sum()) == 0.0
    assert bool((stat[1][~c.no_key] > 0).all())
    del owners
    return o.cpu(), None if attn is None else attn.cpu(), dq.cpu(), dkv.cpu()


def _ops_run(c, need_w, p=0.0, seed=0, kernel=True):
    """through ops.self_attention / ops.cross_attention (kernel) or ops.masked_attention -> (o, attn or None, dq, dkv) on the CPU"""
    from transformertts_amd import ops
    dev = _dev()
    dead = None if c.dead is None else c.dead.to(dev)
    add_mask = None if c.add_mask is None else c.add_mask.to(dev)
    lens_d, do_d, d = _lens(c, dev), c.do.to(dev), c.d
    qg, kvg = _g(c.q), _g(c.kv)
    if not kernel:
        am = None if add_mask is None else ops._mask_operand(add_mask, c.B, c.H, c.Tq, c.Tk).clamp_min(torch.finfo(torch.float32).min)
        out, w = ops.masked_attention(qg, kvg[..., :d], kvg[..., d:], lens_d, c.H, c.causal, p, dead, am)
    elif c.packed and not need_w:
        out, w = ops.self_attention(torch.cat([qg, kvg], dim=-1), lens_d, c.H, c.causal, p, seed, dead=dead, add_mask=add_mask), None
    elif c.packed:
        out, w = ops.AttentionFn.apply(torch.cat([qg, kvg], dim=-1), None, lens_d, c.H, c.causal, p, seed, True, None, None, None,
                                       dead, add_mask)
    else:
        out, w = ops.cross_attention(qg, kvg, lens_d, c.H, p, seed, need_w, dead=dead, add_mask=add_mask)
    out.backward(do_d)
    return out.detach().cpu(), (w.detach().cpu() if need_w else None), qg.grad.cpu(), kvg.grad.cpu()


# ============================================================================================ a. the C ABI and ops against fp64
@pytest.mark.parametrize("name", sorted(CASES))
def test_masked_kernels_through_the_c_abi_vs_fp64(name):
    """every case's masks at head_dim 128, in place"""
    c = _case(name, 128)
    lines, worst = [f"# {name}: allowed share {c.share:.3f}, rows without a key {int(c.no_key.sum())} of {c.no_key.numel()}"], 0.0
    for need_w in ((False,) if c.causal else (True, False)):
        errs = _errors(_abi(c, need_w), c)
        lines.append(f"{name} weights={need_w}: " + " ".join(f"{k}={v:.3e}" for k, v in sorted(errs.items())))
        worst = max(worst, *errs.values())
    print("\n".join(lines))
    _report(f"abi_{name}", [f"# worst {worst:.3e} (gate {TOL:g})"] + lines)
    assert worst < TOL, lines


@pytest.mark.parametrize("name", sorted(CASES))
def test_masked_attention_through_ops_vs_fp64(name):
    """every case at its own head_dim (128 in place; 96, 64 and 16 padded to 128): self_attention / cross_attention, with and
    without the weights"""
    c = _case(name)
    lines, worst = [f"# {name} hd{c.hd}: allowed share {c.share:.3f}, rows without a key {int(c.no_key.sum())} of {c.no_key.numel()}"], 0.0
    for need_w in ((False,) if c.causal else (True, False)):
        errs = _errors(_ops_run(c, need_w), c)
        lines.append(f"{name} hd{c.hd} weights={need_w}: " + " ".join(f"{k}={v:.3e}" for k, v in sorted(errs.items())))
        worst = max(worst, *errs.values())
    print("\n".join(lines))
    _report(f"ops_{name}", [f"# worst {worst:.3e} (gate {TOL:g})"] + lines)
    assert worst < TOL, lines


# ============================================================================================ b. peaked softmaxes
@pytest.mark.parametrize("name", ["self200", "cross150x70"])
def test_masked_peaked_softmax_no_worse_than_twice_stock_fp32(name):
    """q and k scaled by 6 (scores of standard deviation 36: most rows are one-hot in fp32).  No flat gate: every figure at most
    twice what stock fp32 torch (ops.masked_attention, autograd) leaves against fp64 on the same inputs and masks, and never
    above 1e-4."""
    c = _case(name, None, 6.0)

    def run(kernel):
        o, w, dq, dkv = _ops_run(c, c.weights, kernel=kernel)
        errs = {"o": rel_l2(o, c.ref.o), "dq": rel_l2(dq, c.ref.dq), "dkv": rel_l2(dkv, c.ref.dkv)}
        if w is not None:
            errs["attn"] = rel_l2(w, c.ref.a)
        return errs

    stock, kern = run(False), run(True)
    lines = [f"{name} x6 {k}: kernels {kern[k]:.3e}  stock fp32 torch {stock[k]:.3e}" for k in sorted(kern)]
    print("\n".join(lines))
    _report(f"peaked_{name}", lines)
    bad = {k: (kern[k], stock[k]) for k in kern if not (kern[k] <= 2.0 * stock[k] and kern[k] <= 1e-4)}
    assert not bad, bad


# ============================================================================================ c. the mask is the library's
class _Drops:
    """records the dropout launches (ops._drop_observer) of what runs inside"""

    def __enter__(self):
        from transformertts_amd import ops
        self.drops = []
        ops._drop_observer = lambda *rec: self.drops.append(rec)
        return self

    def __exit__(self, *exc):
        from transformertts_amd import ops
        ops._drop_observer = None


@pytest.mark.parametrize("word", [None, 0x0F1E2D3C4B5A6978])
@pytest.mark.parametrize("name", ["band200", "self161"])
def test_masked_dropout_mask_is_keep_attn(name, word):
    """p = 0.25: the returned weights are non-zero exactly at keep_attn & allowed and equal the p = 0 weights x drop_scale; o and
    the gradients against the fp64 reference that drops by keep_attn; one observed `attn` site per masked attention.  The causal
    case returns no weights from its own kernel form: its weights are read from the non-causal form given the causal pattern as
    a bool mask (the same allowed set, the same row ids).  `word`: under a StepState whose seed word the kernels XOR into the
    site seed.
    band200 is the case that caught the dK/dV kernel reading the last register of its dP accumulator too early (DESIGN.md 15,
    "A read that came too early"): a band leaves waves whose low query rows are all forbidden, and only dropout uses that
    early read."""
    from transformertts_amd import ops
    dev = _dev()
    c = _case(name)
    st = contextlib.nullcontext()
    if word is not None:
        st = ops.StepState(dev)
        st.push(seed=word, lr=0.0, p_tf=1.0, step=1)
    B, H, T, p, seed = c.B, c.H, c.Tq, 0.25, 0x0123456789ABCDEF
    keep = _t(dm.keep_attn(dm.site_seed(seed, word), B * H * T, T, p), B, H, T, T)
    dead = c.dead.to(dev)
    if c.causal:
        wmask = torch.triu(torch.ones(T, T, dtype=torch.bool, device=dev), diagonal=1)
    else:
        wmask = c.add_mask.to(dev)
    qkv = torch.cat([c.q, c.kv], dim=-1).to(dev)
    with torch.no_grad(), st, _Drops() as seen:
        _, a0 = ops.AttentionFn.apply(qkv, None, _lens(c, dev), H, False, 0.0, 0, True, None, None, None, dead, wmask)
        _, a1 = ops.AttentionFn.apply(qkv, None, _lens(c, dev), H, False, p, seed, True, None, None, None, dead, wmask)
    assert seen.drops == [("attn", seed, p, (B * H * T, T), None)], seen.drops
    a0, a1 = a0.cpu(), a1.cpu()
    assert bool((a0[c.allowed] > 0).all()) and float(a0[~c.allowed].abs().sum()) == 0.0
    share = (keep & c.allowed).float().mean().item()
    assert torch.equal(a1 != 0, keep & c.allowed), int(((a1 != 0) != (keep & c.allowed)).sum())
    assert abs(share - (1 - p) * c.share) < 0.01                     # (and that set is what the hash and the masks leave)
    e_w = rel_l2(a1, a0.double() * keep * dm.drop_scale(p))
    assert e_w < 1e-6

    # o and the gradients of the case's own form under that mask
    ref = _ref(c.q, c.kv, c.do, H, c.allowed, c.add, keep.double() * dm.drop_scale(p))
    with st, _Drops() as seen:
        got = _ops_run(c, False, p, seed)
    assert seen.drops == [("attn", seed, p, (B * H * T, T), None)], seen.drops
    errs = _errors(got, c, ref)
    _report(f"dropout_{name}" + ("_stepstate" if word is not None else ""),
            [f"kept and allowed share {share:.3f}", f"weights vs p=0 weights x keep x scale: {e_w:.3e} (gate 1e-6)"] +
            [f"p=0.25 {k}: {v:.3e} (gate {TOL:g})" for k, v in sorted(errs.items())])
    assert max(errs.values()) < TOL, errs


# ============================================================================================ d. the layers
def _layer_masks(B, Tq, Tk, g):
    tgt_kpm = masks._holes(B, Tq, [37, 30, 21], 3, g)
    mem_kpm = masks._holes(B, Tk, [29, 17, 8], 2, g)
    mem_mask = (torch.arange(Tq)[:, None] * Tk // Tq - torch.arange(Tk)[None, :]).abs() > 5       # a band along the diagonal
    return tgt_kpm, mem_kpm, mem_mask


def test_masked_decoder_layer_draws_the_library_masks():
    """dropout 0.1, train mode, a band `memory_mask` and key-padding masks with holes: both attentions draw their masks from the
    library's hash (one observed `attn` site each, with seeds from ops.seeds) and none from torch's generator"""
    from transformertts_amd import ops
    from transformertts_amd.model import layers as L
    d, h, ff, B, Tq, Tk = 128, 2, 256, 3, 37, 29
    torch.manual_seed(11)
    layer = L.TransformerDecoderLayer(d, h, ff, dropout=0.1).cuda().train()
    g = torch.Generator().manual_seed(5)
    tgt, mem = torch.randn(B, Tq, d, generator=g).cuda(), torch.randn(B, Tk, d, generator=g).cuda()
    tgt_kpm, mem_kpm, mem_mask = _layer_masks(B, Tq, Tk, g)
    ops.seeds.manual_seed(1234)
    state = torch.cuda.get_rng_state()
    try:
        with _Drops() as seen:
            y, w = layer(tgt, mem, memory_mask=mem_mask.cuda(), tgt_key_padding_mask=tgt_kpm.cuda(),
                         memory_key_padding_mask=mem_kpm.cuda(), tgt_is_causal=True)
    finally:
        ops.seeds.follow_torch()
    attn = [r for r in seen.drops if r[0] == "attn"]
    assert [r[3] for r in attn] == [(B * h * Tq, Tq), (B * h * Tq, Tk)], seen.drops
    assert len({r[1] for r in seen.drops}) == len(seen.drops)                     # every site its own seed
    assert torch.equal(torch.cuda.get_rng_state(), state)                        # torch's generator drew nothing
    assert bool(torch.isfinite(y).all()) and w.shape == (B, h, Tq, Tk)
    # the returned alignments are the post-dropout weights under the site's mask: zero wherever the masks forbid
    allowed = ~(mem_mask[None, None] | mem_kpm[:, None, None, :]).expand(B, h, Tq, Tk)
    keep = _t(dm.keep_attn(attn[1][1], B * h * Tq, Tk, 0.1), B, h, Tq, Tk)
    assert torch.equal(w.cpu() != 0, keep & allowed)


def test_masked_layers_match_torch_on_the_kernels(monkeypatch):
    """dropout 0: the comparisons of tests/test_hip_masks.py (torch's own layers in fp64, its gate) hold with every masked
    attention on the kernels -- counted at the launchers -- and none in ops.masked_attention"""
    from transformertts_amd import ops
    calls = {"kernels": 0, "algebra": 0}
    fwd, algebra = ops._attn_wide_fwd, ops.masked_attention

    def count_fwd(*a, mask=None):
        calls["kernels"] += mask is not None          # the masked entry point: the one launcher takes both forms
        return fwd(*a, mask=mask)

    def count_algebra(*a, **k):
        calls["algebra"] += 1
        return algebra(*a, **k)
    monkeypatch.setattr(ops, "_attn_wide_fwd", count_fwd)
    monkeypatch.setattr(ops, "masked_attention", count_algebra)
    masks.test_decoder_layer_with_arbitrary_masks_matches_torch(False)
    assert calls == {"kernels": 2, "algebra": 0}, calls
    masks.test_decoder_layer_with_arbitrary_masks_matches_torch(True)
    assert calls == {"kernels": 4, "algebra": 0}, calls
    masks.test_encoder_with_mask_and_holes_matches_torch()
    assert calls == {"kernels": 6, "algebra": 0}, calls


# ============================================================================================ e. graph replay
def test_masked_attention_graph_replay_equals_eager_bitwise():
    """forward + backward of ops.self_attention and ops.cross_attention with masks, p = 0.1, under a step state, captured into one
    HIP graph: a replay equals the eager call bit for bit on o, the weights and every gradient, for the captured step word and
    for another one (the masks come from the (site seed, step word) hash, read from device memory; no host read, nothing from
    torch's generator)"""
    from transformertts_amd import ops
    dev = _dev()
    cs, cc = _case("band200"), _case("cross150x70")
    p, seeds = 0.1, (0x1111222233334444, 0x5555666677778888)
    st = ops.StepState(dev)
    ins = dict(qkv=torch.cat([cs.q, cs.kv], dim=-1).to(dev).requires_grad_(), do_s=cs.do.to(dev), dead_s=cs.dead.to(dev),
               mask_s=cs.add_mask.to(dev), lens_s=_lens(cs, dev),
               q=cc.q.to(dev).requires_grad_(), kv=cc.kv.to(dev).requires_grad_(), do_c=cc.do.to(dev), dead_c=cc.dead.to(dev),
               mask_c=cc.add_mask.to(dev), lens_c=_lens(cc, dev))

    def step():
        for t in (ins["qkv"], ins["q"], ins["kv"]):
            t.grad = None
        o_s = ops.self_attention(ins["qkv"], ins["lens_s"], cs.H, False, p, seeds[0], dead=ins["dead_s"], add_mask=ins["mask_s"])
        o_c, w = ops.cross_attention(ins["q"], ins["kv"], ins["lens_c"], cc.H, p, seeds[1], True, dead=ins["dead_c"],
                                     add_mask=ins["mask_c"])
        o_s.backward(ins["do_s"])
        o_c.backward(ins["do_c"])
        return [o_s.detach(), o_c.detach(), w.detach(), ins["qkv"].grad, ins["q"].grad, ins["kv"].grad]

    words = (0x0F1E2D3C4B5A6978, 0x7766554433221100)
    with st:
        st.push(seed=words[0], lr=0.0, p_tf=1.0, step=1)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()                                                   # warm-up off the capturing stream
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            captured = step()
        for n, word in enumerate(words):
            st.push(seed=word, lr=0.0, p_tf=1.0, step=n + 1)
            graph.replay()
            torch.cuda.synchronize()
            replayed = [t.clone() for t in captured]
            eager = [t.clone() for t in step()]
            for name, a, b in zip(("o self", "o cross", "weights", "dqkv", "dq", "dkv"), replayed, eager):
                assert torch.equal(a, b), (name, hex(word))
            if n == 0:
                first = replayed
        assert not torch.equal(first[2], replayed[2])                # and the step word matters


# ============================================================================================ f. memory
def test_masked_attention_keeps_no_score_matrix():
    """causal self-attention B=2, H=2, T=1024, head_dim 128 with dead keys and a shared 2-D mask: forward + backward allocate o,
    the row statistics, the lengths, delta and dqkv (about 10 MB) -- less than ONE (B, H, T, T) fp32 score matrix (16.8 MB).  The
    shared mask (4 MB) is the caller's and is used in place."""
    from transformertts_amd import ops
    dev = _dev()
    B, H, T, hd = 2, 2, 1024, 128
    d = H * hd
    qkv, do = _g(_rand(B, T, 3 * d, seed=1)), _rand(B, T, d, seed=2).to(dev)
    g = torch.Generator().manual_seed(3)
    dead = (torch.rand(B, T, generator=g) < 0.3).to(dev)
    mask = (torch.rand(T, T, generator=g) * 8 - 4).masked_fill(torch.rand(T, T, generator=g) < 0.3, NEG_INF).to(dev)
    lens = torch.full((B,), T, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = ops.self_attention(qkv, lens, H, True, 0.0, 0, dead=dead, add_mask=mask)
    out.backward(do)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(qkv.grad).all())
    print(f"peak {peak} bytes, one score matrix {B * H * T * T * 4} bytes")
    _report("memory", [f"forward + backward peak {peak} bytes; one (B,H,T,T) fp32 score matrix {B * H * T * T * 4} bytes"])
    assert peak < B * H * T * T * 4, peak
