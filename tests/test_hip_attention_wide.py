"""Attention for heads of 65 .. 128 columns (csrc/attention_wide.hip; ttts_attention_fwd_wide / ttts_attention_bwd_wide):
the kernels through the C ABI and through ops against fp64, peaked softmaxes against stock fp32 torch, the dropout mask
against its host restatement, the dropout-on model and the captured training step at head_dim 128, and what a
forward + backward allocates.  Measured worst errors: attention_wide_*.txt in REPORT_DIR, and DESIGN.md."""
import functools
import os
import types

import numpy as np
import pytest
import torch

from conftest import rel_l2
import test_hip_dropout_parity as parity      # (modules, not names: an imported test_* function would be collected here again)
import test_hip_graph as graph_tests
from test_hip_dropout_parity import REPORT_DIR, _t
from test_hip_ops import TOL, _dev, _g, _rand, _ref_attention

from oracle import dropmask as dm

pytestmark = pytest.mark.gpu

# tile edges of a 128-row block and of the 32-row stages, ragged ends, an utterance without keys, one key
CASES = {
    "causal200": dict(B=3, H=2, Tq=200, Tk=200, lens=[200, 131, 64], causal=True, packed=True),
    "cross150x70": dict(B=3, H=2, Tq=150, Tk=70, lens=[70, 33, 1], causal=False, packed=False),
    "cross33x129": dict(B=3, H=2, Tq=33, Tk=129, lens=[129, 128, 5], causal=False, packed=False),
    "cross5x9_nokeys": dict(B=2, H=2, Tq=5, Tk=9, lens=[9, 0], causal=False, packed=False),
    "self1": dict(B=2, H=2, Tq=1, Tk=1, lens=[1, 1], causal=True, packed=True),
    "self100": dict(B=2, H=2, Tq=100, Tk=100, lens=[100, 33], causal=False, packed=True),
}


def _report(name, lines):
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(f"{REPORT_DIR}/attention_wide_{name}.txt", "w") as f:
        f.write("\n".join(lines) + "\n")


def _ref(q_, kv_, do, lens, H, causal, keep=None):
    """fp64 on the CPU: (o (B,Tq,d), weights (B,H,Tq,Tk) after `keep` (a (B,H,Tq,Tk) multiplier, or None), dq, dkv); an
    utterance without keys gives zeros everywhere (the reference softmax has no answer there)"""
    B, Tq, d = q_.shape
    Tk, hd = kv_.shape[1], d // H
    qd, kvd = q_.double().requires_grad_(), kv_.double().requires_grad_()
    idx = (lens > 0).nonzero().flatten()
    q = qd[idx].view(len(idx), Tq, H, hd).transpose(1, 2)
    k, v = [t[idx].view(len(idx), Tk, H, hd).transpose(1, 2) for t in kvd.split(d, dim=-1)]
    _, a = _ref_attention(q, k, v, lens[idx], causal)
    if keep is not None:
        a = a * keep[idx]
    o = (a @ v).transpose(1, 2).reshape(len(idx), Tq, d)
    o.backward(do.double()[idx])
    ref_o, ref_a = torch.zeros(B, Tq, d, dtype=torch.float64), torch.zeros(B, H, Tq, Tk, dtype=torch.float64)
    ref_o[idx], ref_a[idx] = o.detach(), a.detach()
    return types.SimpleNamespace(o=ref_o, a=ref_a, dq=qd.grad, dkv=kvd.grad)


@functools.lru_cache(maxsize=None)
def _case(name, hd, qk_scale=1.0):
    """inputs (CPU fp32) and the fp64 reference of one case, computed once and shared (read-only)"""
    c = CASES[name]
    B, H, Tq, Tk = c["B"], c["H"], c["Tq"], c["Tk"]
    d, s = H * hd, 1000 * sorted(CASES).index(name) + hd
    q_, kv_, do = _rand(B, Tq, d, seed=s + 1), _rand(B, Tk, 2 * d, seed=s + 2), _rand(B, Tq, d, seed=s + 3)
    q_ = q_ * qk_scale
    kv_ = torch.cat([kv_[..., :d] * qk_scale, kv_[..., d:]], dim=-1)
    lens = torch.tensor(c["lens"], dtype=torch.int64)
    return types.SimpleNamespace(q=q_, kv=kv_, do=do, lens=lens, ref=_ref(q_, kv_, do, lens, H, c["causal"]),
                                 **{k: v for k, v in c.items() if k != "lens"})


def _abi(q_, kv_, do, lens, H, causal, packed, need_w, p=0.0, seed=0, ss=None):
    """head_dim 128 in place through ttts_attention_fwd_wide / ttts_attention_bwd_wide -> (o, attn or None, dq, dkv) on the CPU.
    `packed`: one (B, T, 3d) buffer read and one gradient buffer written with row stride 3d.  Every output starts as NaN."""
    from transformertts_amd import _lib
    from transformertts_amd.ops import _off, _p, _stream
    lib, dev = _lib.load(), _dev()
    B, Tq, d = q_.shape
    Tk = kv_.shape[1]
    assert d == H * 128
    nan = float("nan")
    if packed:
        buf = torch.cat([q_, kv_], dim=-1).to(dev)
        g = torch.full_like(buf, nan)
        ins, lds = [_off(buf, 0), _off(buf, d), _off(buf, 2 * d)], [3 * d] * 3
        outs, dq, dkv = [_off(g, 0), _off(g, d), _off(g, 2 * d)], g[..., :d], g[..., d:]
    else:
        q, kv = q_.to(dev), kv_.to(dev)
        dq, dkv = torch.full_like(q, nan), torch.full_like(kv, nan)
        ins, lds = [_p(q), _off(kv, 0), _off(kv, d)], [d, 2 * d, 2 * d]
        outs = [_p(dq), _off(dkv, 0), _off(dkv, d)]
    o = torch.full((B, Tq, d), nan, device=dev)
    stat = torch.full((2, B, H, Tq), nan, device=dev)
    attn = torch.full((B, H, Tq, Tk), nan, device=dev) if need_w else None
    delta = torch.empty(B, H, Tq, device=dev)
    lens_d, do_d = lens.to(dev), do.to(dev)
    scale, c = 128 ** -0.5, 1 if causal else 0
    _lib.check(lib.ttts_attention_fwd_wide(*ins, _p(o), _p(stat), _p(attn), _p(lens_d), B, H, Tq, Tk, *lds, d, c, scale, p, seed,
                                           ss, _stream()), "ttts_attention_fwd_wide")
    _lib.check(lib.ttts_attention_bwd_wide(*ins, _p(o), _p(do_d), _p(stat), _p(delta), *outs, _p(lens_d), B, H, Tq, Tk, *lds, d,
                                           *lds, c, scale, p, seed, ss, _stream()), "ttts_attention_bwd_wide")
    torch.cuda.synchronize()
    return o.cpu(), None if attn is None else attn.cpu(), dq.cpu(), dkv.cpu()


def _errors(got, ref, c, do):
    """worst-case figures of one run against the fp64 reference; asserts what is exact (an utterance without keys, one key)"""
    o, attn, dq, dkv = got
    for t in (o, dq, dkv) + (() if attn is None else (attn,)):
        assert bool(torch.isfinite(t).all())
    errs = {"o": rel_l2(o, ref.o), "dkv": rel_l2(dkv, ref.dkv)}
    if attn is not None:
        errs["attn"] = rel_l2(attn, ref.a)
    if c["Tk"] == 1:     # one key: the weights are constant 1 and dq is exactly zero in fp64 -- absolute bound instead
        assert dq.abs().max().item() < 1e-6 * do.abs().max().item()
    else:
        errs["dq"] = rel_l2(dq, ref.dq)
    for b, n in enumerate(c["lens"]):
        if attn is not None:
            assert float(attn[b, :, :, n:].abs().sum()) == 0.0          # zero mass on dead keys
        assert float(dkv[b, n:].abs().sum()) == 0.0
        if n == 0:       # an utterance without keys: exact zeros
            assert float(o[b].abs().sum()) == 0.0 and float(dq[b].abs().sum()) == 0.0 and float(dkv[b].abs().sum()) == 0.0
    return errs


# ============================================================================================ 1. the C ABI, head_dim 128 in place
@pytest.mark.parametrize("name", sorted(CASES))
def test_wide_kernels_through_the_c_abi_vs_fp64(name):
    c = _case(name, 128)
    lines, worst = [], 0.0
    for need_w in ((False,) if c.causal else (True, False)):
        errs = _errors(_abi(c.q, c.kv, c.do, c.lens, c.H, c.causal, c.packed, need_w), c.ref, CASES[name], c.do)
        lines.append(f"{name} weights={need_w}: " + " ".join(f"{k}={v:.3e}" for k, v in sorted(errs.items())))
        worst = max(worst, *errs.values())
    print("\n".join(lines))
    _report(f"abi_{name}", [f"# worst {worst:.3e} (gate {TOL:g})"] + lines)
    assert worst < TOL, lines


# ============================================================================================ 2. through ops
@pytest.mark.parametrize("hd", [128, 96, 72])
def test_wide_attention_through_ops_vs_fp64(hd):
    """in place (128), padded (96), padded with a width that is no multiple of 16 (72): AttentionFn, self_attention and
    cross_attention, with and without the weights"""
    from transformertts_amd import ops
    dev = _dev()
    lines, worst = [], 0.0
    for name in sorted(CASES):
        c = _case(name, hd)
        d = c.H * hd
        lens_d, do_d = c.lens.to(dev), c.do.to(dev)
        runs = []
        if c.packed:
            for via in ("fn", "self_attention"):
                qkv = _g(torch.cat([c.q, c.kv], dim=-1))
                if via == "fn":
                    out, w = ops.AttentionFn.apply(qkv, None, lens_d, c.H, c.causal, 0.0, 0, False)
                    assert w.numel() == 0
                else:
                    out = ops.self_attention(qkv, lens_d, c.H, c.causal, 0.0, 0)
                out.backward(do_d)
                runs.append((via, (out.detach().cpu(), None, qkv.grad[..., :d].cpu(), qkv.grad[..., d:].cpu())))
        else:
            for via, need_w in (("fn", True), ("cross_attention", True), ("cross_attention", False)):
                qg, kvg = _g(c.q), _g(c.kv)
                if via == "fn":
                    out, w = ops.AttentionFn.apply(qg, kvg, lens_d, c.H, False, 0.0, 0, need_w)
                else:
                    out, w = ops.cross_attention(qg, kvg, lens_d, c.H, 0.0, 0, need_w)
                    assert need_w or w is None or w.numel() == 0      # (no weights: nothing, as at 64 columns)
                out.backward(do_d)
                runs.append((f"{via} weights={need_w}", (out.detach().cpu(), w.cpu() if need_w else None, qg.grad.cpu(), kvg.grad.cpu())))
        for via, got in runs:
            errs = _errors(got, c.ref, CASES[name], c.do)
            lines.append(f"hd{hd} {name} {via}: " + " ".join(f"{k}={v:.3e}" for k, v in sorted(errs.items())))
            worst = max(worst, *errs.values())
    print("\n".join(lines))
    _report(f"ops_hd{hd}", [f"# worst {worst:.3e} (gate {TOL:g})"] + lines)
    assert worst < TOL, lines


# ============================================================================================ 3. peaked softmaxes
@pytest.mark.parametrize("name", ["causal200", "cross150x70"])
def test_peaked_softmax_no_worse_than_twice_stock_fp32(name):
    """q and k scaled by 6 (scores of standard deviation 36: most rows are one-hot in fp32).  No flat gate: every figure at
    most twice what stock fp32 torch (ops.masked_attention, autograd) leaves against fp64 on the same inputs, and never above
    1e-4."""
    from transformertts_amd import ops
    dev = _dev()
    c = _case(name, 128, 6.0)
    d = c.H * 128
    lens_d, do_d = c.lens.to(dev), c.do.to(dev)

    def run(kernel):
        qg, kvg = _g(c.q), _g(c.kv)
        if kernel and c.packed:
            qkv = torch.cat([qg, kvg], dim=-1)
            out, w = ops.self_attention(qkv, lens_d, c.H, c.causal, 0.0, 0), None
        elif kernel:
            out, w = ops.cross_attention(qg, kvg, lens_d, c.H, 0.0, 0, True)
        else:
            out, w = ops.masked_attention(qg, kvg[..., :d], kvg[..., d:], lens_d, c.H, c.causal, 0.0)
            w = None if c.packed else w.detach()
        out.backward(do_d)
        errs = {"o": rel_l2(out, c.ref.o), "dq": rel_l2(qg.grad, c.ref.dq), "dkv": rel_l2(kvg.grad, c.ref.dkv)}
        if w is not None:
            errs["attn"] = rel_l2(w, c.ref.a)
        return errs

    stock, kern = run(False), run(True)
    lines = [f"{name} x6 {k}: kernels {kern[k]:.3e}  stock fp32 torch {stock[k]:.3e}" for k in sorted(kern)]
    print("\n".join(lines))
    _report(f"peaked_{name}", lines)
    bad = {k: (kern[k], stock[k]) for k in kern if not (kern[k] <= 2.0 * stock[k] and kern[k] <= 1e-4)}
    assert not bad, bad


# ============================================================================================ 4. the mask is the library's
@pytest.mark.parametrize("word", [None, 0x0F1E2D3C4B5A6978])
def test_wide_dropout_mask_is_keep_attn(word):
    """cross-attention weights at p = 0.25 are non-zero exactly at keep_attn & live and equal the p = 0 weights x drop_scale;
    causal self-attention (weights never returned) against the fp64 reference that drops by keep_attn.  `word`: under a
    StepState whose seed word the kernels XOR into the site seed."""
    import contextlib
    from transformertts_amd import ops
    dev = _dev()
    st = contextlib.nullcontext()
    if word is not None:
        st = ops.StepState(dev)
        st.push(seed=word, lr=0.0, p_tf=1.0, step=1)
    B, H, Tq, Tk, p, seed = 2, 2, 70, 23, 0.25, 0x0123456789ABCDEF
    d = H * 128
    q_, kv_ = _rand(B, Tq, d, seed=1), _rand(B, Tk, 2 * d, seed=2)
    lens = torch.tensor([23, 9], dtype=torch.int64)
    keep = _t(dm.keep_attn(dm.site_seed(seed, word), B * H * Tq, Tk, p), B, H, Tq, Tk)
    live = (torch.arange(Tk).view(1, 1, 1, Tk) < lens.view(B, 1, 1, 1)).expand(B, H, Tq, Tk)
    with torch.no_grad(), st:
        _, a0 = ops.cross_attention(q_.to(dev), kv_.to(dev), lens.to(dev), H, 0.0, 0, True)
        _, a1 = ops.cross_attention(q_.to(dev), kv_.to(dev), lens.to(dev), H, p, seed, True)
    a0, a1 = a0.cpu(), a1.cpu()
    assert bool((a0[live] > 0).all())
    assert torch.equal(a1 != 0, keep & live), int(((a1 != 0) != (keep & live)).sum())
    e_w = rel_l2(a1, a0.double() * keep * dm.drop_scale(p))
    assert e_w < 1e-6
    if word is not None:          # and the word matters
        assert not np.array_equal(keep.numpy().ravel(), dm.keep_attn(seed, B * H * Tq, Tk, p).ravel())

    T, seed2 = 70, 0xFEDCBA9876543210
    lens2 = torch.tensor([70, 31], dtype=torch.int64)
    qkv, do = _rand(B, T, 3 * d, seed=3), _rand(B, T, d, seed=4)
    keep2 = _t(dm.keep_attn(dm.site_seed(seed2, word), B * H * T, T, p), B, H, T, T).double() * dm.drop_scale(p)
    ref = _ref(qkv[..., :d], qkv[..., d:], do, lens2, H, True, keep2)
    qg = _g(qkv)
    with st:
        out = ops.self_attention(qg, lens2.to(dev), H, True, p, seed2)
        out.backward(do.to(dev))
    errs = {"o": rel_l2(out, ref.o), "dqkv": rel_l2(qg.grad, torch.cat([ref.dq, ref.dkv], dim=-1))}
    _report("dropout" + ("_stepstate" if word is not None else ""),
            [f"cross weights vs p=0 weights x keep x scale: {e_w:.3e} (gate 1e-6)"] + [f"causal self p=0.25 {k}: {v:.3e} (gate {TOL:g})" for k, v in errs.items()])
    assert max(errs.values()) < TOL, errs


# ============================================================================================ 5. the model, dropout on
@pytest.mark.parametrize("word", [None, 0x0F1E2D3C4B5A6978])
def test_wide_model_dropout_on_vs_oracle(word):
    """tiny1h (d_model 128, one head of 128 columns): every attention site is observed and restated by oracle.dropmask; outputs,
    alignments, loss, BatchNorm statistics and every gradient at that test's own gates"""
    parity.test_dropout_on_forward_backward_vs_oracle("tiny1h", 3, 12, 40, 18, 28, word)


# ============================================================================================ 6. graph replay
def test_wide_graph_replay_equals_eager_bitwise():
    """a captured TrainStep of tiny1h replays the eager steps bit for bit: the masks of the wide attention sites come from the
    (site seed, step word) hash, which a replay reads from device memory like every other site.  (With these sites on
    ops.masked_attention -- torch's generator -- the same comparison fails at the first per-step loss.)"""
    graph_tests.test_graph_replay_equals_eager_bitwise("tiny1h", 3, 12, 40, 150)


# ============================================================================================ 7. memory
def test_wide_attention_keeps_no_score_matrix():
    """causal self-attention without weights, B=2, H=2, T=1024, head_dim 128: forward + backward allocate o, the row statistics,
    delta and dqkv (about 10 MB) -- less than ONE (B, H, T, T) fp32 score matrix (16.8 MB)"""
    from transformertts_amd import ops
    dev = _dev()
    B, H, T, hd = 2, 2, 1024, 128
    d = H * hd
    qkv, do = _g(_rand(B, T, 3 * d, seed=1)), _rand(B, T, d, seed=2).to(dev)
    lens = torch.tensor([T, 700], dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = ops.self_attention(qkv, lens, H, True, 0.0, 0)
    out.backward(do)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(qkv.grad).all())
    print(f"peak {peak} bytes, one score matrix {B * H * T * T * 4} bytes")
    _report("memory", [f"forward + backward peak {peak} bytes; one (B,H,T,T) fp32 score matrix {B * H * T * T * 4} bytes"])
    assert peak < B * H * T * T * 4, peak
