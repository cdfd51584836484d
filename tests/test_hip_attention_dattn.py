"""Differentiable attention weights on the 128-column kernels (csrc/attention_wide.hip DATTN forms; ttts_attention_bwd_wide_dattn;
ops.cross_attention(..., weights_grad=True)): the gradients of a loss on the context AND on the returned post-dropout weights,
`loss = (o . do).sum() + (a . G).sum()`, against fp64 on the CPU -- through the C ABI at head_dim 128 in place and through ops at
each case's own head_dim, without masks and under tensor masks, for every layout of G the backward meets, under dropout, for a
loss on the weights alone, in a captured graph -- and the refusals.
Measured worst errors: attention_dattn_*.txt in REPORT_DIR, and DESIGN.md 16."""
import contextlib
import ctypes
import functools
import os
import types

import pytest
import torch

from conftest import rel_l2
from test_hip_dropout_parity import REPORT_DIR, _t
from test_hip_ops import TOL, _dev, _g, _rand

from oracle import dropmask as dm

pytestmark = pytest.mark.gpu
NEG_INF = float("-inf")

# edges of the 128-row query block (150, 200 = 128 + 72, 161 = 128 + 33), of the 32-row stages (70, 161, 33) and of the 4-float
# row padding of G (Tk 70, 161, 1 and 33 are no multiples of 4); `lens`: ragged key counts, one utterance without a key
CASES = {
    "150x70": dict(B=2, H=2, Tq=150, Tk=70, hd=96),
    "200x161": dict(B=2, H=2, Tq=200, Tk=161, hd=64),
    "5x1": dict(B=2, H=2, Tq=5, Tk=1, hd=128),
    "161x33": dict(B=3, H=2, Tq=161, Tk=33, hd=16, lens=(33, 20, 0)),
}


def _report(name, lines):
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(f"{REPORT_DIR}/attention_dattn_{name}.txt", "w") as f:
        f.write("\n".join(lines) + "\n")


def _ref(q_, kv_, do, G, H, allowed, add, keep=None):
    """fp64 on the CPU as tests/test_hip_attention_masked.py::_ref, with loss = (o . do).sum() + (a . G).sum(); `do` or `G` may be
    None (that term is absent).  `keep`: a (B, H, Tq, Tk) multiplier of the weights (dropout x scale), or None."""
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
    loss = 0.0
    if do is not None:
        loss = loss + (o * do.double()).sum()
    if G is not None:
        loss = loss + (a * G.double()).sum()
    loss.backward()
    return types.SimpleNamespace(o=o.detach(), a=a.detach(), dq=qd.grad, dkv=kvd.grad)


@functools.lru_cache(maxsize=None)
def _case(name, hd=None, masked=False):
    """inputs (CPU fp32), the masks and the fp64 reference of one case, computed once and shared (read-only)"""
    c = dict(CASES[name])
    c["hd"] = hd or c["hd"]
    B, H, Tq, Tk, d = c["B"], c["H"], c["Tq"], c["Tk"], c["H"] * c["hd"]
    s = 1000 * sorted(CASES).index(name) + c["hd"] + (500 if masked else 0)
    q_, kv_, do = _rand(B, Tq, d, seed=s + 1), _rand(B, Tk, 2 * d, seed=s + 2), _rand(B, Tq, d, seed=s + 3)
    G = _rand(B, H, Tq, Tk, seed=s + 4)
    lens = torch.tensor(c.get("lens", (Tk,) * B), dtype=torch.int64)
    key = torch.arange(Tk)
    dead, add_mask = None, None
    allowed = (key[None, :] < lens[:, None])[:, None, None, :].expand(B, H, Tq, Tk).clone()
    add = torch.zeros(B, H, Tq, Tk, dtype=torch.float64)
    if masked:      # `dead` (replaces the length mask) + one shared (Tq, Tk) float mask that forbids one whole query row
        g = torch.Generator().manual_seed(s)
        dead = key[None, :] >= lens[:, None]
        if Tk > 1:
            dead = dead | (torch.rand(B, Tk, generator=g) < 0.3)
        else:
            dead[-1] = True
        add_mask = torch.rand(Tq, Tk, generator=g) * 8 - 4
        if Tk > 1:
            add_mask = add_mask.masked_fill(torch.rand(Tq, Tk, generator=g) < 0.3, NEG_INF)
        add_mask[min(7, Tq - 1), :] = NEG_INF
        full = add_mask.expand(B, H, Tq, Tk)
        allowed = ~dead[:, None, None, :].expand(B, H, Tq, Tk) & ~torch.isneginf(full)
        add = full.masked_fill(torch.isneginf(full), 0).double()
    no_key = ~allowed.any(dim=-1)
    if masked or "lens" in c:
        assert int(no_key.sum()) >= 1, name
    return types.SimpleNamespace(q=q_, kv=kv_, do=do, G=G, lens=lens, dead=dead, add_mask=add_mask, allowed=allowed, add=add,
                                 no_key=no_key, d=d, masked=masked, ref=_ref(q_, kv_, do, G, H, allowed, add),
                                 **{k: v for k, v in c.items() if k != "lens"})


def _errors(got, c, ref=None, G=None):
    """worst-case figures of one run against the fp64 reference; asserts what is exact: rows without a key, unseen keys"""
    ref = ref or c.ref
    o, attn, dq, dkv = got
    for t in (o, attn, dq, dkv):
        assert bool(torch.isfinite(t).all())
    errs = {"o": rel_l2(o, ref.o), "attn": rel_l2(attn, ref.a), "dkv": rel_l2(dkv, ref.dkv)}
    assert float(attn[~c.allowed].abs().sum()) == 0.0
    if c.Tk == 1:        # one key: the weights are constant 0 / 1 and dq is exactly zero in fp64 -- absolute bound instead
        big = max(c.do.abs().max().item(), (c.G if G is None else G).abs().max().item())
        assert dq.abs().max().item() < 1e-6 * big
    else:
        errs["dq"] = rel_l2(dq, ref.dq)
    rows = c.no_key.transpose(1, 2)[..., None].expand(c.B, c.Tq, c.H, c.hd).reshape(c.B, c.Tq, c.d)
    assert float(o[rows].abs().sum()) == 0.0 and float(dq[rows].abs().sum()) == 0.0
    unseen = ~c.allowed.any(dim=2)                                              # (B, H, Tk)
    cols = unseen.transpose(1, 2)[..., None].expand(c.B, c.Tk, c.H, c.hd).reshape(c.B, c.Tk, c.d)
    assert float(dkv[..., :c.d][cols].abs().sum()) == 0.0 and float(dkv[..., c.d:][cols].abs().sum()) == 0.0
    return errs


def _abi(c, G=None, p=0.0, seed=0, ss=None):
    """head_dim 128 in place: the forward of the (un)masked entry point, then ttts_attention_bwd_wide_dattn with G used where it
    lies -> (o, attn, dq, dkv) on the CPU.  Every output starts as NaN."""
    from transformertts_amd import _lib, ops
    from transformertts_amd.ops import _off, _p, _stream
    lib, dev = _lib.load(), _dev()
    B, H, Tq, Tk, d = c.B, c.H, c.Tq, c.Tk, c.d
    assert c.hd == 128
    nan = float("nan")
    q, kv = c.q.to(dev), c.kv.to(dev)
    dq, dkv = torch.full_like(q, nan), torch.full_like(kv, nan)
    ins, lds = [_p(q), _off(kv, 0), _off(kv, d)], [d, 2 * d, 2 * d]
    outs = [_p(dq), _off(dkv, 0), _off(dkv, d)]
    o = torch.full((B, Tq, d), nan, device=dev)
    stat = torch.full((2, B, H, Tq), nan, device=dev)
    attn = torch.full((B, H, Tq, Tk), nan, device=dev)
    delta = torch.full((B, H, Tq), nan, device=dev)
    do_d = c.do.to(dev)
    dead = None if c.dead is None else c.dead.to(dev)
    m4 = None if c.add_mask is None else ops._mask_operand(c.add_mask.to(dev), B, H, Tq, Tk)
    margs = ops._mask_args(dead, m4, Tk)
    lens_d = (torch.full((B,), Tk, dtype=torch.int64) if c.masked else c.lens).to(dev)
    g4 = ops.pad_mask_rows((c.G if G is None else G).to(dev))
    assert ops._dattn_in_place(g4, Tk)
    scale = 128 ** -0.5
    if c.masked:
        _lib.check(lib.ttts_attention_fwd_wide_masked(*ins, _p(o), _p(stat), _p(attn), _p(lens_d), B, H, Tq, Tk, *lds, d, 0, scale, p,
                                                      seed, ss, *margs, _stream()), "ttts_attention_fwd_wide_masked")
    else:
        _lib.check(lib.ttts_attention_fwd_wide(*ins, _p(o), _p(stat), _p(attn), _p(lens_d), B, H, Tq, Tk, *lds, d, 0, scale, p, seed,
                                               ss, _stream()), "ttts_attention_fwd_wide")
    _lib.check(lib.ttts_attention_bwd_wide_dattn(*ins, _p(o), _p(do_d), _p(stat), _p(delta), *outs, _p(lens_d), B, H, Tq, Tk, *lds, d,
                                                 *lds, 0, scale, p, seed, ss, *margs, _p(attn), *ops._dattn_args(g4, Tk), _stream()),
               "ttts_attention_bwd_wide_dattn")
    torch.cuda.synchronize()
    return o.cpu(), attn.cpu(), dq.cpu(), dkv.cpu()


def _ops_run(c, G="case", do="case", p=0.0, seed=0, weights_grad=True):
    """through ops.cross_attention -> (o, attn, dq, dkv) on the CPU; G / do: a tensor on the device handed to autograd as it is, "case"
    (the case's own, contiguous) or None (that output gets no gradient)"""
    from transformertts_amd import ops
    dev = _dev()
    dead = None if c.dead is None else c.dead.to(dev)
    add_mask = None if c.add_mask is None else c.add_mask.to(dev)
    lens_d = (torch.full((c.B,), c.Tk, dtype=torch.int64) if c.masked else c.lens).to(dev)
    qg, kvg = _g(c.q), _g(c.kv)
    kw = dict(weights_grad=True) if weights_grad else {}
    out, w = ops.cross_attention(qg, kvg, lens_d, c.H, p, seed, True, dead=dead, add_mask=add_mask, **kw)
    G = c.G.to(dev) if isinstance(G, str) else G
    do = c.do.to(dev) if isinstance(do, str) else do
    outs, grads = zip(*[(t, g) for t, g in ((out, do), (w, G)) if g is not None])
    torch.autograd.backward(outs, grads)
    return out.detach().cpu(), w.detach().cpu(), qg.grad.cpu(), kvg.grad.cpu()


# ============================================================================================ 1, 2. the C ABI and ops against fp64
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_dattn_kernels_through_the_c_abi_vs_fp64(name, masked):
    """every shape at head_dim 128 in place, without masks (both mask pointers NULL) and under `dead` + a shared float mask"""
    c = _case(name, 128, masked)
    errs = _errors(_abi(c), c)
    line = f"{name} hd128 masked={masked}: " + " ".join(f"{k}={v:.3e}" for k, v in sorted(errs.items()))
    print(line)
    _report(f"abi_{name}_{'masked' if masked else 'plain'}", [f"# worst {max(errs.values()):.3e} (gate {TOL:g})", line])
    assert max(errs.values()) < TOL, line


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_dattn_through_ops_vs_fp64(name, masked):
    """every shape at its own head_dim (128 in place; 96, 64 and 16 padded to 128) through ops.cross_attention(weights_grad=True)"""
    c = _case(name, None, masked)
    errs = _errors(_ops_run(c), c)
    line = f"{name} hd{c.hd} masked={masked}: " + " ".join(f"{k}={v:.3e}" for k, v in sorted(errs.items()))
    print(line)
    _report(f"ops_{name}_{'masked' if masked else 'plain'}", [f"# worst {max(errs.values()):.3e} (gate {TOL:g})", line])
    assert max(errs.values()) < TOL, line


# ============================================================================================ 3. the layouts of G
def _layouts(c, dev):
    """name -> (G as the backward receives it, used in place?) ; every one is compared with a contiguous copy of its own values"""
    from transformertts_amd import ops
    B, H, Tq, Tk = c.B, c.H, c.Tq, c.Tk
    G = c.G.to(dev)
    w = Tk + 1 if (Tk + 1) % 4 else Tk + 2           # a row stride that is no multiple of 4
    wide = torch.zeros(B, H, Tq, w, device=dev)
    wide[..., 1:Tk + 1] = G
    return {
        "contiguous": (G, Tk % 4 == 0 or Tq == 1),
        "padded": (ops.pad_mask_rows(G), True),
        "head_expanded": (ops.pad_mask_rows(G[:, :1].contiguous()).expand(B, H, Tq, Tk), True),
        "shared_2d": (ops.pad_mask_rows(G[0, 0].contiguous())[None, None].expand(B, H, Tq, Tk), True),
        "head_expanded_unpadded": (G[:, :1].expand(B, H, Tq, Tk), Tk % 4 == 0 or Tq == 1),
        "column_slice": (wide[..., 1:Tk + 1], False),
    }


@pytest.mark.parametrize("name,masked", [("150x70", True), ("161x33", False)])
def test_dattn_layouts_of_the_gradient_agree_bitwise(name, masked):
    """contiguous, zero-padded rows, expanded over the heads (stride 0), one (Tq, Tk) tensor expanded over batch and heads, and a
    column slice whose row stride is no multiple of 4 (the copy path): each gives, bit for bit, what a contiguous G of the same
    values gives; which ones the kernels read in place is what `_dattn_in_place` says"""
    from transformertts_amd import ops
    c = _case(name, None, masked)
    dev = _dev()
    for lname, (G, in_place) in _layouts(c, dev).items():
        assert tuple(G.shape) == (c.B, c.H, c.Tq, c.Tk)
        assert ops._dattn_in_place(G, c.Tk) == in_place, lname
        got = _ops_run(c, G=G)
        base = _ops_run(c, G=G.contiguous())
        for what, a, b in zip(("o", "attn", "dq", "dkv"), got, base):
            assert torch.equal(a, b), (lname, what)
        if lname == "shared_2d":       # ... and that common value is right
            Gc = G.contiguous().cpu()
            errs = _errors(got, c, _ref(c.q, c.kv, c.do, Gc, c.H, c.allowed, c.add), Gc)
            assert max(errs.values()) < TOL, errs


# ============================================================================================ 4. dropout
@pytest.mark.parametrize("word", [None, 0x0F1E2D3C4B5A6978])
@pytest.mark.parametrize("name,masked", [("150x70", True), ("200x161", False)])
def test_dattn_under_dropout_vs_fp64_with_keep_attn(name, masked, word):
    """p = 0.25, with and without a step word: the weights are A = D o P / (1 - p) under oracle.dropmask.keep_attn's mask, and o, dq,
    dk / dv hold the fp64 reference that differentiates through that mask, at the same gate"""
    from transformertts_amd import ops
    c = _case(name, None, masked)
    st = contextlib.nullcontext()
    if word is not None:
        st = ops.StepState(_dev())
        st.push(seed=word, lr=0.0, p_tf=1.0, step=1)
    p, seed = 0.25, 0x0123456789ABCDEF
    keep = _t(dm.keep_attn(dm.site_seed(seed, word), c.B * c.H * c.Tq, c.Tk, p), c.B, c.H, c.Tq, c.Tk)
    ref = _ref(c.q, c.kv, c.do, c.G, c.H, c.allowed, c.add, keep.double() * dm.drop_scale(p))
    with st:
        got = _ops_run(c, p=p, seed=seed)
    assert torch.equal(got[1] != 0, keep & c.allowed)
    errs = _errors(got, c, ref)
    line = f"{name} hd{c.hd} masked={masked} p=0.25 word={word}: " + " ".join(f"{k}={v:.3e}" for k, v in sorted(errs.items()))
    print(line)
    _report(f"dropout_{name}" + ("_stepstate" if word is not None else ""), [f"# worst {max(errs.values()):.3e} (gate {TOL:g})", line])
    assert max(errs.values()) < TOL, line


# ============================================================================================ 5. a loss on the maps alone
@pytest.mark.parametrize("name,masked", [("150x70", False), ("161x33", True)])
def test_a_loss_on_the_maps_alone_reaches_q_and_kv(name, masked):
    """`(a . G).sum().backward()`, the context unused: autograd calls the backward without a gradient of o, and dq, dk / dv equal the
    fp64 reference (dv is zero: the maps do not depend on v).  Without differentiable weights nothing reaches q and kv at all."""
    c = _case(name, None, masked)
    ref = _ref(c.q, c.kv, None, c.G, c.H, c.allowed, c.add)
    o, attn, dq, dkv = _ops_run(c, do=None)
    assert float(dq.abs().max()) > 0 and float(dkv[..., :c.d].abs().max()) > 0
    assert float(dkv[..., c.d:].abs().max()) == 0.0
    errs = {"dq": rel_l2(dq, ref.dq), "dk": rel_l2(dkv[..., :c.d], ref.dkv[..., :c.d])}
    line = f"{name} hd{c.hd} masked={masked} maps alone: " + " ".join(f"{k}={v:.3e}" for k, v in sorted(errs.items()))
    print(line)
    _report(f"maps_alone_{name}", [f"# worst {max(errs.values()):.3e} (gate {TOL:g})", line])
    assert max(errs.values()) < TOL, line


# ============================================================================================ 6. the flag alone changes nothing
@pytest.mark.parametrize("name,masked", [("150x70", False), ("200x161", True)])
def test_weights_grad_with_only_the_context_used_is_bit_identical(name, masked):
    """weights_grad=True but no gradient on the weights: the backward takes today's entry points, and o, the weights, dq and dk / dv
    are bit-identical to weights_grad=False on the same 128-column route (head_dim 96; head_dim 64 under masks), p = 0.1"""
    c = _case(name, None, masked)
    a = _ops_run(c, G=None, p=0.1, seed=77, weights_grad=True)
    b = _ops_run(c, G=None, p=0.1, seed=77, weights_grad=False)
    for what, x, y in zip(("o", "attn", "dq", "dkv"), a, b):
        assert torch.equal(x, y), what


def test_without_the_flag_the_weights_stay_detached():
    from transformertts_amd import ops
    c = _case("150x70")
    dev = _dev()
    _, w = ops.cross_attention(_g(c.q), _g(c.kv), c.lens.to(dev), c.H, 0.0, 0, True)
    assert not w.requires_grad
    _, w = ops.cross_attention(_g(c.q), _g(c.kv), c.lens.to(dev), c.H, 0.0, 0, True, weights_grad=True)
    assert w.requires_grad


# ============================================================================================ 7. graph replay, repeatability
def test_dattn_graph_replay_equals_eager_bitwise():
    """forward + backward of ops.cross_attention(weights_grad=True) with gradients on o and on the weights, p = 0.1, under a step
    state, captured into one HIP graph: a replay equals the eager call bit for bit on o, the weights, dq and dkv for the captured
    step word and for another one; two eager runs are bit-identical"""
    from transformertts_amd import ops
    dev = _dev()
    c = _case("150x70", None, True)
    p, seed = 0.1, 0x1111222233334444
    st = ops.StepState(dev)
    ins = dict(q=c.q.to(dev).requires_grad_(), kv=c.kv.to(dev).requires_grad_(), do=c.do.to(dev), dead=c.dead.to(dev),
               mask=c.add_mask.to(dev), lens=torch.full((c.B,), c.Tk, dtype=torch.int64, device=dev),
               G=ops.pad_mask_rows(c.G[:, :1].contiguous().to(dev)).expand(c.B, c.H, c.Tq, c.Tk))

    def step():
        ins["q"].grad = ins["kv"].grad = None
        o, w = ops.cross_attention(ins["q"], ins["kv"], ins["lens"], c.H, p, seed, True, dead=ins["dead"], add_mask=ins["mask"],
                                   weights_grad=True)
        torch.autograd.backward([o, w], [ins["do"], ins["G"]])
        return [o.detach(), w.detach(), ins["q"].grad, ins["kv"].grad]

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
            again = [t.clone() for t in step()]
            for what, a, b, e in zip(("o", "weights", "dq", "dkv"), replayed, eager, again):
                assert torch.equal(a, b), (what, hex(word))
                assert torch.equal(b, e), (what, hex(word))
            if n == 0:
                first = replayed
        assert not torch.equal(first[1], replayed[1])                # and the step word matters


# ============================================================================================ 8. refusals
def test_dattn_refusals():
    from transformertts_amd import _lib, ops
    lib, dev = _lib.load(), _dev()
    c = _case("5x1")
    q, kv = _g(c.q), _g(c.kv)
    lens = c.lens.to(dev)
    with pytest.raises(ValueError, match="non-causal form only"):
        ops.AttentionFn.apply(torch.zeros(1, 4, 3 * 128, device=dev), None, torch.tensor([4], device=dev), 1, True, 0.0, 0, True,
                              None, None, None, None, None, True)
    full = torch.zeros(2 * c.B, c.Tq, c.d, device=dev)
    with pytest.raises(ValueError, match="no head image, no twin batch"):
        ops.cross_attention(ops.twin_pair(full)[0], kv, lens, c.H, 0.0, 0, True, weights_grad=True)
    img = ops.HeadImage(torch.zeros(1, 4, 192, device=dev), torch.zeros(1, 4, device=dev), None, 64)
    with pytest.raises(ValueError, match="no head image, no twin batch"):
        ops.cross_attention(ops.HeadImage(torch.zeros(1, 4, 64, device=dev), torch.zeros(1, 4, device=dev), None, 64), img, lens, 1,
                            0.0, 0, True, weights_grad=True)

    # the C ABI, on real device memory; every refusal comes before a launch and names its value
    B, H, Tq, Tk, d = 1, 2, 5, 5, 256
    t = torch.zeros(4096, device=dev)
    a, a4 = ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(t.data_ptr() + 4)
    names = ["q", "k", "v", "o", "d_o", "stat", "delta", "dq", "dk", "dv", "lens", "B", "H", "Tq", "Tk", "ldq", "ldk", "ldv", "ldo",
             "lddq", "lddk", "lddv", "causal", "scale", "p", "seed", "step_seed", "add_mask", "ldm", "mask_stride_b", "mask_stride_h",
             "key_dead", "ldd", "attn", "d_attn", "ld_dattn", "dattn_stride_b", "dattn_stride_h", "stream"]
    defaults = dict({n: a for n in names[:11]}, B=B, H=H, Tq=Tq, Tk=Tk, ldq=d, ldk=d, ldv=d, ldo=d, lddq=d, lddk=d, lddv=d, causal=0,
                    scale=0.1, p=0.0, seed=0, step_seed=None, add_mask=None, ldm=0, mask_stride_b=0, mask_stride_h=0, key_dead=None,
                    ldd=0, attn=a, d_attn=a, ld_dattn=8, dattn_stride_b=0, dattn_stride_h=0, stream=None)

    def bad(needle, **kw):
        assert not set(kw) - set(names)
        rc = lib.ttts_attention_bwd_wide_dattn(*[kw.get(n, defaults[n]) for n in names])
        assert rc == -1 and needle in _lib.last_error(), (rc, _lib.last_error())

    bad("attention_bwd_wide_dattn: attn is NULL", attn=None)
    bad("attention_bwd_wide_dattn: d_attn is NULL", d_attn=None)
    bad("non-causal (cross) form (causal 1)", causal=1)
    bad("multiple of 4 floats and >= Tk (ld_dattn 4, Tk 5)", ld_dattn=4)
    bad("multiple of 4 floats and >= Tk (ld_dattn 6, Tk 5)", ld_dattn=6)
    bad("d_attn must be 16-byte aligned", d_attn=a4)
    bad("dattn_stride_b 42,", dattn_stride_b=42)
    bad("must not be negative (dattn_stride_b 0, dattn_stride_h -40)", dattn_stride_h=-40)
    bad("one d_attn slice exceeds 4 GiB (Tq 1048576, ld_dattn 1024)", Tq=1 << 20, ld_dattn=1024)
    bad("attention_bwd_wide_dattn: null pointer", dq=None)
    bad("(ldm 6, Tk 5)", add_mask=a, ldm=6)                      # a mask that is given is checked as the _masked entry point does
    bad("attention_bwd_wide_dattn: q/k/v/o/d_o must be 16-byte aligned", k=a4)
