"""Differentiable alignment maps and the guided attention loss (ABI v19: ttts_attention_bwd_wide_dattn, csrc/attention_wide.hip;
ttts_guided_attention_fwd / ttts_guided_attention_bwd, csrc/guided.hip): declared, bound, exported, their refusals, the refusals
of the layers above, and which gradient layouts the kernels read in place.  Host logic only, no GPU (every refusal happens
before a launch)."""
import ctypes
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ttts_attention_bwd_wide_dattn", "ttts_guided_attention_fwd", "ttts_guided_attention_bwd")


def test_abi_version_and_the_header_declares_the_new_entry_points():
    from transformertts_amd import _lib
    lib = _lib.load()
    assert lib.ttts_abi_version() >= 19
    hdr = open(os.path.join(REPO, "include", "ttts_hip.h")).read()
    declared = set(re.findall(r"\b(ttts_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, f"{name} is not declared in ttts_hip.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name), f"{name} is not exported / bound"
    P, I, L, F, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_uint64
    # the arguments of the _masked backward, then attn, d_attn, its row stride and its batch / head strides, then the stream
    res, args = _lib.SIGNATURES[NEW[0]]
    res0, args0 = _lib.SIGNATURES["ttts_attention_bwd_wide_masked"]
    assert res == res0 and args == args0[:-1] + [P, P, L, L, L] + args0[-1:]
    decl = re.search(NEW[0] + r"\s*\(([^;]*)\)\s*;", hdr).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")][-6:-1] == ["attn", "d_attn", "ld_dattn", "dattn_stride_b",
                                                                         "dattn_stride_h"]
    assert _lib.SIGNATURES[NEW[1]] == (I, [P, P, P, U, F, I, I, I, I, P, I, I, I, P, P])
    assert _lib.SIGNATURES[NEW[2]] == (I, [P, P, P, U, F, I, I, I, I, I, I, P, P])
    for name in NEW[1:]:      # ctypes and the header agree on the number of arguments
        decl = re.search(name + r"\s*\(([^;]*)\)\s*;", hdr).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1])
    # every declaration cites the torch call site it replaces
    block = hdr[hdr.index("ABI v19"):hdr.index("int ttts_guided_attention_bwd")]
    assert "torch/nn/functional.py" in block and "model/layers.py:68-74" in block


def test_entry_points_refuse_bad_arguments_with_a_message():
    from transformertts_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096 + 16)
    a = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)          # a 16-byte aligned host address (never dereferenced)
    a4 = ctypes.c_void_p(a.value + 4)

    def bad(rc, needle):
        assert rc == -1, rc
        assert needle in _lib.last_error(), _lib.last_error()

    names = ["q", "k", "v", "o", "d_o", "stat", "delta", "dq", "dk", "dv", "lens", "B", "H", "Tq", "Tk", "ldq", "ldk", "ldv", "ldo",
             "lddq", "lddk", "lddv", "causal", "scale", "p", "seed", "step_seed", "add_mask", "ldm", "mask_stride_b", "mask_stride_h",
             "key_dead", "ldd", "attn", "d_attn", "ld_dattn", "dattn_stride_b", "dattn_stride_h", "stream"]
    defaults = dict({n: a for n in names[:11]}, B=1, H=2, Tq=5, Tk=5, ldq=768, ldk=768, ldv=768, ldo=256, lddq=768, lddk=768, lddv=768,
                    causal=0, scale=0.1, p=0.0, seed=0, step_seed=None, add_mask=None, ldm=0, mask_stride_b=0, mask_stride_h=0,
                    key_dead=None, ldd=0, attn=a, d_attn=a, ld_dattn=8, dattn_stride_b=0, dattn_stride_h=0, stream=None)

    def bwd(**kw):
        assert not set(kw) - set(names)
        return lib.ttts_attention_bwd_wide_dattn(*[kw.get(n, defaults[n]) for n in names])

    e = "attention_bwd_wide_dattn"
    bad(bwd(q=None), e + ": null pointer")
    bad(bwd(B=0), e + ": sizes must be positive (B 0,")
    bad(bwd(ldq=770), "multiples of 4 floats (ldq 770,")
    bad(bwd(lddk=128), "gradient strides must be >= H*128 = 256 (lddq 768, lddk 128,")
    bad(bwd(p=1.0), "dropout p 1 is outside [0, 1)")
    bad(bwd(attn=None), e + ": attn is NULL")
    bad(bwd(d_attn=None), e + ": d_attn is NULL")
    bad(bwd(causal=1), "non-causal (cross) form (causal 1)")
    bad(bwd(ld_dattn=4), "multiple of 4 floats and >= Tk (ld_dattn 4, Tk 5)")
    bad(bwd(ld_dattn=6), "multiple of 4 floats and >= Tk (ld_dattn 6, Tk 5)")
    bad(bwd(d_attn=a4), "d_attn must be 16-byte aligned")
    bad(bwd(dattn_stride_b=42), "dattn_stride_b 42,")
    bad(bwd(dattn_stride_h=-40), "must not be negative (dattn_stride_b 0, dattn_stride_h -40)")
    bad(bwd(dattn_stride_b=-8), "must not be negative (dattn_stride_b -8,")
    bad(bwd(Tq=1 << 20, ld_dattn=1024), "one d_attn slice exceeds 4 GiB (Tq 1048576, ld_dattn 1024)")
    # both masks may be NULL (the refusal comes from a later check); a mask that is given is checked
    bad(bwd(k=a4), e + ": q/k/v/o/d_o must be 16-byte aligned")
    bad(bwd(add_mask=a, ldm=6), "(ldm 6, Tk 5)")
    bad(bwd(key_dead=a, ldd=4), "dead-key row stride must be >= Tk (ldd 4, Tk 5)")

    fn = ["attn", "plens", "mlens", "head_mask", "sigma", "B", "H", "Tm", "Tp", "partials", "map_index", "n_maps", "n_selected",
          "loss", "stream"]
    fd = dict(attn=a, plens=a, mlens=a, head_mask=0, sigma=0.4, B=2, H=4, Tm=7, Tp=5, partials=a, map_index=0, n_maps=1,
              n_selected=4, loss=a, stream=None)
    bn = ["g", "plens", "mlens", "head_mask", "sigma", "n_selected", "B", "H", "Tm", "Tp", "ld", "d_attn", "stream"]
    bd = dict(g=a, plens=a, mlens=a, head_mask=0, sigma=0.4, n_selected=4, B=2, H=4, Tm=7, Tp=5, ld=8, d_attn=a, stream=None)
    fwd = lambda **kw: lib.ttts_guided_attention_fwd(*[kw.get(n, fd[n]) for n in fn])
    gbw = lambda **kw: lib.ttts_guided_attention_bwd(*[kw.get(n, bd[n]) for n in bn])
    for call, name in ((fwd, "guided_attention_fwd"), (gbw, "guided_attention_bwd")):
        bad(call(plens=None), name + ": null pointer")
        bad(call(sigma=0.0), name + ": sigma 0 must be positive")
        bad(call(sigma=-1.0), name + ": sigma -1 must be positive")
        bad(call(Tp=0), name + ": sizes must be positive (B 2, H 4, Tm 7, Tp 0)")
        bad(call(n_selected=0), name + ": n_selected 0 must be positive")
        bad(call(head_mask=0x10), name + ": head_mask 0x10 selects a head past H 4")
        bad(call(head_mask=1, H=65), "at most 64 heads (H 65)")
    bad(fwd(attn=None), "guided_attention_fwd: null pointer")
    bad(fwd(map_index=1), "map_index 1 is outside [0, n_maps 1)")
    bad(gbw(g=None), "guided_attention_bwd: null pointer")
    bad(gbw(ld=6), "multiple of 4 floats and >= Tp (ld 6, Tp 5)")
    bad(gbw(ld=4), "multiple of 4 floats and >= Tp (ld 4, Tp 5)")


def test_guided_attention_loss_constructor_and_arguments():
    from transformertts_amd.loss import GuidedAttentionLoss
    for sigma in (0.0, -0.4, float("nan")):
        with pytest.raises(ValueError, match="must be positive"):
            GuidedAttentionLoss(sigma)
    with pytest.raises(ValueError, match="`heads` selects nothing"):
        GuidedAttentionLoss(heads=[])
    with pytest.raises(ValueError, match="`layers` selects nothing"):
        GuidedAttentionLoss(layers=())
    with pytest.raises(ValueError, match="distinct non-negative indices"):
        GuidedAttentionLoss(heads=[-1])
    with pytest.raises(ValueError, match="distinct non-negative indices"):
        GuidedAttentionLoss(layers=[1, 1])
    crit = GuidedAttentionLoss(0.2, heads=(3, 1), layers=[2])
    assert (crit.sigma, crit.heads, crit.layers) == (0.2, [1, 3], [2]) and not list(crit.parameters()) and not crit.state_dict()
    maps, lens = [torch.zeros(2, 4, 6, 5)] * 3, torch.tensor([5, 3])
    with pytest.raises(ValueError, match="head 3 of 2 heads"):
        crit([torch.zeros(2, 2, 6, 5)] * 3, lens, lens)
    with pytest.raises(ValueError, match="layer 2 of 2 alignment maps"):
        crit(maps[:2], lens, lens)
    with pytest.raises(ValueError, match="no alignment maps"):
        GuidedAttentionLoss()([None], lens, lens)
    with pytest.raises(ValueError, match="no CPU fallback"):          # HIP tensors only
        crit(maps, lens, lens)


def test_alignments_grad_needs_need_alignments_and_fp32_operands():
    from oracle import model_config
    from transformertts_amd import ops
    from transformertts_amd.model import TransformerTTS
    from transformertts_amd.model import layers as L
    import inspect
    cfg = model_config("micro")
    m = TransformerTTS(**cfg, device="cpu")
    ph, mel, lens = torch.zeros(1, 3, dtype=torch.int64), torch.zeros(1, 4, cfg["n_mels"]), torch.tensor([3])
    with pytest.raises(ValueError, match="alignments_grad=True needs need_alignments=True"):
        m(ph, mel, lens, torch.tensor([4]), need_alignments=False, alignments_grad=True)
    with pytest.raises(ValueError, match="alignments_grad=True needs need_alignments=True"):
        m.decoder(torch.zeros(1, 4, 32), torch.zeros(1, 3, 32), need_alignments=False, alignments_grad=True)
    # an extension next to need_alignments, off by default, at every level
    assert inspect.signature(TransformerTTS.forward).parameters["alignments_grad"].default is False
    assert inspect.signature(L.TransformerDecoder.forward).parameters["alignments_grad"].default is False
    assert inspect.signature(L.TransformerDecoderLayer.forward).parameters["alignments_grad"].default is False
    assert inspect.signature(L.MultiheadAttention.cross_attention).parameters["weights_grad"].default is False
    assert inspect.signature(ops.cross_attention).parameters["weights_grad"].default is False
    # a head image or a twin batch cannot carry differentiable weights
    img = ops.HeadImage(torch.zeros(1, 4, 192), torch.zeros(1, 4), None, 64)
    with pytest.raises(ValueError, match="no head image, no twin batch"):
        ops.cross_attention(ops.HeadImage(torch.zeros(1, 4, 64), torch.zeros(1, 4), None, 64), img, torch.tensor([4]), 1, 0.0, 0,
                            weights_grad=True)
    half = ops.twin_pair(torch.zeros(2, 4, 64))[0]
    with pytest.raises(ValueError, match="no head image, no twin batch"):
        ops.cross_attention(half, torch.zeros(1, 4, 128), torch.tensor([4]), 1, 0.0, 0, weights_grad=True)
    with pytest.raises(ValueError, match="gives no gradient of the weights"):
        L.MultiheadAttention(64, 1).cross_attention(torch.zeros(1, 4, 64), torch.zeros(1, 4, 64), torch.tensor([4]), None, 0.0,
                                                    kv=img, weights_grad=True)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.cross_attention(torch.zeros(1, 4, 96), torch.zeros(1, 4, 192), torch.tensor([4]), 1, 0.0, 0, weights_grad=True)


def test_lightning_module_config_key():
    from oracle import model_config
    from transformertts_amd.lightning_module import LightningModule
    from transformertts_amd.loss import GuidedAttentionLoss
    training = {"num_epochs": 3, "teacher_forcing_mode": "linear", "warmup_steps": 5}
    mk = lambda t: LightningModule({"model": dict(model_config("micro"), device="cpu"), "loss": {"stop_weight": 8.0}, "training": t})
    keys = set(mk(dict(training)).state_dict())
    for absent in (dict(training), dict(training, guided_attention=None)):
        lm = mk(absent)
        assert lm.guided is None and lm.guided_weight is None
    lm = mk(dict(training, guided_attention={"weight": 0.5, "sigma": 0.3, "heads": [0], "layers": [0]}))
    assert isinstance(lm.guided, GuidedAttentionLoss) and lm.guided_weight == 0.5
    assert (lm.guided.sigma, lm.guided.heads, lm.guided.layers) == (0.3, [0], [0])
    assert set(lm.state_dict()) == keys                                   # the state dict does not change
    with pytest.raises(KeyError):
        mk(dict(training, guided_attention={"sigma": 0.3}))
    with pytest.raises(ValueError, match="must be positive"):
        mk(dict(training, guided_attention={"weight": 1.0, "sigma": 0.0}))


def test_which_gradient_layouts_are_read_in_place():
    """`ops._dattn_in_place` on CPU tensors (it reads shapes, strides, the address and the storage size only)"""
    from transformertts_amd import ops
    B, H, Tq = 2, 3, 5
    ok = ops._dattn_in_place
    assert ok(torch.zeros(B, H, Tq, 8), 8)                                             # contiguous, rows of two quads
    assert not ok(torch.zeros(B, H, Tq, 7), 7)                                         # rows 7 floats apart
    assert ok(torch.zeros(B, H, Tq, 8)[..., :7], 7)                                    # ... padded to 8
    assert ok(ops.pad_mask_rows(torch.zeros(B, H, Tq, 7)), 7)
    assert ok(torch.zeros(B, 1, Tq, 8).expand(B, H, Tq, 8), 8)                         # expanded over the heads: stride 0
    assert ok(torch.zeros(Tq, 8)[None, None].expand(B, H, Tq, 8), 8)                   # one map for every batch and head
    assert ok(torch.zeros(B, Tq, 8)[:, None, :, :5].expand(B, H, Tq, 5), 5)            # what GuidedAttentionFn.backward returns
    assert not ok(torch.zeros(B, H, Tq, 12)[..., 1:9], 8)                              # a slice that starts off a 16-byte boundary
    assert not ok(torch.zeros(B, H, Tq, 10)[..., :8], 8)                               # row stride 10
    assert not ok(torch.zeros(B, H, 8, Tq).transpose(2, 3), 8)                         # columns not contiguous
    assert not ok(torch.zeros(B, H, Tq, 8, dtype=torch.float64), 8)
    assert not ok(torch.zeros(B, H, Tq, 8), 6)                                         # not the (.., Tk) the backward expects
    assert ok(torch.zeros(1, 1, 1, 4)[..., :3], 3)                                     # one row: its stride is free ...
    assert not ok(torch.zeros(1, 1, 1, 3), 3)                                          # ... but its last quad must exist
    assert not ok(torch.zeros(2, 2, 1, 3), 3)                                          # ... but the slices lie 12 bytes apart
    # the last row's padding must lie inside the storage: a (Tq, 7) view of a buffer that ends with the last element does not
    flat = torch.zeros(Tq * 8 - 1)
    assert not ok(flat.as_strided((1, 1, Tq, 7), (0, 0, 8, 1)), 7)
    assert ok(torch.zeros(Tq * 8).as_strided((1, 1, Tq, 7), (0, 0, 8, 1)), 7)
    # the copy keeps the values and is addressable
    g = torch.arange(B * H * Tq * 7, dtype=torch.float32).reshape(B, H, Tq, 7)
    c = ops._dattn_operand(g, 7)
    assert torch.equal(c, g) and ok(c, 7) and c.stride(2) == 8
    same = torch.zeros(B, H, Tq, 8)
    assert ops._dattn_operand(same, 8) is same
