"""`Synthesizer.synthesize(window=AttentionWindow(...))`: the refusals, and the argument checks of
ttts_decode_attention_window (ABI v21).  Host logic only."""
import ctypes
import os
import re

import pytest
import torch


def _model(name="tiny", **over):
    from oracle import model_config
    from transformertts_amd.model import TransformerTTS
    cfg = dict(model_config(name), **over)
    return cfg, TransformerTTS(**cfg, device="cpu")


def _inputs(B=2, Tp=7):
    return torch.zeros(B, Tp, dtype=torch.int64), torch.full((B,), Tp, dtype=torch.int64)


def test_abi_version_and_the_header_declares_the_window():
    from transformertts_amd import _lib
    lib = _lib.load()
    assert lib.ttts_abi_version() >= 21
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "ttts_hip.h")).read()
    assert re.search(r"\bint\s+ttts_decode_attention_window\s*\(", header)
    assert "ttts_decode_attention_window" in _lib.SIGNATURES and hasattr(lib, "ttts_decode_attention_window")
    struct = re.search(r"typedef struct ttts_decode_window \{(.*?)\} ttts_decode_window;", header, re.S)
    assert struct, "the header declares no ttts_decode_window"
    fields = re.findall(r"\b(u?int(?:32|64)_t)\s+(\w+);", struct.group(1))
    assert fields == [("int32_t", "back"), ("int32_t", "ahead"), ("int32_t", "guide_head"), ("int32_t", "pad"),
                      ("uint64_t", "head_mask"), ("int64_t", "reserved")], fields            # 32 bytes, fixed offsets
    assert re.search(r"const ttts_decode_window\*\s*win,\s*int32_t\*\s*pos,\s*int64_t\s+ld_pos", header)


def test_the_package_exports_the_window():
    import transformertts_amd
    from transformertts_amd.synthesis import AttentionWindow
    assert transformertts_amd.AttentionWindow is AttentionWindow and "AttentionWindow" in transformertts_amd.__all__
    w = AttentionWindow(guide=(1, 0))
    assert (w.back, w.ahead, w.layers, w.heads) == (1, 3, None, None)
    with pytest.raises(Exception):
        w.back = 2                                                   # frozen


def test_synthesize_with_a_window_reaches_the_device_check():
    """a valid window on a CPU model is refused for the device only (on a tree without the feature: a TypeError)"""
    from transformertts_amd.synthesis import AttentionWindow, Synthesizer
    cfg, m = _model()
    synth = Synthesizer(m)
    L, H = cfg["decoder_n_layers"], cfg["decoder_n_head"]
    for w in (AttentionWindow((0, 0)), AttentionWindow((L - 1, H - 1), 0, 0), AttentionWindow((1, 1), 5, 2 ** 40),
              AttentionWindow((1, 0), layers=[1], heads=(0,)), AttentionWindow((0, 1), layers=range(L), heads=[1, 0])):
        with pytest.raises(ValueError, match="`model` must be on the HIP device"):
            synth.synthesize(*_inputs(), max_len=20, window=w)
        with pytest.raises(ValueError, match="`model` must be on the HIP device"):
            synth.synthesize(*_inputs(), max_len=20, alignments=True, window=w)
    assert synth.captures == 0 and synth.shape_bytes() == {}


def test_window_refusals_before_the_device():
    from transformertts_amd.synthesis import AttentionWindow, Synthesizer
    cfg, m = _model()
    synth = Synthesizer(m)
    L, H = cfg["decoder_n_layers"], cfg["decoder_n_head"]
    assert (L, H) == (2, 2)

    def refused(match, w):
        with pytest.raises(ValueError, match=match):
            synth.synthesize(*_inputs(), max_len=20, window=w)

    for bad in ((1, 0, 1, 3), {"guide": (0, 0)}, "window", 3, True):
        refused("`window` must be an AttentionWindow", bad)
    # a guide outside the model
    for g in ((L, 0), (0, H), (-1, 0), (0, -1)):
        refused(r"`window.guide`.*outside the model", AttentionWindow(g))
    for g in (0, (0,), (0, 0, 0), (0.0, 0), "00", (True, 0), None):
        refused("`window.guide` must be a", AttentionWindow(g))
    # a guide that is not among the constrained (layer, head)s
    refused("not among the constrained", AttentionWindow((0, 0), layers=[1]))
    refused("not among the constrained", AttentionWindow((0, 0), heads=[1]))
    refused("not among the constrained", AttentionWindow((1, 1), layers=[1], heads=[0]))
    refused("not among the constrained", AttentionWindow((0, 0), layers=[]))
    # back / ahead
    for bad in (-1, 1.0, 2.5, "1", None, True):
        refused("`window.back` must be a non-negative integer", AttentionWindow((0, 0), back=bad))
        refused("`window.ahead` must be a non-negative integer", AttentionWindow((0, 0), ahead=bad))
    # indices out of range, duplicated, of the wrong kind
    refused("`window.layers`.*out of range", AttentionWindow((0, 0), layers=[0, L]))
    refused("`window.layers`.*out of range", AttentionWindow((0, 0), layers=[-1, 0]))
    refused("`window.heads`.*out of range", AttentionWindow((0, 0), heads=[0, H]))
    refused("`window.layers` holds an index twice", AttentionWindow((0, 0), layers=[0, 0]))
    refused("`window.heads` holds an index twice", AttentionWindow((0, 0), heads=[1, 0, 1]))
    refused("`window.heads` must hold integers", AttentionWindow((0, 0), heads=[0.0]))
    refused("`window.layers` must be None or a sequence", AttentionWindow((0, 0), layers=0))
    refused("`window.heads` must be None or a sequence", AttentionWindow((0, 0), heads="01"))
    # the other arguments are still checked, and the model's structure comes first
    with pytest.raises(ValueError, match="`alignments` must be a bool"):
        synth.synthesize(*_inputs(), alignments=1, window=AttentionWindow((0, 0)))
    with pytest.raises(ValueError, match="`max_len`"):
        synth.synthesize(*_inputs(), max_len=1, window=AttentionWindow((0, 0)))
    m.decoder.layers[1].norm_first = True
    refused("`model`.*norm_first", AttentionWindow((0, 0)))
    m.decoder.layers[1].norm_first = False
    assert synth.captures == 0 and synth.shape_bytes() == {}


def test_more_than_64_decoder_heads_are_refused():
    """(d_model <= 1024 and heads of at least 16 columns leave at most 64 heads today: the check is for the head mask's sake)"""
    from transformertts_amd.synthesis import AttentionWindow, Synthesizer
    cfg, m = _model()
    synth = Synthesizer(m)
    for l in m.decoder.layers:
        l.self_attn.num_heads = l.multihead_attn.num_heads = 65
    with pytest.raises(ValueError, match="at most 64 decoder heads, the model has 65"):
        synth.synthesize(*_inputs(), max_len=20, window=AttentionWindow((0, 0)))
    assert synth.captures == 0 and synth.shape_bytes() == {}


def test_window_structs():
    """what _decode copies to the device: per layer (back, ahead, guide head or -1, head mask)"""
    from transformertts_amd.synthesis import AttentionWindow, Synthesizer
    cfg, m = _model()
    synth = Synthesizer(m)
    assert synth._check_window(AttentionWindow((1, 0))) == [(1, 3, -1, 3), (1, 3, 0, 3)]
    assert synth._check_window(AttentionWindow((0, 1), 0, 7, layers=[0], heads=[1])) == [(0, 7, 1, 2), (0, 7, -1, 0)]
    assert synth._check_window(AttentionWindow((0, 0), 2 ** 40, 2 ** 31)) == [(2 ** 31 - 1, 2 ** 31 - 1, 0, 3),
                                                                             (2 ** 31 - 1, 2 ** 31 - 1, -1, 3)]


def test_window_entry_point_rejects_null_pointers_and_bad_sizes():
    from transformertts_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096 + 16)
    a = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)          # a 16-byte aligned host address (never dereferenced)
    odd = ctypes.c_void_p(a.value + 4)
    ws = lib.ttts_decode_attention_workspace_bytes(1, 4, 64, 100)

    def bad(rc, needle):
        assert rc == -1, rc
        assert needle in _lib.last_error(), _lib.last_error()

    # ttts_decode_attention_window(q, ldq, k, v, ld_row, ld_batch, lens, out, ldo, ws, ws_bytes, B, H, hd, max_keys, row_end,
    #                              map, map_ld_head, map_ld_row, map_rows, win, pos, ld_pos, st, stream)
    def attn(q=a, k=a, ld_row=512, lens=a, ws_bytes=ws, B=1, H=4, hd=64, row_end=a, amap=None, ld_head=0, ld_mrow=0, rows=0,
             win=a, pos=a, ld_pos=8, st=a, ldq=256):
        return lib.ttts_decode_attention_window(q, ldq, k, a, ld_row, 0, lens, a, ldq, a, ws_bytes, B, H, hd, 100, row_end, amap,
                                                ld_head, ld_mrow, rows, win, pos, ld_pos, st, None)

    bad(attn(row_end=None), "null pointer (row_end)")
    bad(attn(lens=None), "null pointer (lens)")
    bad(attn(win=None), "null pointer (win)")
    bad(attn(pos=None), "null pointer (pos)")
    bad(attn(k=None), "null pointer")
    bad(attn(st=None), "null pointer")
    bad(attn(hd=24), "head_dim=24")
    bad(attn(H=1, hd=256), "head_dim=256")
    bad(attn(ws_bytes=ws - 4), "workspace")
    bad(attn(ld_row=100), "strides")
    bad(attn(B=0), "bad sizes")
    bad(attn(q=odd), "16-byte aligned")
    bad(attn(H=65, hd=16, ldq=65 * 16, ld_row=65 * 16, ws_bytes=lib.ttts_decode_attention_workspace_bytes(1, 65, 16, 100)),
        "H=65 heads")
    bad(attn(ld_pos=0), "ld_pos=0")
    bad(attn(win=odd), "aligned")
    bad(attn(pos=ctypes.c_void_p(a.value + 2)), "aligned")
    bad(attn(amap=a, ld_head=128 * 8, ld_mrow=64, rows=8), "map of 8 rows")          # ld_row < max_keys = 100
    bad(attn(amap=a, ld_head=128 * 8 - 1, ld_mrow=128, rows=8), "map of 8 rows")     # ld_head < rows * ld_row
    bad(attn(amap=a, ld_head=1024, ld_mrow=128, rows=0), "map of 0 rows")
