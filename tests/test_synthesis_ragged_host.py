"""`Synthesizer.synthesize` refusals and the argument checks of the per-row decode entry points (ABI v16): host logic only."""
import ctypes
import os
import re

import pytest
import torch


def _model(name="tiny", **over):
    from oracle import model_config
    from transformertts_amd.model import TransformerTTS
    cfg = dict(model_config(name), **over)
    return TransformerTTS(**cfg, device="cpu")


def _inputs(B=2, Tp=7):
    return torch.zeros(B, Tp, dtype=torch.int64), torch.full((B,), Tp, dtype=torch.int64)


def test_synthesize_refuses_what_call_refuses_before_the_device():
    from transformertts_amd.synthesis import Synthesizer
    m = _model()
    synth = Synthesizer(m)
    for max_len in (1, 0, 5002):
        with pytest.raises(ValueError, match="`max_len`"):
            synth.synthesize(*_inputs(), max_len=max_len)
    with pytest.raises(ValueError, match="`model` must be on the HIP device"):
        synth.synthesize(*_inputs(), max_len=5001)
    with pytest.raises(ValueError, match="`model` must be on the HIP device"):
        synth.synthesize(*_inputs(), max_len=20, stop_threshold=0.5, alignments=True)
    for bad in (1, 0, None, "yes", torch.tensor(True)):
        with pytest.raises(ValueError, match="`alignments` must be a bool"):
            synth.synthesize(*_inputs(), alignments=bad)
    m.decoder.layers[1].norm_first = True
    with pytest.raises(ValueError, match="`model`.*norm_first"):
        synth.synthesize(*_inputs())
    m.decoder.layers[1].norm_first = False
    m.decoder.norm = torch.nn.LayerNorm(m.emb.weight.shape[1])
    with pytest.raises(ValueError, match="`model`.*norm"):
        synth.synthesize(*_inputs())
    with pytest.raises(ValueError, match="`model`"):
        Synthesizer(_model().double()).synthesize(*_inputs())
    assert synth.captures == 0 and synth.shape_bytes() == {}


def test_abi_version_and_the_header_declares_the_per_row_entry_points():
    from transformertts_amd import _lib
    lib = _lib.load()
    assert lib.ttts_abi_version() >= 16
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "ttts_hip.h")).read()
    for name in ("ttts_decode_linear_rows", "ttts_decode_frame_in_rows", "ttts_decode_frame_out_rows",
                 "ttts_decode_layernorm_rows", "ttts_decode_attention_rows", "ttts_mask_rows"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "TTTS_DECODE_PER_ROW" in header


def test_per_row_entry_points_reject_null_pointers_and_bad_sizes():
    from transformertts_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096 + 16)
    a = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)          # a 16-byte aligned host address (never dereferenced)
    odd = ctypes.c_void_p(a.value + 4)

    def bad(rc, needle):
        assert rc == -1, rc
        assert needle in _lib.last_error(), _lib.last_error()

    # ttts_decode_linear_rows(x, ldx, x_ts, w, bias, res, ldr, y, ldy, y_ts, y2, ldy2, y2_ts, n_split, M, N, K, act, row_end, st, stream)
    bad(lib.ttts_decode_linear_rows(a, 16, 0, a, None, None, 0, a, 16, 0, None, 0, 0, 16, 1, 16, 16, 0, None, a, None),
        "null pointer (row_end)")
    bad(lib.ttts_decode_linear_rows(None, 16, 0, a, None, None, 0, a, 16, 0, None, 0, 0, 16, 1, 16, 16, 0, a, a, None), "null pointer")
    bad(lib.ttts_decode_linear_rows(a, 16, 0, a, None, None, 0, a, 16, 0, None, 0, 0, 16, 1, 16, 16, 0, a, None, None), "null pointer")
    bad(lib.ttts_decode_linear_rows(a, 16, 0, a, None, None, 0, a, 16, 0, None, 0, 0, 16, 1, 16, 18, 0, a, a, None), "bad sizes")
    bad(lib.ttts_decode_linear_rows(a, 16, 0, a, None, None, 0, a, 16, 0, None, 0, 0, 8, 1, 16, 16, 0, a, a, None), "null pointer (y2")
    bad(lib.ttts_decode_linear_rows(odd, 16, 0, a, None, None, 0, a, 16, 0, None, 0, 0, 16, 1, 16, 16, 0, a, a, None), "16-byte aligned")
    # ttts_decode_frame_in_rows(ys, ld_ys, n_mels, w1, b1, w2, b2, pe, alpha, tmp, out, B, d, row_end, st, stream)
    bad(lib.ttts_decode_frame_in_rows(a, 80, 80, a, None, a, None, a, a, a, a, 1, 256, None, a, None), "null pointer (row_end)")
    bad(lib.ttts_decode_frame_in_rows(a, 80, 80, a, None, a, None, None, a, a, a, 1, 256, a, a, None), "null pointer")
    bad(lib.ttts_decode_frame_in_rows(a, 80, 80, a, None, a, None, a, a, a, a, 1, 250, a, a, None), "bad sizes")
    # ttts_decode_frame_out_rows(x, w_mel, b_mel, w_stop, b_stop, ys, ld_ys, stop, ld_stop, B, d, n_mels, row_end, st, stream)
    bad(lib.ttts_decode_frame_out_rows(a, a, None, a, None, a, 80, a, 16, 1, 256, 80, None, a, None), "null pointer (row_end)")
    bad(lib.ttts_decode_frame_out_rows(a, a, None, a, None, a, 80, None, 16, 1, 256, 80, a, a, None), "null pointer")
    bad(lib.ttts_decode_frame_out_rows(a, a, None, a, None, a, 80, a, 16, 0, 256, 80, a, a, None), "bad sizes")
    bad(lib.ttts_decode_frame_out_rows(a, a, None, odd, None, a, 80, a, 16, 1, 256, 80, a, a, None), "16-byte aligned")
    # ttts_decode_layernorm_rows(x, gamma, beta, y, M, d, eps, row_end, st, stream)
    bad(lib.ttts_decode_layernorm_rows(a, a, a, a, 1, 256, 1e-5, None, a, None), "null pointer (row_end)")
    bad(lib.ttts_decode_layernorm_rows(a, None, a, a, 1, 256, 1e-5, a, a, None), "null pointer")
    bad(lib.ttts_decode_layernorm_rows(a, a, a, a, 1, 2048, 1e-5, a, a, None), "bad sizes")
    # ttts_decode_attention_rows(q, ldq, k, v, ld_row, ld_batch, lens, out, ldo, ws, ws_bytes, B, H, hd, max_keys, row_end,
    #                            map, map_ld_head, map_ld_row, map_rows, st, stream)
    ws = lib.ttts_decode_attention_workspace_bytes(1, 4, 64, 100)

    def attn(q=a, k=a, ld_row=512, ws_bytes=ws, B=1, H=4, hd=64, row_end=a, amap=None, ld_head=0, ld_mrow=0, rows=0, st=a):
        return lib.ttts_decode_attention_rows(q, 256, k, a, ld_row, 0, None, a, 256, a, ws_bytes, B, H, hd, 100, row_end, amap,
                                              ld_head, ld_mrow, rows, st, None)

    bad(attn(row_end=None), "null pointer (row_end)")
    bad(attn(k=None), "null pointer")
    bad(attn(st=None), "null pointer")
    bad(attn(hd=24), "head_dim=24")
    bad(attn(H=1, hd=256), "head_dim=256")
    bad(attn(ws_bytes=ws - 4), "workspace")
    bad(attn(ld_row=100), "strides")
    bad(attn(B=0), "bad sizes")
    bad(attn(q=odd), "16-byte aligned")
    bad(attn(amap=a, ld_head=128 * 8, ld_mrow=64, rows=8), "map of 8 rows")          # ld_row < max_keys = 100
    bad(attn(amap=a, ld_head=128 * 8 - 1, ld_mrow=128, rows=8), "map of 8 rows")     # ld_head < rows * ld_row
    bad(attn(amap=a, ld_head=1024, ld_mrow=128, rows=0), "map of 0 rows")
    # ttts_mask_rows(x, lens, outer, group, T, C, stream)
    bad(lib.ttts_mask_rows(None, a, 1, 1, 4, 4, None), "null pointer")
    bad(lib.ttts_mask_rows(a, None, 1, 1, 4, 4, None), "null pointer")
    bad(lib.ttts_mask_rows(a, a, 0, 1, 4, 4, None), "bad sizes")
    bad(lib.ttts_mask_rows(a, a, 70000, 1, 4, 4, None), "bad sizes")
    bad(lib.ttts_mask_rows(a, a, 1, 0, 4, 4, None), "bad sizes")
    bad(lib.ttts_mask_rows(a, a, 1, 1, 0, 4, None), "bad sizes")
    bad(lib.ttts_mask_rows(a, a, 1, 1, 4, 0, None), "bad sizes")
    bad(lib.ttts_mask_rows(ctypes.c_void_p(a.value + 2), a, 1, 1, 4, 4, None), "4-byte aligned")
