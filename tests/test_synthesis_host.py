"""Synthesizer refusals and the decode entry points' argument checks: host logic only, no GPU."""
import ctypes

import pytest
import torch


def _model(name="tiny", **over):
    from oracle import model_config
    from transformertts_amd.model import TransformerTTS
    cfg = dict(model_config(name), **over)
    return TransformerTTS(**cfg, device="cpu")


def _inputs(B=2, Tp=7):
    return torch.zeros(B, Tp, dtype=torch.int64), torch.full((B,), Tp, dtype=torch.int64)


def test_refuses_norm_first_decoder_layers():
    from transformertts_amd.synthesis import Synthesizer
    m = _model()
    m.decoder.layers[1].norm_first = True
    with pytest.raises(ValueError, match="`model`.*norm_first"):
        Synthesizer(m)(*_inputs())


def test_refuses_a_final_decoder_norm():
    from transformertts_amd.synthesis import Synthesizer
    m = _model()
    m.decoder.norm = torch.nn.LayerNorm(m.emb.weight.shape[1])
    with pytest.raises(ValueError, match="`model`.*norm"):
        Synthesizer(m)(*_inputs())


@pytest.mark.parametrize("d,heads", [(96, 4), (256, 1)])      # head_dim 24 (not a multiple of 16), head_dim 256 (> 128)
def test_refuses_head_dims_the_kernels_do_not_take(d, heads):
    from transformertts_amd.synthesis import Synthesizer
    m = _model(d_model=d, encoder_prenet_in_channel=d, encoder_prenet_out_channel=d, encoder_n_head=heads, decoder_n_head=heads)
    assert d // heads in (24, 256)
    with pytest.raises(ValueError, match="`model` head_dim"):
        Synthesizer(m)


@pytest.mark.parametrize("max_len", [1, 0, 5002])
def test_refuses_max_len_before_the_device_check(max_len):
    from transformertts_amd.synthesis import Synthesizer
    m = _model()
    assert m.pe.pe.shape[0] == 5000
    with pytest.raises(ValueError, match="`max_len`"):
        Synthesizer(m)(*_inputs(), max_len=max_len)


def test_refuses_a_model_or_inputs_off_the_device_and_non_fp32_parameters():
    from transformertts_amd.synthesis import Synthesizer
    m = _model()
    synth = Synthesizer(m)
    with pytest.raises(ValueError, match="`model` must be on the HIP device"):
        synth(*_inputs(), max_len=5001)           # the largest max_len the table takes passes the structural checks
    m2 = _model().double()
    with pytest.raises(ValueError, match="`model`"):
        Synthesizer(m2)(*_inputs())
    with pytest.raises(ValueError, match="`max_shapes`"):
        Synthesizer(m, max_shapes=0)


def test_decode_entry_points_reject_null_pointers_and_bad_sizes():
    from transformertts_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096 + 16)
    a = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)          # a 16-byte aligned host address (never dereferenced)

    def bad(rc, needle):
        assert rc == -1, rc
        assert needle in _lib.last_error(), _lib.last_error()

    # ttts_decode_linear(x, ldx, x_ts, w, bias, res, ldr, y, ldy, y_ts, y2, ldy2, y2_ts, n_split, M, N, K, act, st, stream)
    bad(lib.ttts_decode_linear(None, 16, 0, a, None, None, 0, a, 16, 0, None, 0, 0, 16, 1, 16, 16, 0, a, None), "null pointer")
    bad(lib.ttts_decode_linear(a, 16, 0, a, None, None, 0, a, 16, 0, None, 0, 0, 16, 1, 16, 16, 0, None, None), "null pointer")
    bad(lib.ttts_decode_linear(a, 16, 0, a, None, None, 0, a, 16, 0, None, 0, 0, 16, 1, 16, 18, 0, a, None), "bad sizes")
    bad(lib.ttts_decode_linear(a, 16, 0, a, None, None, 0, a, 16, 0, None, 0, 0, 16, 0, 16, 16, 0, a, None), "bad sizes")
    bad(lib.ttts_decode_linear(a, 8192, 0, a, None, None, 0, a, 16, 0, None, 0, 0, 16, 1, 16, 8192, 0, a, None), "bad sizes")
    bad(lib.ttts_decode_linear(a, 16, 0, a, None, None, 0, a, 16, 0, None, 0, 0, 8, 1, 16, 16, 0, a, None), "null pointer (y2")
    bad(lib.ttts_decode_linear(a, 16, 0, a, None, None, 0, a, 16, 0, None, 0, 0, 16, 1, 16, 16, 2, a, None), "act=2")
    bad(lib.ttts_decode_linear(a, 8, 0, a, None, None, 0, a, 16, 0, None, 0, 0, 16, 2, 16, 16, 0, a, None), "ldx=8 < K=16")
    bad(lib.ttts_decode_linear(ctypes.c_void_p(a.value + 4), 16, 0, a, None, None, 0, a, 16, 0, None, 0, 0, 16, 1, 16, 16, 0,
                               a, None), "16-byte aligned")
    # ttts_decode_frame_in(ys, ld_ys, n_mels, w1, b1, w2, b2, pe, alpha, tmp, out, B, d, st, stream)
    bad(lib.ttts_decode_frame_in(a, 80, 80, a, None, a, None, None, a, a, a, 1, 256, a, None), "null pointer")
    bad(lib.ttts_decode_frame_in(a, 80, 80, a, None, a, None, a, a, a, a, 1, 250, a, None), "bad sizes")
    # ttts_decode_frame_out(x, w_mel, b_mel, w_stop, b_stop, ys, ld_ys, stop, ld_stop, B, d, n_mels, st, stream)
    bad(lib.ttts_decode_frame_out(a, a, None, a, None, a, 80, None, 16, 1, 256, 80, a, None), "null pointer")
    bad(lib.ttts_decode_frame_out(a, a, None, a, None, a, 80, a, 16, 0, 256, 80, a, None), "bad sizes")
    # ttts_decode_layernorm(x, gamma, beta, y, M, d, eps, st, stream)
    bad(lib.ttts_decode_layernorm(a, None, a, a, 1, 256, 1e-5, a, None), "null pointer")
    bad(lib.ttts_decode_layernorm(a, a, a, a, 1, 2048, 1e-5, a, None), "bad sizes")
    # ttts_decode_attention(q, ldq, k, v, ld_row, ld_batch, lens, out, ldo, ws, ws_bytes, B, H, hd, max_keys, st, stream)
    ws = lib.ttts_decode_attention_workspace_bytes(1, 4, 64, 100)
    assert ws == 1 * 4 * 2 * (64 + 4) * 4
    assert lib.ttts_decode_attention_workspace_bytes(1, 4, 64, 0) == 0
    bad(lib.ttts_decode_attention(a, 256, None, a, 512, 0, None, a, 256, a, ws, 1, 4, 64, 100, a, None), "null pointer")
    bad(lib.ttts_decode_attention(a, 256, a, a, 512, 0, None, a, 256, a, ws, 1, 8, 32, 100, None, None), "null pointer")
    bad(lib.ttts_decode_attention(a, 256, a, a, 512, 0, None, a, 256, a, ws, 1, 4, 24, 100, a, None), "head_dim=24")
    bad(lib.ttts_decode_attention(a, 256, a, a, 512, 0, None, a, 256, a, ws, 1, 1, 256, 100, a, None), "head_dim=256")
    bad(lib.ttts_decode_attention(a, 256, a, a, 512, 0, None, a, 256, a, ws - 4, 1, 4, 64, 100, a, None), "workspace")
    bad(lib.ttts_decode_attention(a, 256, a, a, 100, 0, None, a, 256, a, ws, 1, 4, 64, 100, a, None), "strides")
    bad(lib.ttts_decode_attention(a, 256, a, a, 512, 0, None, a, 256, a, ws, 0, 4, 64, 100, a, None), "bad sizes")
    with pytest.raises(RuntimeError):
        _lib.check(-1, "ttts_decode_attention")
