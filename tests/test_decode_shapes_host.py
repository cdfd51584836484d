"""Host-side companions of test_hip_decode_shapes.py: the width the decode LayerNorm refuses (through the C ABI, before any
launch) and the state-dict contract of the "wide" configuration the engine is run at there."""
import ctypes

from oracle import fill_state, model_config, state_spec


def test_decode_layernorm_refuses_more_than_1024_columns():
    from transformertts_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    a = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)          # a host address: never dereferenced
    for rc in (lib.ttts_decode_layernorm(a, a, a, a, 1, 1025, 1e-5, a, None),
               lib.ttts_decode_layernorm_rows(a, a, a, a, 1, 1025, 1e-5, a, a, None)):
        assert rc == -1, rc
        assert "bad sizes" in _lib.last_error() and "d=1025" in _lib.last_error(), _lib.last_error()
    for d in (0, -4):
        assert lib.ttts_decode_layernorm(a, a, a, a, 1, d, 1e-5, a, None) == -1
        assert "bad sizes" in _lib.last_error(), _lib.last_error()


def test_wide_config_sits_on_the_synthesizer_s_limits():
    cfg = model_config("wide")
    d, H = cfg["d_model"], cfg["decoder_n_head"]
    assert (d, cfg["decoder_d_ffn"], d // H) == (1024, 4096, 128)
    assert cfg["encoder_n_layers"] == cfg["decoder_n_layers"] == 1
    spec = state_spec(cfg)
    assert spec["decoder.layers.0.linear1.weight"] == (4096, 1024) and spec["decoder.layers.0.linear2.weight"] == (1024, 4096)
    assert spec["decoder.layers.0.self_attn.in_proj_weight"] == (3072, 1024)
    sd = fill_state(cfg, 3)
    assert list(sd) == list(spec) and all(tuple(sd[k].shape) == tuple(spec[k]) for k in spec)
