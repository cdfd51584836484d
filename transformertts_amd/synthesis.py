"""Synthesizer: `TransformerTTS.inference` as replays of a captured HIP graph on the decode kernels of csrc/decode.hip.

    synth = Synthesizer(model)
    out = synth(phoneme, phoneme_lens, max_len=1500, stop_threshold=0.5)     # the dict model.inference(...) returns

Same semantics as the reference's `inference` (model/model.py:323-394) and as `TransformerTTS.inference`: eval mode (the model
is left in it), the encoder runs without a padding mask, cross-attention is masked by `phoneme_lens`, decoding stops at the
first frame where every utterance's stop probability reaches the threshold or after `max_len - 1` frames, and the post-net
runs once at the end.

Per call, the encoder, the memory K/V projection of every decoder layer and the post-net run once, eagerly, on the `ops` path.
The frames run on the decode kernels alone: one frame is a fixed launch sequence (pre-net + positional encoding, per layer
the in-projection with its K/V written into the layer's cache, self-attention, out-projection, LayerNorm, cross q,
cross-attention, out-projection, LayerNorm, FFN, LayerNorm, then the heads and the stop decision) whose frame index, length,
threshold and stop state live in a device-side `ttts_decode_state`.  `chunk` frames of it are captured as ONE graph per
batch shape; a call resets the state with one small host-to-device copy and replays the graph until the state read back
after a chunk says the decoding has ended.  Frames replayed past the end return at once and change nothing.

Graphs and their static buffers are cached per (B, Tp rounded up to 64, capacity rounded up to 256 frames), least recently
used evicted beyond `max_shapes`.  The kernels read the parameters' own storage, so in-place updates (`load_state_dict`,
FlatAdam, `.data` writes into the same storage) are seen by the next call; a parameter whose storage moved (replaced, or the
module moved) makes the next call drop the graphs and capture again.
"""
from __future__ import annotations

from collections import OrderedDict
from ctypes import c_void_p

import torch

from . import _lib, ops

_CAPTURE_MODE = "thread_local"      # as step.py: illegal-during-capture checks confined to the capturing thread
_TP_ROUND = 64
_CAP_ROUND = 256
_ACT_NONE, _ACT_RELU = 0, 1


def _up(x: int, m: int) -> int:
    return -(-x // m) * m


def _ptr(t: torch.Tensor, offset_floats: int = 0) -> c_void_p:
    return c_void_p(t.data_ptr() + 4 * offset_floats)


class _Shape:
    """Static buffers of one (B, Tp_pad, cap) and the chunk graph captured over them."""

    def __init__(self, model, B: int, Tp_pad: int, cap: int, dev):
        d = model.emb.weight.shape[1]
        layers = list(model.decoder.layers)
        d_ffn = layers[0].linear1.weight.shape[0]
        H = layers[0].self_attn.num_heads
        nm = model.n_mels
        f32 = dict(dtype=torch.float32, device=dev)
        self.B, self.Tp_pad, self.cap = B, Tp_pad, cap
        self.state = torch.zeros(4, dtype=torch.int64, device=dev)          # ttts_decode_state (32 bytes)
        self.ys = torch.zeros(B, cap, nm, **f32)                             # frame 0 (the go frame) stays zero
        self.stop = torch.zeros(B, cap, **f32)
        self.h = torch.zeros(B, d, **f32)
        self.tmp = torch.zeros(B, d, **f32)
        self.q = torch.zeros(B, d, **f32)
        self.ctx = torch.zeros(B, d, **f32)
        self.ffn = torch.zeros(B, d_ffn, **f32)
        self.cache = [torch.zeros(B, cap, 2 * d, **f32) for _ in layers]
        self.memkv = [torch.zeros(B, Tp_pad, 2 * d, **f32) for _ in layers]
        self.lens = torch.zeros(B, dtype=torch.int64, device=dev)
        lib = _lib.load()
        self.ws_bytes = max(lib.ttts_decode_attention_workspace_bytes(B, H, d // H, cap),
                            lib.ttts_decode_attention_workspace_bytes(B, H, d // H, Tp_pad))
        self.ws = torch.zeros(max(self.ws_bytes // 4, 4), **f32)
        self.calls = None
        self.graph = None

    def nbytes(self) -> int:
        ts = [self.state, self.ys, self.stop, self.h, self.tmp, self.q, self.ctx, self.ffn, self.lens, self.ws]
        return sum(t.numel() * t.element_size() for t in ts + self.cache + self.memkv)


class Synthesizer:
    """Graph-replayed greedy synthesis for one TransformerTTS model (see the module docstring)."""

    def __init__(self, model, max_shapes: int = 4, chunk: int = 16):
        if int(max_shapes) < 1:
            raise ValueError("Synthesizer: `max_shapes` must be at least 1")
        if int(chunk) < 1:
            raise ValueError("Synthesizer: `chunk` must be at least 1")
        _check_structure(model)
        self.model = model
        self.max_shapes = int(max_shapes)
        self._chunk = int(chunk)
        self._shapes: "OrderedDict[tuple, _Shape]" = OrderedDict()
        self._weights_sig = None
        self._side = None
        self.captures = 0            # chunk graphs captured so far (a shape's first call, or after its weights moved)
        self.recaptures = 0          # times moved parameter storage dropped the captured graphs

    @property
    def chunk(self) -> int:
        """frames per captured graph (one replay, then one device-to-host read of the decode state)"""
        return self._chunk

    def shape_bytes(self) -> dict:
        """static-buffer footprint of every cached shape, {(B, Tp_pad, cap): bytes}"""
        return {k: s.nbytes() for k, s in self._shapes.items()}

    # ------------------------------------------------------------------------------------------------------ checks
    def _check_call(self, phoneme, phoneme_lens, max_len):
        m = self.model
        _check_structure(m)
        if int(max_len) < 2:
            raise ValueError(f"Synthesizer: `max_len` must be at least 2 (one decoded frame), got {max_len}")
        pe_rows = m.pe.pe.shape[0]
        if int(max_len) - 1 > pe_rows:
            raise ValueError(f"Synthesizer: `max_len` - 1 = {int(max_len) - 1} frames exceed the positional-encoding table "
                             f"({pe_rows} rows)")
        params = list(m.parameters())
        if not all(p.is_cuda for p in params) or not m.pe.pe.is_cuda:
            raise ValueError("Synthesizer: `model` must be on the HIP device (there is no CPU path)")
        if not all(p.dtype == torch.float32 for p in params) or m.pe.pe.dtype != torch.float32:
            raise ValueError("Synthesizer: `model` parameters must be fp32")
        dev = params[0].device
        if not (torch.is_tensor(phoneme) and phoneme.is_cuda and phoneme.device == dev):
            raise ValueError("Synthesizer: `phoneme` must be on the model's HIP device")
        if not (torch.is_tensor(phoneme_lens) and phoneme_lens.is_cuda and phoneme_lens.device == dev):
            raise ValueError("Synthesizer: `phoneme_lens` must be on the model's HIP device")
        if phoneme.dim() != 2 or phoneme.size(0) < 1 or phoneme.size(1) < 1:
            raise ValueError(f"Synthesizer: `phoneme` must be (B, Tp), got {tuple(phoneme.shape)}")
        if tuple(phoneme_lens.shape) != (phoneme.size(0),):
            raise ValueError(f"Synthesizer: `phoneme_lens` must be (B,) = ({phoneme.size(0)},), got {tuple(phoneme_lens.shape)}")

    # ------------------------------------------------------------------------------------------------------ weights
    def _weight_tensors(self):
        m = self.model
        ts = [m.dec_prenet.linear1.linear.weight, m.dec_prenet.linear1.linear.bias, m.dec_prenet.linear2.linear.weight,
              m.dec_prenet.linear2.linear.bias, m.pe.pe, m.pe.alpha, m.linear1.linear.weight, m.linear1.linear.bias,
              m.linear2.linear.weight, m.linear2.linear.bias]
        for l in m.decoder.layers:
            ts += [l.self_attn.in_proj_weight, l.self_attn.in_proj_bias, l.self_attn.out_proj.weight, l.self_attn.out_proj.bias,
                   l.multihead_attn.in_proj_weight, l.multihead_attn.in_proj_bias, l.multihead_attn.out_proj.weight,
                   l.multihead_attn.out_proj.bias, l.linear1.weight, l.linear1.bias, l.linear2.weight, l.linear2.bias,
                   l.norm1.weight, l.norm1.bias, l.norm2.weight, l.norm2.bias, l.norm3.weight, l.norm3.bias]
        return ts

    def _follow_weights(self):
        sig = tuple(t.data_ptr() for t in self._weight_tensors())
        if self._weights_sig is not None and sig != self._weights_sig:
            for s in self._shapes.values():
                s.graph = None
                s.calls = None
            self.recaptures += 1
        self._weights_sig = sig

    # ------------------------------------------------------------------------------------------------------ shapes
    def _shape(self, B: int, Tp: int, max_len: int, dev) -> _Shape:
        Tp_pad = _up(Tp, _TP_ROUND)
        fits = [k for k in self._shapes if k[0] == B and k[1] == Tp_pad and k[2] >= max_len]
        if fits:
            key = min(fits, key=lambda k: k[2])
        else:
            key = (B, Tp_pad, _up(max_len, _CAP_ROUND))
            while len(self._shapes) >= self.max_shapes:
                self._shapes.popitem(last=False)        # (the side stream is idle: every call ends in a synchronising read)
            self._shapes[key] = _Shape(self.model, B, Tp_pad, key[2], dev)
        self._shapes.move_to_end(key)
        return self._shapes[key]

    def _frame_calls(self, sh: _Shape):
        """the launch sequence of one frame: [(entry point, arguments without the stream)]"""
        lib = _lib.load()
        m = self.model
        layers = list(m.decoder.layers)
        B, cap, nm = sh.B, sh.cap, m.n_mels
        d = m.emb.weight.shape[1]
        H = layers[0].self_attn.num_heads
        hd = d // H
        d_ffn = layers[0].linear1.weight.shape[0]
        st = _ptr(sh.state)
        h, tmp, q, ctx, ffn, ws = _ptr(sh.h), _ptr(sh.tmp), _ptr(sh.q), _ptr(sh.ctx), _ptr(sh.ffn), _ptr(sh.ws)
        p1, p2 = m.dec_prenet.linear1.linear, m.dec_prenet.linear2.linear
        calls = [(lib.ttts_decode_frame_in, (_ptr(sh.ys), cap * nm, nm, _ptr(p1.weight), _ptr(p1.bias), _ptr(p2.weight),
                                             _ptr(p2.bias), _ptr(m.pe.pe), _ptr(m.pe.alpha), tmp, h, B, d, st))]

        def linear(x, K, w, b, y, N, res=None, act=_ACT_NONE):
            return (lib.ttts_decode_linear, (x, K, 0, _ptr(w), _ptr(b), res, d if res is not None else 0, y, N, 0, None, 0, 0,
                                             N, B, N, K, act, st))

        for l, cache, mkv in zip(layers, sh.cache, sh.memkv):
            sa, ca = l.self_attn, l.multihead_attn
            # in-projection: q to `q`, the K/V columns straight into row t - 1 of this layer's cache
            calls.append((lib.ttts_decode_linear, (h, d, 0, _ptr(sa.in_proj_weight), _ptr(sa.in_proj_bias), None, 0, q, d, 0,
                                                   _ptr(cache), cap * 2 * d, 2 * d, d, B, 3 * d, d, _ACT_NONE, st)))
            calls.append((lib.ttts_decode_attention, (q, d, _ptr(cache), _ptr(cache, d), 2 * d, cap * 2 * d, None, ctx, d, ws,
                                                      sh.ws_bytes, B, H, hd, cap, st)))
            calls.append(linear(ctx, d, sa.out_proj.weight, sa.out_proj.bias, tmp, d, res=h))
            calls.append((lib.ttts_decode_layernorm, (tmp, _ptr(l.norm1.weight), _ptr(l.norm1.bias), h, B, d, l.norm1.eps, st)))
            calls.append(linear(h, d, ca.in_proj_weight, ca.in_proj_bias, q, d))          # rows 0 .. d - 1: the q projection
            calls.append((lib.ttts_decode_attention, (q, d, _ptr(mkv), _ptr(mkv, d), 2 * d, sh.Tp_pad * 2 * d, _ptr(sh.lens), ctx,
                                                      d, ws, sh.ws_bytes, B, H, hd, sh.Tp_pad, st)))
            calls.append(linear(ctx, d, ca.out_proj.weight, ca.out_proj.bias, tmp, d, res=h))
            calls.append((lib.ttts_decode_layernorm, (tmp, _ptr(l.norm2.weight), _ptr(l.norm2.bias), h, B, d, l.norm2.eps, st)))
            calls.append(linear(h, d, l.linear1.weight, l.linear1.bias, ffn, d_ffn, act=_ACT_RELU))
            calls.append(linear(ffn, d_ffn, l.linear2.weight, l.linear2.bias, tmp, d, res=h))
            calls.append((lib.ttts_decode_layernorm, (tmp, _ptr(l.norm3.weight), _ptr(l.norm3.bias), h, B, d, l.norm3.eps, st)))
        hm, hs = m.linear1.linear, m.linear2.linear
        calls.append((lib.ttts_decode_frame_out, (h, _ptr(hm.weight), _ptr(hm.bias), _ptr(hs.weight), _ptr(hs.bias), _ptr(sh.ys),
                                                  cap * nm, _ptr(sh.stop), cap, B, d, nm, st)))
        return calls

    def _run_chunk(self, sh: _Shape, stream: c_void_p):
        for _ in range(self._chunk):
            for fn, args in sh.calls:
                _lib.check(fn(*args, stream), fn.__name__)

    def _read_state(self, sh: _Shape):
        v = sh.state.cpu()             # one small device-to-host read on the side stream (synchronising)
        return int(v[0]), int(v[2])

    # ------------------------------------------------------------------------------------------------------ the call
    @torch.no_grad()
    def __call__(self, phoneme: torch.Tensor, phoneme_lens: torch.Tensor, max_len: int = 1500,
                 stop_threshold: float = 0.5) -> dict:
        self._check_call(phoneme, phoneme_lens, max_len)
        max_len = int(max_len)
        m = self.model
        m.eval()
        self._follow_weights()
        B, Tp = phoneme.shape
        dev = phoneme.device
        d = m.emb.weight.shape[1]
        layers = list(m.decoder.layers)
        # once per call, eagerly on the ops path: the encoder (no padding mask, as inference()) and the memory K/V per layer
        full = torch.full((B,), Tp, dtype=torch.int64, device=dev)
        memory = m.encode(phoneme, full)
        sh = self._shape(B, Tp, max_len, dev)
        for l, buf in zip(layers, sh.memkv):
            ca = l.multihead_attn
            kv = ops.linear(memory, ops.param_rows(ca.in_proj_weight, d, 3 * d), ops.param_rows(ca.in_proj_bias, d, 3 * d))
            buf[:, :Tp].copy_(kv)
        sh.lens.copy_(phoneme_lens.to(torch.int64))
        host = torch.tensor([1, max_len, -1, 0], dtype=torch.int64)
        host.view(torch.float32)[6] = float(stop_threshold)
        sh.state.copy_(host)
        if sh.calls is None:
            sh.calls = self._frame_calls(sh)
        if self._side is None or self._side.device != dev:
            self._side = torch.cuda.Stream(device=dev)
        side = self._side
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            stream = c_void_p(side.cuda_stream)
            if sh.graph is None:
                self._run_chunk(sh, stream)                  # the shape's first frames run eagerly ...
                g = torch.cuda.CUDAGraph()
                g.capture_begin(capture_error_mode=_CAPTURE_MODE)
                try:
                    self._run_chunk(sh, stream)              # ... then the same launches are captured (not run)
                finally:
                    g.capture_end()
                sh.graph = g
                self.captures += 1
            t, stop_frame = self._read_state(sh)
            while stop_frame < 0 and t < max_len:
                sh.graph.replay()
                t, stop_frame = self._read_state(sh)
        torch.cuda.current_stream(dev).wait_stream(side)
        n = stop_frame if stop_frame >= 0 else max_len - 1
        pred = sh.ys[:, 1:n + 1].clone()
        stops = sh.stop[:, :n].clone().unsqueeze(-1)
        post = ops.AddFn.apply(m.postnet(pred), pred)
        return {'pred_melspec': pred, 'post_melspec': post, 'pred_stop': stops}


def _check_structure(model):
    """what the decode kernels take: post-norm decoder layers, no final decoder norm, heads a multiple of 16 columns up to 128"""
    dec = model.decoder
    layers = list(dec.layers)
    if not layers:
        raise ValueError("Synthesizer: `model` has no decoder layers")
    if dec.norm is not None:
        raise ValueError("Synthesizer: `model` has a final decoder `norm`; the decode kernels run the reference's decoder "
                         "(no final norm)")
    if any(l.norm_first for l in layers):
        raise ValueError("Synthesizer: `model` has norm_first decoder layers; the decode kernels run post-norm layers only")
    d = model.emb.weight.shape[1]
    H = layers[0].self_attn.num_heads
    if d % H != 0 or (d // H) % 16 != 0 or d // H > 128:
        raise ValueError(f"Synthesizer: `model` head_dim = d_model / n_head = {d} / {H} is not a multiple of 16 up to 128")
    d_ffn = layers[0].linear1.weight.shape[0]
    if d > 1024 or d_ffn > 4096 or d_ffn % 4 != 0 or model.n_mels % 4 != 0:
        raise ValueError(f"Synthesizer: `model` sizes outside the decode kernels' range (d_model {d} <= 1024, d_ffn {d_ffn} <= "
                         f"4096 and n_mels {model.n_mels} multiples of 4)")
