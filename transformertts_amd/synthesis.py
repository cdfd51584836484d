"""Synthesizer: `TransformerTTS.inference` as replays of a captured HIP graph on the decode kernels of csrc/decode.hip.

    synth = Synthesizer(model)
    out = synth(phoneme, phoneme_lens, max_len=1500, stop_threshold=0.5)     # the dict model.inference(...) returns
    out = synth.synthesize(phoneme, phoneme_lens, max_len=1500, stop_threshold=0.5, alignments=False)   # each row at its own length

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

`synthesize` is the batched form a caller of a TTS engine wants: every utterance ends at ITS first frame at or above the
threshold (that frame is kept), the call ends when the last one has, and the dict carries `mel_lens` and exact zeros behind
each row's end.  The per-row end frames live in a device array right behind the decode state (one copy resets both), and the
kernels skip the rows that have ended.  A cached shape holds up to three chunk graphs over the same buffers, each captured the
first time it is needed: `__call__`'s (the entry points without per-row state: reading it costs every kernel a little, which
`__call__` does not pay), `synthesize`'s, and `synthesize(alignments=True)`'s, whose cross-attention kernels are the
map-writing variant; the map buffers are allocated with that capture.  Within a method, `max_len`, the threshold and where the
rows stop are data: they never cause a capture.

`synthesize(..., window=AttentionWindow(guide=(layer, head), back=1, ahead=3))` is the attention window that attention-TTS
engines decode with: every utterance keeps a position, the phoneme the guide head attended at the previous frame, and the
constrained heads' cross-attention sees only `back` phonemes behind and `ahead` phonemes ahead of it.  The positions live in a
(B, cap) device array the guide head's kernel writes one entry of per frame, and the window, the guide and the selection of
heads are a 32-byte struct per layer that the call copies next to the state reset: they are data too, so one more chunk graph
per shape (and one for the map-writing kernels) serves every `AttentionWindow`.
"""
from __future__ import annotations

import numbers
from collections import OrderedDict
from ctypes import c_void_p
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import torch

from . import _lib, ops

_CAPTURE_MODE = "thread_local"      # as step.py: illegal-during-capture checks confined to the capturing thread
_TP_ROUND = 64
_CAP_ROUND = 256
_ACT_NONE, _ACT_RELU = 0, 1
_PER_ROW = 1                        # TTTS_DECODE_PER_ROW


_WINDOW_MODES = ("win", "winmaps")
_I32_MAX = 2 ** 31 - 1


@dataclass(frozen=True)
class AttentionWindow:
    """The attention window of `Synthesizer.synthesize(window=...)`.  `guide`: the (decoder layer, head) whose largest
    in-window score at a frame becomes the utterance's position for the next frame.  A constrained head sees the keys
    max(0, position - back) .. min(phoneme_len - 1, position + ahead), both inclusive; `layers` / `heads` select the constrained
    ones as `GuidedAttentionLoss(layers=..., heads=...)` does (None = all, else the indices), and the guide must be among them."""
    guide: Tuple[int, int]
    back: int = 1
    ahead: int = 3
    layers: Optional[Sequence[int]] = None
    heads: Optional[Sequence[int]] = None


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
        # ttts_decode_state (32 bytes), then row_end (B entries, allocated up to a multiple of 4 as the kernels read it)
        self.state = torch.zeros(4 + _up(B, 4), dtype=torch.int64, device=dev)
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
        self.win = torch.zeros(4 * len(layers), dtype=torch.int64, device=dev)     # one ttts_decode_window (32 bytes) per layer
        self.pos = torch.zeros(B, cap, dtype=torch.int32, device=dev)        # attention-window positions, entry t - 1 per frame t
        self.maps = None                                                     # per layer (B, H, cap, Tp_pad), once asked for
        self._map_shape = (B, H, cap, Tp_pad)
        self.drop_graphs()

    def drop_graphs(self):
        self.calls = {}                               # keyed by the mode of Synthesizer._frame_calls
        self.graph = {}

    def alloc_maps(self, n_layers: int):
        if self.maps is None:
            self.maps = [torch.zeros(*self._map_shape, dtype=torch.float32, device=self.state.device) for _ in range(n_layers)]

    def nbytes(self) -> int:
        ts = [self.state, self.ys, self.stop, self.h, self.tmp, self.q, self.ctx, self.ffn, self.lens, self.ws, self.win, self.pos]
        return sum(t.numel() * t.element_size() for t in ts + self.cache + self.memkv + (self.maps or []))


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
        self.captures = 0            # chunk graphs captured so far (per shape: the first __call__, the first synthesize, the
        #                              first synthesize with alignments, the first with a window, the first with a window and
        #                              alignments; and again after its weights moved)
        self.recaptures = 0          # times moved parameter storage dropped the captured graphs

    @property
    def chunk(self) -> int:
        """frames per captured graph (one replay, then one device-to-host read of the decode state)"""
        return self._chunk

    def shape_bytes(self) -> dict:
        """static-buffer footprint of every cached shape (alignment maps included once allocated), {(B, Tp_pad, cap): bytes}"""
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

    def _check_window(self, window):
        """-> per decoder layer (back, ahead, guide head or -1, head mask), or raises: host logic only"""
        if not isinstance(window, AttentionWindow):
            raise ValueError(f"Synthesizer: `window` must be an AttentionWindow or None, got {type(window).__name__}")
        layers = list(self.model.decoder.layers)
        if layers and layers[0].self_attn.num_heads > 64:        # (the head mask of ttts_decode_window holds 64)
            raise ValueError(f"Synthesizer: an attention window takes at most 64 decoder heads, the model has "
                             f"{layers[0].self_attn.num_heads}")
        _check_structure(self.model)
        n_layers, H = len(layers), layers[0].self_attn.num_heads

        def integer(x):
            return isinstance(x, numbers.Integral) and not isinstance(x, bool)

        for name, v in (("back", window.back), ("ahead", window.ahead)):
            if not integer(v) or v < 0:
                raise ValueError(f"Synthesizer: `window.{name}` must be a non-negative integer, got {v!r}")
        sel = {}
        for name, v, n in (("layers", window.layers, n_layers), ("heads", window.heads, H)):
            if v is None:
                sel[name] = list(range(n))
                continue
            if isinstance(v, (str, bytes)) or not hasattr(v, "__iter__"):
                raise ValueError(f"Synthesizer: `window.{name}` must be None or a sequence of indices, got {v!r}")
            idx = list(v)
            if not all(integer(i) for i in idx):
                raise ValueError(f"Synthesizer: `window.{name}` must hold integers, got {idx!r}")
            idx = [int(i) for i in idx]
            if len(set(idx)) != len(idx):
                raise ValueError(f"Synthesizer: `window.{name}` holds an index twice: {idx!r}")
            if any(i < 0 or i >= n for i in idx):
                raise ValueError(f"Synthesizer: `window.{name}` = {idx!r} out of range (the decoder has {n})")
            sel[name] = sorted(idx)
        g = window.guide
        if isinstance(g, (str, bytes)) or not hasattr(g, "__len__") or len(g) != 2 or not all(integer(i) for i in g):
            raise ValueError(f"Synthesizer: `window.guide` must be a (decoder layer, head) pair of integers, got {g!r}")
        gl, gh = int(g[0]), int(g[1])
        if not (0 <= gl < n_layers and 0 <= gh < H):
            raise ValueError(f"Synthesizer: `window.guide` = ({gl}, {gh}) is outside the model ({n_layers} decoder layers of {H} "
                             f"heads)")
        if gl not in sel["layers"] or gh not in sel["heads"]:
            raise ValueError(f"Synthesizer: `window.guide` = ({gl}, {gh}) is not among the constrained (layer, head)s "
                             f"(layers {sel['layers']}, heads {sel['heads']})")
        mask = sum(1 << h for h in sel["heads"])
        back, ahead = min(int(window.back), _I32_MAX), min(int(window.ahead), _I32_MAX)
        return [(back, ahead, gh if i == gl else -1, mask if i in sel["layers"] else 0) for i in range(n_layers)]

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
                s.drop_graphs()
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

    def _frame_calls(self, sh: _Shape, mode: str):
        """the launch sequence of one frame: [(entry point, arguments without the stream)].  `mode` "call": the entry points
        without per-row state (no row ever ends); "rows": the *_rows entry points on the shape's row_end; "maps": those, with
        cross-attention also writing row t - 1 of every layer's alignment map; "win" / "winmaps": as "rows" / "maps" with the
        cross-attention of every layer on ttts_decode_attention_window (which heads of which layers it constrains is data)"""
        lib = _lib.load()
        m = self.model
        layers = list(m.decoder.layers)
        B, cap, nm = sh.B, sh.cap, m.n_mels
        d = m.emb.weight.shape[1]
        H = layers[0].self_attn.num_heads
        hd = d // H
        d_ffn = layers[0].linear1.weight.shape[0]
        st = _ptr(sh.state)
        rows = mode != "call"
        re = (_ptr(sh.state, 8),) if rows else ()    # row_end: behind the 32 bytes of the state
        f_in, f_lin, f_ln, f_att, f_out = ((lib.ttts_decode_frame_in_rows, lib.ttts_decode_linear_rows,
                                            lib.ttts_decode_layernorm_rows, lib.ttts_decode_attention_rows,
                                            lib.ttts_decode_frame_out_rows) if rows else
                                           (lib.ttts_decode_frame_in, lib.ttts_decode_linear, lib.ttts_decode_layernorm,
                                            lib.ttts_decode_attention, lib.ttts_decode_frame_out))
        h, tmp, q, ctx, ffn, ws = _ptr(sh.h), _ptr(sh.tmp), _ptr(sh.q), _ptr(sh.ctx), _ptr(sh.ffn), _ptr(sh.ws)
        p1, p2 = m.dec_prenet.linear1.linear, m.dec_prenet.linear2.linear
        calls = [(f_in, (_ptr(sh.ys), cap * nm, nm, _ptr(p1.weight), _ptr(p1.bias), _ptr(p2.weight), _ptr(p2.bias), _ptr(m.pe.pe),
                         _ptr(m.pe.alpha), tmp, h, B, d, *re, st))]

        def linear(x, K, w, b, y, N, res=None, act=_ACT_NONE):
            return (f_lin, (x, K, 0, _ptr(w), _ptr(b), res, d if res is not None else 0, y, N, 0, None, 0, 0, N, B, N, K, act,
                            *re, st))

        def norm(n):
            return (f_ln, (tmp, _ptr(n.weight), _ptr(n.bias), h, B, d, n.eps, *re, st))

        for i, (l, cache, mkv) in enumerate(zip(layers, sh.cache, sh.memkv)):
            sa, ca = l.self_attn, l.multihead_attn
            no_map = (*re, None, 0, 0, 0) if rows else ()
            amap = (*re, _ptr(sh.maps[i]), cap * sh.Tp_pad, sh.Tp_pad, cap) if mode in ("maps", "winmaps") else no_map
            f_cross, win = f_att, ()
            if mode in _WINDOW_MODES:
                f_cross, win = lib.ttts_decode_attention_window, (c_void_p(sh.win.data_ptr() + 32 * i), c_void_p(sh.pos.data_ptr()), cap)
            # in-projection: q to `q`, the K/V columns straight into row t - 1 of this layer's cache
            calls.append((f_lin, (h, d, 0, _ptr(sa.in_proj_weight), _ptr(sa.in_proj_bias), None, 0, q, d, 0, _ptr(cache),
                                  cap * 2 * d, 2 * d, d, B, 3 * d, d, _ACT_NONE, *re, st)))
            calls.append((f_att, (q, d, _ptr(cache), _ptr(cache, d), 2 * d, cap * 2 * d, None, ctx, d, ws, sh.ws_bytes, B, H, hd,
                                  cap, *no_map, st)))
            calls.append(linear(ctx, d, sa.out_proj.weight, sa.out_proj.bias, tmp, d, res=h))
            calls.append(norm(l.norm1))
            calls.append(linear(h, d, ca.in_proj_weight, ca.in_proj_bias, q, d))          # rows 0 .. d - 1: the q projection
            calls.append((f_cross, (q, d, _ptr(mkv), _ptr(mkv, d), 2 * d, sh.Tp_pad * 2 * d, _ptr(sh.lens), ctx, d, ws, sh.ws_bytes,
                                    B, H, hd, sh.Tp_pad, *amap, *win, st)))
            calls.append(linear(ctx, d, ca.out_proj.weight, ca.out_proj.bias, tmp, d, res=h))
            calls.append(norm(l.norm2))
            calls.append(linear(h, d, l.linear1.weight, l.linear1.bias, ffn, d_ffn, act=_ACT_RELU))
            calls.append(linear(ffn, d_ffn, l.linear2.weight, l.linear2.bias, tmp, d, res=h))
            calls.append(norm(l.norm3))
        hm, hs = m.linear1.linear, m.linear2.linear
        calls.append((f_out, (h, _ptr(hm.weight), _ptr(hm.bias), _ptr(hs.weight), _ptr(hs.bias), _ptr(sh.ys), cap * nm,
                              _ptr(sh.stop), cap, B, d, nm, *re, st)))
        return calls

    def _run_chunk(self, calls, stream: c_void_p):
        for _ in range(self._chunk):
            for fn, args in calls:
                _lib.check(fn(*args, stream), fn.__name__)

    def _read_state(self, sh: _Shape):
        v = sh.state[:4].cpu()         # one 32-byte device-to-host read on the side stream (synchronising)
        return int(v[0]), int(v[2])

    # ------------------------------------------------------------------------------------------------------ the call
    def _decode(self, phoneme, phoneme_lens, max_len: int, stop_threshold: float, mode: str, window=None):
        """encoder, memory K/V, then the chunk graph of `mode` until the state says the decoding has ended: (shape, frames
        decoded).  `window`: the per-layer structs of _check_window for the window modes"""
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
        host = torch.full((sh.state.numel(),), -1, dtype=torch.int64)        # every row running
        host[0], host[1], host[3] = 1, max_len, 0
        host.view(torch.float32)[6] = float(stop_threshold)
        host.view(torch.int32)[7] = _PER_ROW if mode != "call" else 0
        sh.state.copy_(host)
        if window is not None:
            whost = torch.zeros(sh.win.numel(), dtype=torch.int64)          # ttts_decode_window per layer
            for i, (back, ahead, guide_head, mask) in enumerate(window):
                whost.view(torch.int32)[8 * i:8 * i + 3] = torch.tensor([back, ahead, guide_head], dtype=torch.int32)
                whost[4 * i + 2] = mask - (1 << 64) if mask >= 1 << 63 else mask
            sh.win.copy_(whost)
        if mode in ("maps", "winmaps"):
            sh.alloc_maps(len(layers))
        if sh.calls.get(mode) is None:
            sh.calls[mode] = self._frame_calls(sh, mode)
        calls = sh.calls[mode]
        if self._side is None or self._side.device != dev:
            self._side = torch.cuda.Stream(device=dev)
        side = self._side
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            stream = c_void_p(side.cuda_stream)
            if sh.graph.get(mode) is None:
                self._run_chunk(calls, stream)               # the shape's first frames run eagerly ...
                g = torch.cuda.CUDAGraph()
                g.capture_begin(capture_error_mode=_CAPTURE_MODE)
                try:
                    self._run_chunk(calls, stream)           # ... then the same launches are captured (not run)
                finally:
                    g.capture_end()
                sh.graph[mode] = g
                self.captures += 1
            t, stop_frame = self._read_state(sh)
            while stop_frame < 0 and t < max_len:
                sh.graph[mode].replay()
                t, stop_frame = self._read_state(sh)
        torch.cuda.current_stream(dev).wait_stream(side)
        return sh, (stop_frame if stop_frame >= 0 else max_len - 1)

    @torch.no_grad()
    def __call__(self, phoneme: torch.Tensor, phoneme_lens: torch.Tensor, max_len: int = 1500,
                 stop_threshold: float = 0.5) -> dict:
        self._check_call(phoneme, phoneme_lens, max_len)
        m = self.model
        sh, n = self._decode(phoneme, phoneme_lens, int(max_len), stop_threshold, "call")
        pred = sh.ys[:, 1:n + 1].clone()
        stops = sh.stop[:, :n].clone().unsqueeze(-1)
        post = ops.AddFn.apply(m.postnet(pred), pred)
        return {'pred_melspec': pred, 'post_melspec': post, 'pred_stop': stops}

    @torch.no_grad()
    def synthesize(self, phoneme: torch.Tensor, phoneme_lens: torch.Tensor, max_len: int = 1500, stop_threshold: float = 0.5,
                   alignments: bool = False, window: Optional[AttentionWindow] = None) -> dict:
        """Every utterance at its own length.  Row b ends at its first frame t (1-based) with sigmoid(stop[b, t - 1]) >=
        `stop_threshold` -- that frame is kept -- or at `max_len` - 1; the call ends when every row has.  Returns `pred_melspec`,
        `post_melspec` (B, T, n_mels), `pred_stop` (B, T, 1) with T = mel_lens.max(), `mel_lens` (B,) int64 on the device, and
        with `alignments=True` one (B, heads, T, Tp) cross-attention map per decoder layer.  Everything at frame >= mel_lens[b]
        of row b is exactly 0; a row's frames before its end are bit for bit those of `__call__` for that row, and its
        `post_melspec` is the post-net of its own frames (the rows behind each end are zeroed between the post-net's layers).

        `window`: None, or an `AttentionWindow`.  Utterance b then carries a position, 0 at the first frame; at every frame the
        constrained (layer, head)s take their cross-attention softmax over the keys max(0, position - back) ..
        min(phoneme_lens[b] - 1, position + ahead) only, and the guide's key with the largest score among those (the lowest
        one on equal scores) is the position every layer of the next frame uses.  Every other head, and self-attention, are
        what they are without a window.  The call also returns `attention_positions` (B, T) int64 on the device: entry [b, f] is
        the position after frame f + 1 (1-based), -1 at f >= mel_lens[b]; with `alignments=True` the maps of constrained heads
        are exactly 0 outside each frame's window and their rows sum to 1.  A guide is a (layer, head) whose map is diagonal:
        take `extract_durations(...)['choice']` (or what `teacher_durations(...)` chose) on a few utterances of the model."""
        if not isinstance(alignments, bool):
            raise ValueError(f"Synthesizer: `alignments` must be a bool, got {type(alignments).__name__}")
        structs = self._check_window(window) if window is not None else None
        self._check_call(phoneme, phoneme_lens, max_len)
        m = self.model
        max_len = int(max_len)
        if structs is None:
            mode = "maps" if alignments else "rows"
        else:
            mode = "winmaps" if alignments else "win"
        sh, n = self._decode(phoneme, phoneme_lens, max_len, stop_threshold, mode, structs)
        B, Tp = phoneme.shape
        row_end = sh.state[4:4 + B]
        mel_lens = torch.where(row_end > 0, row_end, torch.full_like(row_end, max_len - 1))
        pred = _mask_rows(sh.ys[:, 1:n + 1].clone(), mel_lens)
        stops = _mask_rows(sh.stop[:, :n].clone().unsqueeze(-1), mel_lens)
        x = pred
        for conv, act in _postnet_layers(m.postnet):
            x = _mask_rows(conv.fused(x, act, 0.0), mel_lens)          # (eval mode: the post-net's dropout is off)
        post = ops.AddFn.apply(x, pred)
        out = {'pred_melspec': pred, 'post_melspec': post, 'pred_stop': stops, 'mel_lens': mel_lens}
        if alignments:
            out['alignments'] = [_mask_rows(a[:, :, :n, :Tp].clone(), mel_lens) for a in sh.maps]
        if structs is not None:
            frames = torch.arange(n, device=mel_lens.device).unsqueeze(0)
            pos = sh.pos[:, :n].to(torch.int64)
            out['attention_positions'] = torch.where(frames < mel_lens.unsqueeze(1), pos, torch.full_like(pos, -1))
        return out


def _mask_rows(x: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
    """x (B, T, C) or (B, H, T, C), fresh and contiguous: rows t >= lens[b] := 0, in place"""
    if not (x.is_contiguous() and x.dtype == torch.float32):
        raise RuntimeError("Synthesizer: masking expects a contiguous fp32 tensor")
    group = x.shape[1] if x.dim() == 4 else 1
    lib = _lib.load()
    _lib.check(lib.ttts_mask_rows(_ptr(x), c_void_p(lens.data_ptr()), x.shape[0] * group, group, x.shape[-2], x.shape[-1],
                                  ops._stream()), "ttts_mask_rows")
    return x


def _postnet_layers(postnet):
    """[(ConvNormBN, activation)] in the order PostNet.forward runs them"""
    mods = list(postnet.layers)
    out = []
    for i, mod in enumerate(mods):
        if hasattr(mod, "fused"):
            tanh = i + 1 < len(mods) and isinstance(mods[i + 1], torch.nn.Tanh)
            out.append((mod, ops.ACT_TANH if tanh else ops.ACT_NONE))
    return out


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
