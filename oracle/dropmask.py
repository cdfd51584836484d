"""CPU restatement of the counter-based dropout RNG of the HIP kernels (test infrastructure).

Written from the comments and formulas of `transformertts_amd/csrc/ttts_common.h` (`drop_threshold`, `attn_quad_hash`,
`attn_drop_mult`, `attn_keep`, `elem_quad_hash`, `keep_elem`, `site_seed`): the keep decision of a dropout site is a pure
function of (64-bit site seed, element index) in 32-bit integer arithmetic, so it can be restated exactly on the host and the
fp64 oracle can be given the very masks the kernels drew (`oracle.ref_model.drop_masks`).  numpy only, no GPU.
tests/test_hip_dropout_parity.py pins it to the kernels element for element.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

_M32 = np.uint64(0xFFFFFFFF)
# the odd constant of element e = idx & 3 of a quad (attn_drop_mult)
_MULT = np.array([0x9E3779B1, 0xC2B2AE3D, 0x27D4EB2F, 0x165667B1], dtype=np.uint64)


def drop_threshold(p: float) -> int:
    """round(p * 65536) clamped to [0, 65535]; p is the float32 the C ABI receives.  An element is kept iff its 16-bit draw
    reaches the threshold, so p is honoured to 2^-17 ~ 7.6e-6 (half a step; the header says 1.5e-5, one step)."""
    t = float(np.float32(p)) * 65536.0 + 0.5
    return int(min(max(t, 0.0), 65535.0))


def drop_scale(p: float) -> float:
    """the float32 value `1.f / (1.f - p)` the kernels multiply kept elements by, as a double"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def site_seed(seed: int, step_word: Optional[int] = None) -> int:
    """effective seed of a site: the seed passed by value XOR the 64-bit word of the active step state (None: no state)"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed if step_word is None else seed ^ (int(step_word) & 0xFFFFFFFFFFFFFFFF)


def _quad_hash(seed: int, row: np.ndarray, key_quad: np.ndarray) -> np.ndarray:
    """attn_quad_hash on uint64 arrays that hold 32-bit values; every product is reduced mod 2^32"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    const = np.uint64((seed & 0xFFFFFFFF) ^ (((seed >> 32) * 0xC2B2AE3D) & 0xFFFFFFFF))
    x = ((row * np.uint64(0x9E3779B1)) & _M32) ^ ((((key_quad + np.uint64(0x632BE5AB)) & _M32) * np.uint64(0x85EBCA77)) & _M32) ^ const
    x = (x * np.uint64(0x7feb352d)) & _M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & _M32
    return x


def _keep_word(word: np.ndarray, elem: np.ndarray, thr: int) -> np.ndarray:
    """attn_keep_word: the top 16 bits of word * mult[e] reach thr  <=>  (word * mult[e]) mod 2^32 >= thr << 16"""
    return ((word * _MULT[elem]) & _M32) >= np.uint64(thr << 16)


def keep_flat(seed: int, n: int, p: float, start: int = 0) -> np.ndarray:
    """bool (n,): keep_elem(seed, idx, drop_threshold(p)) for idx in start .. start + n - 1 (the flat element index of the
    output as stored: row * N + col)"""
    idx = np.arange(start, start + n, dtype=np.uint64)
    word = _quad_hash(seed, (idx >> np.uint64(2)) & _M32, idx >> np.uint64(34))
    return _keep_word(word, (idx & np.uint64(3)).astype(np.int64), drop_threshold(p))


def keep_attn(seed: int, rows: int, Tk: int, p: float) -> np.ndarray:
    """bool (rows, Tk): attn_keep(seed, row, key, thr << 16) over the (B * H * Tq, Tk) weight matrix, row = (b * H + h) * Tq + q"""
    row = np.arange(rows, dtype=np.uint64)[:, None]
    key = np.arange(Tk, dtype=np.uint64)[None, :]
    word = _quad_hash(seed, row, key >> np.uint64(2))
    return _keep_word(word, np.broadcast_to((key & np.uint64(3)).astype(np.int64), word.shape), drop_threshold(p))
