"""The 17 forward-type GEMM entry points (Linear and Conv1d, forward and data gradient, in the fp32-MFMA, bf16x6, fp16x3,
image-operand, LDS-DMA and head-image-output forms; csrc/gemm.hip): every refusal of their shared host bodies, the route of a
Linear launch (`ops._linear_route`) as a table, and that `ops._linear_fwd` / `ops._linear_bwd_data` launch what the route names.
Host logic only, no GPU (every refusal happens before a launch; the launches of the recorder test go to a stand-in library)."""
import ctypes

import pytest

# ---------------------------------------------------------------------------------------------------------------- refusals
_FWD_EPI = ["act", "p", "seed", "step_seed"]
_LIN_FWD = ["x", "w", "bias", "residual", "y", "M", "N", "K"] + _FWD_EPI
_LIN_BWD = ["dy", "w", "residual", "dx", "M", "N", "K", "relu_out", "relu_scale"]
_CONV = ["B", "T", "cin", "cout", "taps"]
# entry (without ttts_) -> (form, kind, argument names in ABI order)
ENTRIES = {
    "linear_fwd": ("f32", "lin_fwd", _LIN_FWD + ["row_shift", "T", "stream"]),
    "linear_fwd_x6": ("x6", "lin_fwd", _LIN_FWD + ["row_shift", "T", "stream"]),
    "linear_fwd_h3": ("h3", "lin_fwd", _LIN_FWD + ["row_shift", "T", "x_amax", "y_amax_out", "stream"]),
    "linear_fwd_h3i": ("h3i", "lin_fwd", ["x", "x_row_inv", "w", "bias", "residual", "y", "M", "N", "K"] + _FWD_EPI +
                       ["y_amax_out", "stream"]),
    "linear_fwd_h3d": ("h3d", "lin_fwd", _LIN_FWD + ["x_amax", "y_amax_out", "stream"]),
    "linear_fwd_h3d_img": ("img", "lin_fwd", ["x", "w", "bias", "y", "y_row_inv", "M", "N", "K", "x_amax", "y_amax_out",
                                              "amax_section_cols", "stream"]),
    "linear_bwd_data": ("f32", "lin_bwd", _LIN_BWD + ["stream"]),
    "linear_bwd_data_x6": ("x6", "lin_bwd", _LIN_BWD + ["stream"]),
    "linear_bwd_data_h3": ("h3", "lin_bwd", _LIN_BWD + ["dy_amax", "dx_amax_out", "stream"]),
    "linear_bwd_data_h3i": ("h3i", "lin_bwd", ["dy", "dy_row_inv", "w", "residual", "dx", "M", "N", "K", "relu_out", "relu_scale",
                                               "dx_amax_out", "stream"]),
    "linear_bwd_data_h3d": ("h3d", "lin_bwd", _LIN_BWD + ["dy_amax", "dx_amax_out", "stream"]),
    "conv1d_fwd": ("f32", "conv_fwd", ["x", "w", "bias", "y"] + _CONV + ["stream"]),
    "conv1d_fwd_x6": ("x6", "conv_fwd", ["x", "w", "bias", "y"] + _CONV + ["stream"]),
    "conv1d_fwd_h3": ("h3", "conv_fwd", ["x", "w", "bias", "y"] + _CONV + ["x_amax", "bn_partials", "stream"]),
    "conv1d_bwd_data": ("f32", "conv_bwd", ["dy", "w", "dx"] + _CONV + ["stream"]),
    "conv1d_bwd_data_x6": ("x6", "conv_bwd", ["dy", "w", "dx"] + _CONV + ["stream"]),
    "conv1d_bwd_data_h3": ("h3", "conv_bwd", ["dy", "w", "dx"] + _CONV + ["dy_amax", "stream"]),
}
# what a form asks of (reduction depth, output width): the multiples, and whether the output pointer is alignment-checked
_DEPTH_MULT = {"f32": 16, "x6": 16, "h3": 4, "h3i": 32, "h3d": 32, "img": 32}
_WIDTH_MULT = {"f32": 1, "x6": 1, "h3": 4, "h3i": 4, "h3d": 4, "img": 64}
_CHECKS_OUTPUT = ("h3i", "h3d", "img")
# kind -> (activation operand, output, the dimension names of (depth, width))
_ROLES = {"lin_fwd": ("x", "y", "K", "N"), "lin_bwd": ("dy", "dx", "N", "K"),
          "conv_fwd": ("x", "y", "cin", "cout"), "conv_bwd": ("dy", "dx", "cout", "cin")}
_OPTIONAL = ("bias", "residual", "relu_out", "step_seed", "y_amax_out", "dx_amax_out", "bn_partials", "stream")


def test_the_header_and_the_bindings_declare_the_seventeen_entry_points():
    from transformertts_amd import _lib
    lib = _lib.load()
    assert lib.ttts_abi_version() >= 24
    assert len(ENTRIES) == 17
    for name, (_, _, order) in ENTRIES.items():
        assert len(_lib.SIGNATURES["ttts_" + name][1]) == len(order), name
        assert hasattr(lib, "ttts_" + name)


def test_gemm_entry_points_refuse_bad_arguments_with_a_message():
    """One refusal table over all 17 entries: rc == -1 and a message that holds `<entry>:` and the needle."""
    from transformertts_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096 + 16)
    a = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)          # a 16-byte aligned host address (never dereferenced)
    a4 = ctypes.c_void_p(a.value + 4)
    checked = 0

    for name, (form, kind, order) in ENTRIES.items():
        act_op, out, depth, width = _ROLES[kind]
        conv = kind.startswith("conv")
        defaults = {n: None for n in order}
        defaults.update({n: a for n in order if n not in _OPTIONAL and n not in
                         ("M", "N", "K", "T", "B", "cin", "cout", "taps", "act", "p", "seed", "row_shift", "relu_scale",
                          "amax_section_cols")})
        defaults.update(M=640, N=256, K=256, B=2, T=320, cin=256, cout=256, taps=5, act=0, p=0.0, seed=0, row_shift=0,
                        relu_scale=1.0, amax_section_cols=0)
        if kind == "lin_fwd" and "T" in order:
            defaults["T"] = 0
        defaults = {n: v for n, v in defaults.items() if n in order}

        def call(**kw):
            unknown = set(kw) - set(order)
            assert not unknown, (name, unknown)
            return getattr(lib, "ttts_" + name)(*[kw.get(n, defaults[n]) for n in order])

        def bad(needle, *holds, **kw):
            nonlocal checked
            rc = call(**kw)
            msg = _lib.last_error()
            assert rc == -1, (name, kw, rc)
            assert name + ":" in msg and needle in msg, (name, kw, msg)
            for h in holds:
                assert h in msg, (name, kw, msg)
            checked += 1

        required = [n for n in order if defaults[n] is a]
        assert {act_op, "w", out} <= set(required), (name, required)
        if form in ("h3", "h3d", "img"):
            assert (act_op + "_amax") in required, name      # the activation's partial maxima
        if form == "h3i":
            assert (act_op + "_row_inv") in required, name
        for ptr in required:
            bad("null pointer", **{ptr: None})
        dims = _CONV if conv else ["M", "N", "K"]
        for d in dims:
            bad("bad dims", **{d: 0})
            bad("bad dims", **{d: -3})
        if conv:
            bad("bad dims", taps=4)                          # same-padded: an odd number of taps
        else:
            bad("bad dims", M=1 << 31)
        dm, wm = _DEPTH_MULT[form], _WIDTH_MULT[form]
        bad("multiple", f"{depth}={256 + 1}", **{depth: 256 + 1})
        bad("multiple", f"{depth}={256 - 1}", **{depth: 256 - 1})
        if dm > 4:
            bad("multiple", f"{depth}={256 + 4}", **{depth: 256 + 4})
        if wm > 1:
            bad("multiple", f"{width}={256 + 1}", **{width: 256 + 1})
            bad("multiple", f"{width}={256 - 1}", **{width: 256 - 1})
        if wm == 64:
            bad("multiple", f"{width}={256 + 32}", **{width: 256 + 32})
        if name == "linear_bwd_data":                        # (the fp32 data gradient also needs K % 4)
            bad("multiple", "K=258", K=258)
        bad("16-byte aligned", **{act_op: a4})
        bad("16-byte aligned", w=a4)
        if form in _CHECKS_OUTPUT:
            bad("16-byte aligned", **{out: a4})
        if conv:
            bad("4 GiB", B=1, T=1 << 26, **{depth: 16})
            bad("4 GiB", B=1 << 13, T=1 << 13, **{depth: 16})
        else:
            bad("4 GiB", M=1 << 20, **{depth: 1024})
            bad("4 GiB", M=16, N=32768, K=32768)             # the weight
        if "act" in order:
            bad("act must be 0 (none) or 1 (relu)", act=2)
            bad("act must be 0 (none) or 1 (relu)", act=-1)
        if "p" in order:
            bad("dropout p", p=1.0)
            bad("dropout p", p=-0.25)
        if "row_shift" in order:
            bad("row_shift needs T>0", row_shift=1, T=0)
            bad("row_shift needs T>0", row_shift=1, T=7)      # 640 rows are no whole number of 7-row utterances
        if form == "img":
            bad("amax sections", amax_section_cols=96)
            bad("amax sections", amax_section_cols=-64)
            bad("amax sections", N=320, amax_section_cols=128)     # whole heads that do not divide N
        if "bn_partials" in order:
            bad("bn_partials", "16-byte aligned", bn_partials=a4)
    assert checked > 17 * 15
    with pytest.raises(RuntimeError, match="ttts_conv1d_fwd_x6 failed"):
        _lib.check(lib.ttts_conv1d_fwd_x6(None, None, None, None, 1, 1, 16, 16, 1, None), "ttts_conv1d_fwd_x6")


# ------------------------------------------------------------------------------------------------------------------ routes
# Which kernel family a Linear launch takes, written out from the two ladders of ops._linear_fwd / ops._linear_bwd_data as they
# stood before one function (ops._linear_route) made the decision.  Families: x bf16x6 (the shape fallback), i image operand,
# d LDS-DMA, h gemm_h3.  A pattern holds one letter per (rows, depth, width) of the recorder's grid (tools/gemm_route_ab.py):
# five groups (rows 4096, 8192, 13920, 41760, 65536) of five depths (80, 250, 256, 512, 1024) x six widths (80, 81, 256, 512,
# 1024, 2048), width fastest.
_PATTERNS = {
    # gemm_h3 wherever the shape is a multiple of 4
    "plain": "hxhhhhxxxxxxhxhhhhhxhhhhhxhhhh hxhhhhxxxxxxhxhhhhhxhhhhhxhhhh hxhhhhxxxxxxhxhhhhhxhhhhhxhhhh "
             "hxhhhhxxxxxxhxhhhhhxhhhhhxhhhh hxhhhhxxxxxxhxhhhhhxhhhhhxhhhh",
    # no gate: depth <= 256 -> width >= 1024 when 256 tiles of 256 x 256 exist, the square projections from DMA_MIN_TILES tiles on
    "dma":   "hxhhhhxxxxxxhxhhhhhxhhhhhxhhhh hxhhhhxxxxxxhxhhhdhxhhhhhxhhhh hxhhhhxxxxxxhxhhhdhxhhhhhxhhhh "
             "hxhhhhxxxxxxhxdhddhxhdhhhxhhhh hxhhhhxxxxxxhxdhddhxhdhhhxhhhh",
    "image": "ixiiiixxxxxxixiiiiixiiiiixiiii ixiiiixxxxxxixiiiiixiiiiixiiii ixiiiixxxxxxixiiiiixiiiiixiiii "
             "ixiiiixxxxxxixiiiiixiiiiixiiii ixiiiixxxxxxixiiiiixiiiiixiiii",
    # a ready weight image: gemm_h3 on it, whatever its shape
    "ready": "hhhhhhhhhhhhhhhhhhhhhhhhhhhhhh hhhhhhhhhhhhhhhhhhhhhhhhhhhhhh hhhhhhhhhhhhhhhhhhhhhhhhhhhhhh "
             "hhhhhhhhhhhhhhhhhhhhhhhhhhhhhh hhhhhhhhhhhhhhhhhhhhhhhhhhhhhh",
    # a relu gate: 256 -> 512+ from 8192 rows on
    "gated": "hxhhhhxxxxxxhxhhhhhxhhhhhxhhhh hxhhhhxxxxxxhxhdddhxhhhhhxhhhh hxhhhhxxxxxxhxhdddhxhhhhhxhhhh "
             "hxhhhhxxxxxxhxddddhxhdhhhxhhhh hxhhhhxxxxxxhxddddhxhdhhhxhhhh",
    # the data gradient takes an operand image only on `_image_shape_ok` shapes
    "imgok": "hxhhhhxxxxxxhxhhhhhxhhhhhxhhhh hxhhhhxxxxxxhxiiiihxiiiihxiiii hxhhhhxxxxxxhxiiiihxiiiihxiiii "
             "hxhhhhxxxxxxhxiiiihxiiiihxiiii hxhhhhxxxxxxhxiiiihxiiiihxiiii",
    # DMA_BIG_FWD off: only the square projections are left
    "small": "hxhhhhxxxxxxhxhhhhhxhhhhhxhhhh hxhhhhxxxxxxhxhhhhhxhhhhhxhhhh hxhhhhxxxxxxhxhhhhhxhhhhhxhhhh "
             "hxhhhhxxxxxxhxdhhhhxhdhhhxhhhh hxhhhhxxxxxxhxdhhhhxhdhhhxhhhh",
}
_FLAG_SETTINGS = ({}, {"DMA_GEMMS": False}, {"DMA_BIG_FWD": False}, {"LAYERNORM_IMAGES": True})
_LINEAR_ROUTES = [
    # direction, operand image, tiles, then forward: shift / data gradient: gate, skip, w_image;
    #                                         defaults  DMA_GEMMS off  DMA_BIG_FWD off  LAYERNORM_IMAGES on
    ("fwd", 0, 0, 0,                          "plain",  "plain",       "plain",         "plain"),
    ("fwd", 0, 0, 1,                          "plain",  "plain",       "plain",         "plain"),
    ("fwd", 0, 1, 0,                          "dma",    "plain",       "small",         "dma"),
    ("fwd", 0, 1, 1,                          "plain",  "plain",       "plain",         "plain"),    # (a row shift drops `tiles`)
    ("fwd", 1, 0, 0,                          "plain",  "plain",       "plain",         "plain"),
    ("fwd", 1, 0, 1,                          "plain",  "plain",       "plain",         "plain"),
    ("fwd", 1, 1, 0,                          "image",  "image",       "image",         "image"),    # (the forward trusts its caller)
    ("fwd", 1, 1, 1,                          "plain",  "plain",       "plain",         "plain"),
    ("bwd", 0, 0, 0, 0, 0,                    "plain",  "plain",       "plain",         "plain"),
    ("bwd", 0, 0, 0, 0, 1,                    "ready",  "ready",       "ready",         "ready"),
    ("bwd", 0, 0, 0, 1, 0,                    "plain",  "plain",       "plain",         "plain"),
    ("bwd", 0, 0, 0, 1, 1,                    "ready",  "ready",       "ready",         "ready"),
    ("bwd", 0, 0, 1, 0, 0,                    "plain",  "plain",       "plain",         "plain"),
    ("bwd", 0, 0, 1, 0, 1,                    "ready",  "ready",       "ready",         "ready"),
    ("bwd", 0, 0, 1, 1, 0,                    "plain",  "plain",       "plain",         "plain"),
    ("bwd", 0, 0, 1, 1, 1,                    "ready",  "ready",       "ready",         "ready"),
    ("bwd", 0, 1, 0, 0, 0,                    "dma",    "plain",       "small",         "dma"),
    ("bwd", 0, 1, 0, 0, 1,                    "ready",  "ready",       "ready",         "ready"),
    ("bwd", 0, 1, 0, 1, 0,                    "dma",    "plain",       "small",         "dma"),
    ("bwd", 0, 1, 0, 1, 1,                    "ready",  "ready",       "ready",         "ready"),
    ("bwd", 0, 1, 1, 0, 0,                    "gated",  "plain",       "gated",         "gated"),
    ("bwd", 0, 1, 1, 0, 1,                    "ready",  "ready",       "ready",         "ready"),
    ("bwd", 0, 1, 1, 1, 0,                    "plain",  "plain",       "plain",         "plain"),    # (gate plus skip: never DMA)
    ("bwd", 0, 1, 1, 1, 1,                    "ready",  "ready",       "ready",         "ready"),
    ("bwd", 1, 0, 0, 0, 0,                    "plain",  "plain",       "plain",         "plain"),
    ("bwd", 1, 0, 0, 0, 1,                    "ready",  "ready",       "ready",         "ready"),
    ("bwd", 1, 0, 0, 1, 0,                    "plain",  "plain",       "plain",         "plain"),
    ("bwd", 1, 0, 0, 1, 1,                    "ready",  "ready",       "ready",         "ready"),
    ("bwd", 1, 0, 1, 0, 0,                    "plain",  "plain",       "plain",         "plain"),
    ("bwd", 1, 0, 1, 0, 1,                    "ready",  "ready",       "ready",         "ready"),
    ("bwd", 1, 0, 1, 1, 0,                    "plain",  "plain",       "plain",         "plain"),
    ("bwd", 1, 0, 1, 1, 1,                    "ready",  "ready",       "ready",         "ready"),
    ("bwd", 1, 1, 0, 0, 0,                    "imgok",  "imgok",       "imgok",         "imgok"),
    ("bwd", 1, 1, 0, 0, 1,                    "ready",  "ready",       "ready",         "ready"),
    ("bwd", 1, 1, 0, 1, 0,                    "imgok",  "imgok",       "imgok",         "imgok"),
    ("bwd", 1, 1, 0, 1, 1,                    "ready",  "ready",       "ready",         "ready"),
    ("bwd", 1, 1, 1, 0, 0,                    "imgok",  "imgok",       "imgok",         "imgok"),
    ("bwd", 1, 1, 1, 0, 1,                    "ready",  "ready",       "ready",         "ready"),
    ("bwd", 1, 1, 1, 1, 0,                    "imgok",  "imgok",       "imgok",         "imgok"),
    ("bwd", 1, 1, 1, 1, 1,                    "ready",  "ready",       "ready",         "ready"),
]


def _recorder_tool():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "gemm_route_ab.py")
    spec = importlib.util.spec_from_file_location("gemm_route_ab", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _route(ops, direction, M, red, out, kw):
    if direction == "fwd":
        return ops._linear_route(True, M, red, out, operand_image=kw["image"], shifted=kw["shift"] != 0, tiles=kw["tiles"])
    return ops._linear_route(False, M, red, out, operand_image=kw["image"], gate=kw["gate"], skip=kw["skip"], tiles=kw["tiles"],
                             w_image=kw["w_image"])


def _table_rows():
    for row in _LINEAR_ROUTES:
        direction = row[0]
        if direction == "fwd":
            kw = dict(image=bool(row[1]), tiles=bool(row[2]), shift=row[3])
            yield direction, kw, row[4:]
        else:
            kw = dict(image=bool(row[1]), tiles=bool(row[2]), gate=bool(row[3]), skip=bool(row[4]), w_image=bool(row[5]))
            yield direction, kw, row[6:]


def test_the_route_of_a_linear_launch(monkeypatch):
    from transformertts_amd import ops
    tool = _recorder_tool()
    assert (ops.DMA_GEMMS, ops.DMA_BIG_FWD, ops.LAYERNORM_IMAGES, ops.IMAGE_MIN_ROWS, ops.DMA_MIN_TILES) == (True, True, False, 8192, 320)
    assert tool.FLAGS == _FLAG_SETTINGS
    assert len({row[:4 if row[0] == "fwd" else 6] for row in _LINEAR_ROUTES}) == len(_LINEAR_ROUTES) == 8 + 32
    shapes = list(tool.shapes())
    families = {v: k for k, v in tool.FAMILY.items()}
    for col, flags in enumerate(_FLAG_SETTINGS):
        with monkeypatch.context() as mp:
            for k, v in flags.items():
                mp.setattr(ops, k, v)
            for direction, kw, expected in _table_rows():
                letters = _PATTERNS[expected[col]].replace(" ", "")
                for (M, red, out), letter in zip(shapes, letters, strict=True):
                    kind, mode, sibling = _route(ops, direction, M, red, out, kw)
                    assert kind == families[letter], (flags, direction, kw, M, red, out)
                    base = 0 if direction == "fwd" else 1
                    want = {"x": ops.X6_LIN_FWD, "i": ops.H3D_LIN_FWD, "d": ops.H3D_LIN_FWD, "h": ops.H3_LIN_FWD}[letter] + base
                    assert mode == (None if kw.get("w_image") else want)
                    # a sibling image only where a row count on the other side of a threshold would take the other kernel
                    assert sibling in (None, {ops.H3D_LIN_FWD + base: ops.H3_LIN_FWD + base,
                                              ops.H3_LIN_FWD + base: ops.H3D_LIN_FWD + base}.get(mode))
                    if letter == "i":
                        assert sibling is not None
                    if letter == "x" or not kw["tiles"] or kw.get("shift") or kw.get("w_image"):
                        assert sibling is None
                    elif letter != "i":
                        assert (sibling is not None) == (ops._dma_dims(red, out) or ops._image_dims(red, out))


def test_linear_launches_are_what_the_route_names(monkeypatch):
    """`_linear_fwd` / `_linear_bwd_data` on a stand-in library: exactly the entry point of the route's family, exactly the
    `_planes` modes it names -- the sibling first, and none inside a capture --, the operand's maxima measured only for the
    families that take them."""
    import torch as _torch
    from transformertts_amd import _lib, ops
    tool = _recorder_tool()
    patterns = set()
    for capturing in (False, True):
        for flags in _FLAG_SETTINGS:
            with monkeypatch.context() as mp:
                rec = tool.Recorder(ops, _torch, _lib)
                rec.install(mp.setattr, capturing)
                for k, v in flags.items():
                    mp.setattr(ops, k, v)
                for direction, _, kw in tool.combos():
                    entry = "linear_fwd_" if direction == "fwd" else "linear_bwd_data_"
                    dims = "NxK" if direction == "fwd" else "KxN"
                    for M, red, out in tool.shapes():
                        kind, mode, sibling = _route(ops, direction, M, red, out, kw)
                        want = ["amax"] if kind in ("h3", "h3d") else []
                        if sibling is not None and not capturing:
                            want.append(f"planes {sibling} {dims}")
                        if mode is not None:
                            want.append(f"planes {mode} {dims}")
                        want.append(entry + kind)
                        got = tool.launch(rec, direction, M, red, out, kw)
                        assert got == ", ".join(want), (capturing, flags, direction, kw, M, red, out)
                        M_, N_, K_ = (M, out, red) if direction == "fwd" else (M, red, out)
                        assert (M_, N_, K_) in zip(rec.args, rec.args[1:], rec.args[2:]), rec.args
                        if not capturing:
                            patterns.add((direction, got))
    assert sum(d == "fwd" for d, _ in patterns) == 5 and sum(d == "bwd" for d, _ in patterns) == 6, sorted(patterns)
    assert ("fwd", "amax, planes 8 NxK, planes 4 NxK, linear_fwd_h3") in patterns       # the sibling image is made first
