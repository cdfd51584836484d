"""The ten weight-gradient entry points (csrc/gemm.hip: the size query, the class query, three Linear forms, `parts`, the grouped
launch, three Conv1d forms): every refusal of their shared host body from one table, the two size queries as literal tables, and
what `ops._weight_grad` / `ReduceQueue.launch_wgrads` hand the library, recorded on a stand-in.
Host logic only, no GPU.  Pointers are aligned host addresses that are never dereferenced, so EVERY call of a launching entry in
this file is one the library refuses (an accepted one would launch a kernel on them where there is a GPU)."""
import ctypes
import hashlib
import itertools
import os
import re

import pytest

_LIN = ["dy", "x", "dw", "dbias", "ws", "ws_bytes", "M", "N", "K", "row_shift", "T", "accumulate"]
_CONV = ["dy", "x", "dw", "dbias", "ws", "ws_bytes", "B", "T", "cin", "cout", "taps", "accumulate"]
_TAIL = ["queue", "stream"]
_AMAX = ["dy_amax", "x_amax"]
# entry (without ttts_) -> (form, kind, argument names in ABI order)
ENTRIES = {
    "linear_bwd_weight": ("f32", "lin", _LIN + _TAIL),
    "linear_bwd_weight_x6": ("x6", "lin", _LIN + _TAIL),
    "linear_bwd_weight_h3": ("h3", "lin", _LIN + _AMAX + _TAIL),
    "linear_bwd_weight_h3_parts": ("h3", "parts", ["dy", "x", "dw_parts", "dbias_parts", "nparts", "ws", "ws_bytes", "M", "N", "K",
                                                   "accumulate"] + _AMAX + _TAIL),
    "wgrad_group": ("h3", "group", ["n", "dy", "x", "dw", "dbias", "ws", "ws_bytes", "M", "N", "K", "taps", "T", "row_shift",
                                    "accumulate"] + _AMAX + _TAIL),
    "conv1d_bwd_weight": ("f32", "conv", _CONV + _TAIL),
    "conv1d_bwd_weight_x6": ("x6", "conv", _CONV + _TAIL),
    "conv1d_bwd_weight_h3": ("h3", "conv", _CONV + _AMAX + _TAIL),
}
QUERIES = {"wgrad_workspace_bytes": 4, "wgrad_group_ok": 4}
_POINTERS = ("dy", "x", "dw", "dbias", "ws", "dw_parts", "dbias_parts", "dy_amax", "x_amax")
_OPTIONAL = ("dbias", "dbias_parts", "queue", "stream")
_BIG = 1 << 40                # a workspace size no check finds too small
_GROUP_MEMBER = ("dy", "x", "dw", "dbias", "ws", "ws_bytes", "M", "N", "K", "taps", "T", "row_shift", "dy_amax", "x_amax")
# the partial sums of the default group -- ONE member of 640 rows, 256 x 256: 20 k-tiles of 32 rows, at least 8 per split -> 3 row
# splits of (256 x 256 products + 256 column sums) floats
_GROUP_DEFAULT_NEED = 3 * (256 * 256 + 256) * 4


def test_the_header_and_the_bindings_declare_the_ten_entry_points():
    from transformertts_amd import _lib
    lib = _lib.load()
    assert lib.ttts_abi_version() == 24
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "ttts_hip.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    counts = {name: len(order) for name, (_, _, order) in ENTRIES.items()}
    counts.update(QUERIES)
    assert len(counts) == 10
    for name, n in counts.items():
        assert len(_lib.SIGNATURES["ttts_" + name][1]) == n, name
        assert hasattr(lib, "ttts_" + name)
        decl = re.findall(r"\bttts_" + name + r"\s*\(([^;{]*)\)\s*;", header)
        assert len(decl) == 1 and decl[0].count(",") + 1 == n, (name, decl)


# ---------------------------------------------------------------------------------------------------------------- refusals
# One row: (id, needle, keyword arguments that replace the defaults, note).  `note` is None where the parent of the commit that
# stated the host body once refuses the same call with the same needle under the entry's own name; otherwise it says
# what that parent did instead, and the row's test id ends in `parent_differs`:
#   crash     the process ended with SIGFPE (a division by zero in the planner: no dimension was looked at before it)
#   accepted  no -1: the convolution entries checked no dimension and no parity of `taps`
#   name      the message named the family (`linear_bwd_weight:` / `conv1d_bwd_weight:` for the _x6 / _h3 entries, `weight
#             gradient:` for the 4 GiB refusal), not the entry
#   wording   another message for the same fault (`parts` reported K % 4 as bad dims and N % 4 through its block split)
# Run on that parent with `-k "not parent_differs"`.
def _rows(name):
    form, kind, order = ENTRIES[name]
    named = None if name in ("linear_bwd_weight", "conv1d_bwd_weight", "linear_bwd_weight_h3_parts", "wgrad_group") else "name"
    rows = []

    def row(rid, needle, note=None, **kw):
        rows.append((rid, needle, kw, note or named))

    group = kind == "group"
    one = (lambda v: [v]) if group else (lambda v: v)          # (a group's arguments are arrays: here of one member)
    required = [p for p in order if p in _POINTERS and p not in _OPTIONAL]
    assert {"dy", "x", "ws"} <= set(required) and (form != "h3") == (not set(_AMAX) <= set(required))
    for p in required:
        row(f"null_{p}", "null pointer", **{p: one(None)})
        if group:
            row(f"null_array_{p}", "bad arguments", **{p: None})
    dims = {"lin": ("M", "N", "K"), "parts": ("M", "N", "K"), "group": ("M", "N", "K", "taps"), "conv": ("B", "T", "cin", "cout", "taps")}[kind]
    bad_dims = "not of the group's class" if group else "bad dims"
    for d in dims:
        row(f"zero_{d}", bad_dims, "crash" if kind == "conv" else None, **{d: one(0)})
        row(f"negative_{d}", bad_dims, "accepted" if kind == "conv" else None, **{d: one(-8)})
    if kind == "conv":
        row("rows_2pow31", "B*T too large", "accepted", B=1 << 16, T=1 << 15)
        row("even_taps", "bad dims", "accepted", taps=4)
    else:
        row("rows_2pow31", bad_dims, M=one(1 << 31))
    n_, k_ = ("cout", "cin") if kind == "conv" else ("N", "K")
    multiple = "not of the group's class" if group else "multiple"
    row("N_mod_4", multiple, "wording" if kind == "parts" else None, **{n_: one(258)})
    row("K_mod_4", multiple, "wording" if kind == "parts" else None, **{k_: one(258)})
    for p in ("dy", "x", "ws"):
        row(f"misaligned_{p}", "16-byte aligned", **{p: one("a4")})
    if kind == "conv":
        row("4GiB_dy", "4 GiB", "name", B=1 << 10, T=1 << 10, cout=1024)
        row("4GiB_x", "4 GiB", "name", B=1 << 10, T=1 << 10, cin=1024)
    else:
        row("4GiB_dy", "4 GiB", None if group else "name", M=one(1 << 20), N=one(1024))
        row("4GiB_x", "4 GiB", None if group else "name", M=one(1 << 20), K=one(1024))
    row("workspace_short", "too small", ws_bytes=one("short"))
    if "row_shift" in order and not group:
        row("shift_without_T", "row_shift needs T>0", row_shift=1, T=0)
        row("shift_ragged_T", "row_shift needs T>0", row_shift=1, T=7)         # 640 rows are no whole number of 7-row utterances
    if kind == "parts":
        row("nparts_0", "does not split", nparts=0)
        row("nparts_65", "does not split", nparts=65)
        row("nparts_ragged", "does not split", nparts=3, dw_parts=["a"] * 3)
        row("null_destination", "null destination", dw_parts=["a", None])
    if group:
        row("n_0", "bad arguments", n=0)
        row("n_5", "bad arguments", n=5)
        two = {p: ["a", "a"] for p in _GROUP_MEMBER if p in _POINTERS}
        row("other_class", "not of the group's class", n=2, **two, ws_bytes=[_BIG] * 2, M=[640] * 2, N=[256] * 2, K=[256, 80], taps=[1] * 2,
            T=[0] * 2, row_shift=[0] * 2)
        row("shift_without_T", "needs its utterance length", row_shift=[1], T=[0])
        row("shift_ragged_T", "needs its utterance length", row_shift=[1], T=[7])
        row("conv_without_T", "needs its utterance length", taps=[5], T=[0])
        row("conv_with_shift", "takes no row shift", taps=[5], T=[320], row_shift=[1])
        # ttts_wgrad_group_ok(640, 256, 256, 4) answers class 1, as for any tap count: the parity is the launch's own check
        row("even_taps", "taps=4", "accepted", taps=[4], T=[320])
        # class 2 (whole 256 x 256 tiles by LDS-DMA) clips utterances of at least 16 rows only
        row("class2_short_T", "needs its utterance length", M=[25632], N=[1024], K=[256], row_shift=[1], T=[8])
    return rows


_ALL_ROWS = [(name, *r) for name in ENTRIES for r in _rows(name)]


def _call(lib, name, kw):
    form, kind, order = ENTRIES[name]
    buf = ctypes.create_string_buffer(64)
    a = (ctypes.addressof(buf) + 15) & ~15                       # a 16-byte aligned host address (never dereferenced)
    group = kind == "group"
    defaults = dict(M=640, N=256, K=256, B=2, T=320 if kind == "conv" else 0, cin=256, cout=256, taps=5 if kind == "conv" else 1,
                    row_shift=0, accumulate=0, nparts=2, n=1, ws_bytes=_BIG, queue=None, stream=None)
    defaults.update({p: "a" for p in _POINTERS})
    defaults.update(dw_parts=["a", "a"], dbias_parts=["a", "a"])
    if group:
        defaults.update({p: [defaults[p]] for p in _GROUP_MEMBER})
    unknown = set(kw) - set(order)
    assert not unknown, (name, unknown)
    args = {p: kw.get(p, defaults[p]) for p in order}
    if "short" in (args["ws_bytes"] if group else [args["ws_bytes"]]):
        need = _GROUP_DEFAULT_NEED if group else lib.ttts_wgrad_workspace_bytes(
            args["B"] * args["T"] if kind == "conv" else args["M"], args.get("cout", args.get("N")), args.get("cin", args.get("K")),
            args.get("taps", 1))
        assert need > 4
        args["ws_bytes"] = [need - 4] if group else need - 4     # one float short
    address = lambda v: None if v is None else a + 4 if v == "a4" else a      # noqa: E731
    keep = []

    def convert(p, v):
        if p in ("dw_parts", "dbias_parts") or (group and p in _POINTERS):
            if v is None:
                return None
            keep.append((ctypes.c_void_p * len(v))(*[address(e) for e in v]))
            return keep[-1]
        if p in _POINTERS:
            return address(v)
        if group and p in _GROUP_MEMBER:
            if v is None:
                return None
            ctype = {"ws_bytes": ctypes.c_size_t, "M": ctypes.c_int64}.get(p, ctypes.c_int)
            keep.append((ctype * len(v))(*v))
            return keep[-1]
        return v
    return getattr(lib, "ttts_" + name)(*[convert(p, args[p]) for p in order])


@pytest.mark.parametrize("name,rid,needle,kw,note", _ALL_ROWS,
                         ids=[f"{r[0]}-{r[1]}" + ("-parent_differs" if r[4] else "") for r in _ALL_ROWS])
def test_weight_gradient_entry_points_refuse_bad_arguments_with_a_message(name, rid, needle, kw, note):
    """One refusal table over the eight launching entries: rc == -1 and a message that holds `<entry>:` and the needle."""
    from transformertts_amd import _lib
    lib = _lib.load()
    rc = _call(lib, name, kw)
    msg = _lib.last_error()
    assert rc == -1, (name, rid, rc)
    assert msg.startswith(name + ":") and needle in msg, (name, rid, msg)


@pytest.mark.parametrize("name,rid,needle,kw,note", [r for r in _ALL_ROWS if r[2] in ("bad dims", "multiple") and r[1] != "rows_2pow31"],
                         ids=lambda v: v if isinstance(v, str) and ("_" in v) else "")
def test_dimension_refusals_print_their_values(name, rid, needle, kw, note):
    """(the parent's `bad dims` and the convolutions' `multiples of 4` named no value)"""
    from transformertts_amd import _lib
    lib = _lib.load()
    assert _call(lib, name, kw) == -1
    msg = _lib.last_error()
    for dim, v in kw.items():
        assert f"{dim}={v}" in msg, (name, rid, msg)


def test_the_refusal_table_is_complete():
    per_entry = {name: [r for r in _ALL_ROWS if r[0] == name] for name in ENTRIES}
    assert min(len(v) for v in per_entry.values()) >= 21 and len(_ALL_ROWS) > 8 * 24
    ids = [r[:2] for r in _ALL_ROWS]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("bad", [0, -1])
def test_the_size_queries_answer_zero_for_bad_dims(bad):
    """(on the parent the planner divided by the zero: SIGFPE)"""
    from transformertts_amd import _lib
    lib = _lib.load()
    good = (640, 256, 256, 1)
    for i in range(4):
        dims = good[:i] + (bad,) + good[i + 1:]
        assert lib.ttts_wgrad_workspace_bytes(*dims) == 0, dims
        assert lib.ttts_wgrad_group_ok(*dims) == 0, dims
    assert lib.ttts_wgrad_workspace_bytes(*good) > 0 and lib.ttts_wgrad_group_ok(*good) == 1


# ------------------------------------------------------------------------------------------------------------- size queries
# ttts_wgrad_group_ok and ttts_wgrad_workspace_bytes over M x N x K x taps, taken from the parent's library.  Classes: one digit per
# (N, K), K fastest, one string per (M, taps).  Bytes: a sha256 per M over the decimal values in the order (taps, N, K), plus
# literals for the training step's own weights.
GRID_M = (1, 255, 300, 6400, 6401, 13920, 25600, 25630, 49000, 50000, 55680, 200000)
GRID_NK = (20, 64, 80, 96, 128, 256, 300, 512, 768, 1024)
GRID_TAPS = (1, 5)
_SHORT = "0000000000000000000000004444440000444444003311111100331111110033111111003311111100331111110033111111"      # under 800 k-tiles
_LONG1 = "0000000000000000000000004444440000444444003311111100331111220033110000003311022200331202220033120222"
_LONG5 = "0000000000000000000000004444440000444444003311111100331202220033100000003312022200331202220033120222"
CLASSES = {(M, t): _SHORT if M < 25600 else _LONG1 if t == 1 else _LONG5 for M in GRID_M for t in GRID_TAPS}
STEP_BYTES = {
    (13920, 256, 256, 1): 28685312, (13920, 768, 256, 1): 49738752, (13920, 1024, 256, 1): 48422912, (13920, 256, 1024, 1): 48281600,
    (13920, 512, 256, 1): 45791232, (13920, 256, 80, 1): 9040896, (13920, 80, 256, 1): 8964160, (13920, 512, 80, 5): 31207424,
    (13920, 512, 512, 5): 47204352, (13920, 80, 512, 5): 31141760, (13920, 256, 256, 5): 49846272,
    (55680, 256, 256, 1): 32896000, (55680, 768, 256, 1): 65528832, (55680, 1024, 256, 1): 66318336, (55680, 256, 1024, 1): 66124800,
    (55680, 512, 256, 1): 50001920, (55680, 256, 80, 1): 10368000, (55680, 80, 256, 1): 10280000, (55680, 512, 80, 5): 31207424,
    (55680, 512, 512, 5): 62939136, (55680, 80, 512, 5): 31141760, (55680, 256, 256, 5): 65587200,
}
# NOT the parent's values: outputs of ONE tile over 50 000 rows and more, (parent's bytes, bytes now).  Alone in a grouped launch such
# a member is planned 256 row splits of at least 8 k-tiles (196 at 50 000 rows, 218 at 55 680); the parent's query covered the
# launches of its own only (at most 192 row splits of the fp32 form's 64 x 64 tiles), and the group refused the workspace.
ONE_TILE_BYTES = {
    (50000, 128, 128, 1): (12152832, 12945408), (50000, 80, 128, 1): (7595520, 8090880), (50000, 96, 128, 1): (9114624, 9709056),
    (50000, 128, 80, 1): (7630848, 8128512), (50000, 128, 96, 1): (9138176, 9734144),
    (55680, 128, 128, 1): (12152832, 14398464), (55680, 80, 128, 1): (7595520, 8999040), (55680, 96, 128, 1): (9114624, 10798848),
    (55680, 128, 80, 1): (7630848, 9040896), (55680, 128, 96, 1): (9138176, 10826752),
    (200000, 128, 128, 1): (12549120, 16512000), (200000, 80, 128, 1): (7843200, 10320000), (200000, 96, 128, 1): (9411840, 12384000),
    (200000, 128, 80, 1): (7879680, 10368000), (200000, 128, 96, 1): (9436160, 12416000),
}
BYTES_SHA256 = {
    1: "9007de80582ede5ef603bce797674abc4db631c003420d51f41aef4b1e79ed4c",
    255: "00230b1bfd56cdbfdf4299133870fd69d8f7bba60ca38222850ac10118596ad6",
    300: "b80da76a16d8ce6752df7bebcd1c73e5fa6077db3583d338d716a666addf4848",
    6400: "2fccb1dcaf405862ddd6130c0fbbf2e323ffb1ab25919538d7906fe181d04f40",
    6401: "39d25f3d6d2dac34c2bc07bdd230f8e5f954cffd37c421155695e4506274eb63",
    13920: "8828a78bb7e6914f7f12334815a4b714a9ac59d6b993e6585047d58a07df0ffc",
    25600: "bb390e84acab392be2226f086c2f246bfad3a3339272c8e367fad3dfa2d19a82",
    25630: "72eff2ec073bc5ffa833160b1650f142b1fafae411c0160da9b69fd594abc5b3",
    49000: "cc4e247ea5781b86ffce7b20cd451eba89002e1632709ca6a35a00906c873eff",
    # (with the fifteen larger values above; the parent's digests: 21d6876d18e0..., 0b57afe0f4a4..., 1411aa68ca86...)
    50000: "e796b6a0068581ac1ea98409cfce54b6995b934ca4a6ecda142ba807d6a6b9e3",
    55680: "450c7888401002610f199a5af93e6271b3d9f4126df0e9c8006aa2e00c1a6f32",
    200000: "92b200adbeaf902cb1f627661bbfcb247931a1294d8779bc8f566edb7baa5921",
}


def _bytes_digest(lib, M):
    vals = [lib.ttts_wgrad_workspace_bytes(M, N, K, t) for t, N, K in itertools.product(GRID_TAPS, GRID_NK, GRID_NK)]
    return hashlib.sha256(",".join(map(str, vals)).encode()).hexdigest()


def test_the_class_of_every_problem_of_the_grid():
    from transformertts_amd import _lib
    lib = _lib.load()
    assert set(CLASSES) == set(itertools.product(GRID_M, GRID_TAPS))
    for (M, t), digits in CLASSES.items():
        got = "".join(str(lib.ttts_wgrad_group_ok(M, N, K, t)) for N, K in itertools.product(GRID_NK, GRID_NK))
        assert got == digits, (M, t)


def test_the_workspace_of_every_problem_of_the_grid():
    from transformertts_amd import _lib
    lib = _lib.load()
    for (M, N, K, t), nbytes in STEP_BYTES.items():
        assert lib.ttts_wgrad_workspace_bytes(M, N, K, t) == nbytes, (M, N, K, t)
    # the lone one-tile members whose group plans more row splits than any launch of their own: the query now covers them
    for (M, N, K, t), (parent, now) in ONE_TILE_BYTES.items():
        assert parent < now == lib.ttts_wgrad_workspace_bytes(M, N, K, t), (M, N, K, t)
        assert lib.ttts_wgrad_group_ok(M, N, K, t) in (1, 3, 4)
    assert {m for m, *_ in ONE_TILE_BYTES} == {m for m in GRID_M if m >= 50000}
    assert set(BYTES_SHA256) == set(GRID_M)
    for M, digest in BYTES_SHA256.items():
        assert _bytes_digest(lib, M) == digest, M


# ----------------------------------------------------------------------------------------------------------------- recorder
class _Fake:
    """stands for a device tensor: an address, an element count, a device"""
    _next = [0x1000]

    def __init__(self, tag, numel=0):
        self.tag, self._numel, self.device = tag, numel, "gpu0"
        self._next[0] += 0x100
        self.addr = self._next[0]

    def data_ptr(self):
        return self.addr

    def numel(self):
        return self._numel

    def __repr__(self):
        return self.tag


class _StandIn:
    """records every launching entry; the two size queries answer as the real library does (host arithmetic)"""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if name in ("ttts_wgrad_group_ok", "ttts_wgrad_workspace_bytes"):
            return getattr(self.real, name)

        def entry(*args):
            self.calls.append((name[len("ttts_"):], args))
            return 0
        return entry


def _install(monkeypatch, groups, defer):
    from transformertts_amd import _lib, ops
    lib = _StandIn(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(ops, "_p", lambda t: t)
    monkeypatch.setattr(ops, "_stream", lambda: "stream")
    monkeypatch.setattr(ops, "_amax", lambda t: "amax(%r)" % (t,))
    monkeypatch.setattr(ops, "_ws", lambda nbytes, device: _Fake("ws", (nbytes + 3) // 4))
    monkeypatch.setattr(ops, "WGRAD_GROUPS", groups)
    monkeypatch.setattr(ops, "DEFER_REDUCE", defer)
    monkeypatch.setattr(ops, "WGRAD_SIDE_STREAM", False)
    queue = object.__new__(ops.ReduceQueue)              # (no library handle, no autograd engine: the fields __init__ sets)
    queue._lib, queue.handle, queue.keep, queue._armed, queue._side, queue._side_busy = lib, "queue", [], True, None, False
    queue.wg = {1: [], 2: [], 3: [], 4: []}
    return ops, lib, queue


# queue, WGRAD_GROUPS, DEFER_REDUCE, (M, N, K, taps, T, row_shift, conv) -> the class it is deferred into, or the entry launched now
_SMALL, _BIGW, _MEL_IN, _MEL_OUT = (13920, 256, 256, 1, 0, 0, False), (25630, 1024, 256, 1, 0, 0, False), (13920, 256, 80, 1, 870, -1, False), \
    (13920, 80, 256, 5, 870, 0, True)
_WEIGHT_GRADS = [
    (1, 1, 1, _SMALL, 1),
    (0, 1, 1, _SMALL, "linear_bwd_weight_h3"),                 # no queue: the destination is read right away
    (1, 0, 1, _SMALL, "linear_bwd_weight_h3"),
    (1, 1, 0, _SMALL, "linear_bwd_weight_h3"),
    (1, 1, 1, _BIGW, 2),
    (1, 1, 1, (25630, 1024, 256, 1, 2563, -1, False), "linear_bwd_weight_h3"),     # class 2 takes no shifted linear
    (1, 1, 1, (13920, 768, 256, 1, 0, 0, False), 1),
    (1, 1, 1, (55680, 768, 256, 1, 0, 0, False), 2),
    (1, 1, 1, (55680, 300, 1024, 1, 0, 0, False), "linear_bwd_weight_h3"),          # a ragged 256-wide tile: a launch of its own
    (1, 1, 1, (13920, 64, 64, 1, 0, 0, False), "linear_bwd_weight_x6"),             # no split-precision shape: no maxima either
    (1, 1, 1, (13920, 256, 20, 1, 0, 0, False), "linear_bwd_weight_x6"),
    (1, 1, 1, _MEL_IN, 3),
    (0, 1, 1, _MEL_IN, "linear_bwd_weight_h3"),
    (1, 1, 1, _MEL_OUT, 4),
    (0, 1, 1, _MEL_OUT, "conv1d_bwd_weight_h3"),
    (1, 1, 1, (13920, 512, 512, 5, 870, 0, True), 1),
    (1, 1, 1, (55680, 512, 512, 5, 870, 0, True), 2),
    (1, 1, 0, (55680, 512, 512, 5, 870, 0, True), "conv1d_bwd_weight_h3"),
    (1, 1, 1, (13920, 32, 32, 5, 870, 0, True), "conv1d_bwd_weight_x6"),
]


@pytest.mark.parametrize("with_queue,groups,defer,problem,expected", _WEIGHT_GRADS)
def test_weight_gradients_go_where_the_table_says(monkeypatch, with_queue, groups, defer, problem, expected):
    """`ops._weight_grad` on a stand-in library: deferred into the class the table names, or the entry and the argument list it
    names, in ABI order."""
    ops, lib, queue = _install(monkeypatch, bool(groups), bool(defer))
    M, N, K, taps, T, shift, conv = problem
    dy, x, dw, db, dya, xa = (_Fake(t) for t in ("dy", "x", "dw", "db", "dy_amax", "x_amax"))
    ops._weight_grad(dy, dya, x, xa, dw, db, 1, queue if with_queue else None, M, N, K, taps, T, shift, conv)
    if isinstance(expected, int):
        assert lib.calls == [] and [c for c in (1, 2, 3, 4) if queue.wg[c]] == [expected]
        assert len(queue.wg[expected]) == 1
        return
    assert not any(queue.wg.values())
    (entry, args), = lib.calls
    assert entry == expected
    ws = args[4]
    nbytes = lib.real.ttts_wgrad_workspace_bytes(M, N, K, taps)
    assert isinstance(ws, _Fake) and ws.numel() * 4 >= nbytes
    dims = (M // T, T, K, N, taps) if conv else (M, N, K, shift, T)
    maxima = (dya, xa) if expected.endswith("_h3") else ()
    qarg = "queue" if (with_queue and defer) else None
    assert args == (dy, x, dw, db, ws, ws.numel() * 4, *dims, 1, *maxima, qarg, "stream")
    assert len(args) == len(ENTRIES[entry][2])
    assert queue.keep == ([ws] if qarg else [])


def test_a_group_reaches_the_library_in_abi_order(monkeypatch):
    """`ReduceQueue.launch_wgrads`: the members' fields as the argument list of ttts_wgrad_group -- a full group launches itself, a
    leftover group of one at the flush, a member of another row count launches what waits."""
    ops, lib, queue = _install(monkeypatch, True, True)
    assert ops.WGRAD_GROUP_SIZE == {1: 4, 2: 3, 3: 2, 4: 2}
    M = 13920
    shapes = [(256, 256, 1, 0, 0), (128, 384, 1, 0, 0), (256, 128, 5, 870, 0), (384, 256, 1, 870, -1)]
    members = []
    for i, (N, K, taps, T, shift) in enumerate(shapes):
        assert lib.real.ttts_wgrad_group_ok(M, N, K, taps) == 1
        t = {k: _Fake(f"{k}{i}") for k in ("dy", "dy_amax", "x", "x_amax", "dw", "db")}
        if i == 1:
            t["db"] = None                                         # (a member without a bias)
        members.append(t)
        assert lib.calls == []
        ops._weight_grad(t["dy"], t["dy_amax"], t["x"], t["x_amax"], t["dw"], t["db"], 1, queue, M, N, K, taps, T, shift, taps > 1)
    (entry, args), = lib.calls
    assert entry == "wgrad_group" and len(args) == len(ENTRIES["wgrad_group"][2]) and not queue.wg[1]
    n, dy, x, dw, dbias, ws, ws_bytes, Ms, Ns, Ks, taps_, Ts, shifts, acc, dya, xa, q, stream = args
    addr = lambda key: [m[key].addr if m[key] is not None else None for m in members]      # noqa: E731
    assert n == 4 and (acc, q, stream) == (1, "queue", "stream")
    assert (list(dy), list(x), list(dw), list(dbias)) == (addr("dy"), addr("x"), addr("dw"), addr("db"))
    assert (list(dya), list(xa)) == (addr("dy_amax"), addr("x_amax"))
    assert list(Ms) == [M] * 4 and list(Ns) == [s[0] for s in shapes] and list(Ks) == [s[1] for s in shapes]
    assert list(taps_) == [s[2] for s in shapes] and list(Ts) == [s[3] for s in shapes] and list(shifts) == [s[4] for s in shapes]
    assert list(ws_bytes) == [w.numel() * 4 for w in queue.keep] and list(ws) == [w.addr for w in queue.keep] and len(queue.keep) == 4
    for nbytes, (N, K, taps, T, shift) in zip(ws_bytes, shapes):
        assert nbytes >= lib.real.ttts_wgrad_workspace_bytes(M, N, K, taps)
    # a leftover member, then one of another row count: the first is launched as a group of one before the second waits
    lib.calls.clear()
    f = [_Fake(f"t{i}") for i in range(12)]
    ops._weight_grad(f[0], f[1], f[2], f[3], f[4], f[5], 1, queue, M, 256, 256)
    ops._weight_grad(f[6], f[7], f[8], f[9], f[10], f[11], 1, queue, 6400, 256, 256)
    assert [(e, a[0], list(a[7])) for e, a in lib.calls] == [("wgrad_group", 1, [M])] and len(queue.wg[1]) == 1
    lib.calls.clear()
    queue.launch_wgrads()
    assert [(e, a[0], list(a[7]), list(a[1])) for e, a in lib.calls] == [("wgrad_group", 1, [6400], [f[6].addr])]
    assert not any(queue.wg.values())


@pytest.mark.parametrize("with_queue", [0, 1])
def test_an_even_tap_count_reaches_neither_a_group_nor_an_entry(monkeypatch, with_queue):
    """`ops._weight_grad` / `ReduceQueue.defer_wgrad` refuse a convolution with an even tap count themselves: the class query
    answers 1 for (640, 256, 256, 4), so without the guard the member would wait in a group."""
    ops, lib, queue = _install(monkeypatch, True, True)
    assert lib.real.ttts_wgrad_group_ok(640, 256, 256, 4) == 1
    f = [_Fake(f"t{i}") for i in range(6)]
    with pytest.raises(ValueError, match="taps=4"):
        ops._weight_grad(*f, 1, queue if with_queue else None, 640, 256, 256, 4, 320, 0, True)
    with pytest.raises(ValueError, match="taps=4"):
        queue.defer_wgrad(1, *f, 640, 256, 256, 4, 320)
    assert lib.calls == [] and not any(queue.wg.values())
