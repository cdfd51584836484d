"""One sha256 per shape -- over the digests of every buffer of every run on it; `--buffers`: one line per buffer -- of the eight
launching weight-gradient entry points (three Linear forms, `parts`, the grouped launch, three Conv1d forms) on fixed seeded
inputs, and the two size queries over a grid: an A/B of two builds of the library.

    TTTS_LIB=<libttts_hip.so of build A> python tools/wgrad_entry_ab.py > a.txt
    TTTS_LIB=<libttts_hip.so of build B> python tools/wgrad_entry_ab.py > b.txt      (a fresh process each), then diff a.txt b.txt
    TTTS_LIB=... python tools/wgrad_entry_ab.py --sizes                               (the size queries only: needs no GPU)
    (--buffers / --sizes --rows: the lines behind a digest that differs)

The buffers are dw, dbias and the WHOLE workspace, which holds a fixed bit pattern before the call: its digest shows exactly which
part a launch wrote, and with that the row-split count its plan chose.  Shapes: the parametrisations of tests/test_hip_modes.py, and
the training step's weights over 25 630 and 55 680 rows (every tile, both workgroup targets).  Every entry runs with `accumulate`
0 and 1, without a queue and with a queue that is flushed; Linear with and without a row shift; groups of every class with all
biases and with one member that has none.  Exits non-zero when an entry refuses.  profiles/wgrad_entry_ab.txt holds both outputs
of this tree and of its parent."""
import ctypes
import hashlib
import itertools
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from transformertts_amd import _lib  # noqa: E402

GRID_M = (1, 255, 300, 6400, 6401, 13920, 25600, 25630, 49000, 50000, 55680, 200000)
GRID_NK = (20, 64, 80, 96, 128, 256, 300, 512, 768, 1024)
PATTERN = 0x5A5AC3C3                      # what the workspace holds where no launch wrote
STEP_ROWS = (25630, 55680)
STEP_LINEAR = [(256, 256), (768, 256), (1024, 256), (256, 1024), (256, 80), (80, 256)]
STEP_CONV = [(80, 512), (512, 512), (512, 80)]           # (cin, cout), five taps
TEST_LINEAR = [(300, 256, 256), (1000, 1024, 256), (777, 256, 1024), (129, 80, 256), (4000, 256, 80), (70, 20, 64)]
TEST_CONV = [(3, 50, 128, 256), (2, 7, 256, 128), (5, 1, 128, 128), (6, 45, 80, 256), (6, 45, 256, 80), (30, 870, 256, 256), (31, 833, 512, 256),
             (1600, 16, 256, 256), (4, 33, 32, 48)]
# (M, T, [(N, K, taps, row_shift)]) of a grouped launch
GROUPS = [(13920, 870, [(256, 256, 1, 0)] * 4), (6401, 0, [(768, 256, 1, 0), (256, 256, 1, 0), (1024, 256, 1, 0), (256, 1024, 1, 0)]),
          (300, 0, [(256, 256, 1, 0), (128, 384, 1, 0)]), (55680, 0, [(256, 256, 1, 0)]),
          (25630, 0, [(256, 1024, 1, 0), (1024, 256, 1, 0), (768, 256, 1, 0)]), (27001, 0, [(512, 512, 1, 0)]),
          (6400, 100, [(256, 256, 5, 0)] * 3 + [(256, 256, 1, 0)]), (26100, 870, [(256, 256, 5, 0)] * 3), (231, 33, [(256, 128, 5, 0), (128, 256, 5, 0)]),
          (13920, 870, [(256, 80, 5, 0), (256, 80, 1, -1)]), (13920, 870, [(80, 256, 5, 0), (80, 256, 1, 0)]),
          (55680, 870, [(512, 80, 5, 0), (256, 80, 1, -1)]), (55680, 870, [(80, 512, 5, 0), (80, 256, 1, 0)])]


def sizes(lib) -> None:
    """bytes/class per (N, K) of the grid: one digest per (M, taps), or (--rows) one line per N"""
    for M, t in itertools.product(GRID_M, (1, 5)):
        rows = [f"sizes M{M} taps{t} N{N} | " + " ".join(f"{lib.ttts_wgrad_workspace_bytes(M, N, K, t)}/{lib.ttts_wgrad_group_ok(M, N, K, t)}"
                                                     for K in GRID_NK) for N in GRID_NK]
        print("\n".join(rows) if "--rows" in sys.argv else f"sizes M{M} taps{t} {hashlib.sha256(chr(10).join(rows).encode()).hexdigest()}")


def main() -> None:
    lib = _lib.load()
    print(f"# abi {lib.ttts_abi_version()}")
    if "--sizes" in sys.argv:
        return sizes(lib)
    import torch
    from transformertts_amd import ops
    from transformertts_amd.ops import _p, _stream
    dev = torch.device("cuda:0")
    cache: dict = {}

    def rand(rows, cols, seed, scale=1.0):
        key = (rows, cols, seed, scale)
        if key not in cache:
            if len(cache) > 6:
                cache.clear()
            cache[key] = (torch.randn(rows, cols, generator=torch.Generator().manual_seed(seed)) * scale).to(dev)
        return cache[key]

    def digest(t) -> str:
        torch.cuda.synchronize()
        return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()

    def workspace(M, N, K, taps):
        return torch.full((lib.ttts_wgrad_workspace_bytes(M, N, K, taps) // 4,), PATTERN, dtype=torch.int32, device=dev).view(torch.float32)

    def modes(big: bool):
        """(accumulate, queued): all four, or for the long row ranges the two that differ in both"""
        return ((0, 0), (1, 1)) if big else ((0, 0), (1, 0), (0, 1), (1, 1))

    pending: list = [None, []]              # the shape whose lines are being collected, and the lines

    def emit(key, line):
        if key != pending[0]:
            if pending[0] is not None and "--buffers" not in sys.argv:
                print(f"{pending[0]} {len(pending[1])} buffers {hashlib.sha256(chr(10).join(pending[1]).encode()).hexdigest()}")
            pending[0], pending[1] = key, []
        if key is not None:
            pending[1].append(line)
            if "--buffers" in sys.argv:
                print(line)

    def launch(entry, case, call, outs, wss):
        """call(queue) -> rc; with a queue the reductions run at its flush"""
        acc, queued = case[-2:]
        q = ctypes.c_void_p(lib.ttts_reduce_queue_create()) if queued else None
        rc = call(q)
        if rc != 0:
            sys.exit(f"{entry} {case}: rc {rc}: {_lib.last_error()}")
        if queued:
            _lib.check(lib.ttts_reduce_queue_flush(q, _stream()), "ttts_reduce_queue_flush")
            torch.cuda.synchronize()
            lib.ttts_reduce_queue_destroy(q)
        tag = "_".join(str(c) for c in case[:-2]) + f"_acc{acc}_q{queued}"
        for name, t in list(outs.items()) + [(f"ws{i}" if len(wss) > 1 else "ws", w) for i, w in enumerate(wss)]:
            if t is not None:
                emit(f"{entry} {case[0].rsplit('_bias', 1)[0]}", f"{entry} {tag} {name} {digest(t.view(torch.int32) if name.startswith('ws') else t)}")

    def sink(*shape, value):
        return torch.full(shape, value, device=dev)

    def linear(form, M, N, K, shift, T, big):
        fn = getattr(lib, "ttts_linear_bwd_weight" + form)
        dy, x = rand(M, N, 1, 1e-3), rand(M, K, 2)
        maxima = (_p(ops._amax(dy)), _p(ops._amax(x))) if form == "_h3" else ()
        for bias, (acc, queued) in itertools.product((1, 0), modes(big)):
            if not bias and (acc, queued) != (0, 0):
                continue
            dw, db, ws = sink(N, K, value=0.5), sink(N, value=-0.25) if bias else None, workspace(M, N, K, 1)
            launch("linear_bwd_weight" + form, (f"M{M}_N{N}_K{K}_shift{shift}_bias{bias}", acc, queued),
                   lambda q: fn(_p(dy), _p(x), _p(dw), _p(db), _p(ws), ws.numel() * 4, M, N, K, shift, T, acc, *maxima, q, _stream()),
                   dict(dw=dw, dbias=db), [ws])

    def conv(form, B, T, cin, cout, taps, big):
        fn = getattr(lib, "ttts_conv1d_bwd_weight" + form)
        M = B * T
        dy, x = rand(M, cout, 3, 1e-3), rand(M, cin, 4)
        maxima = (_p(ops._amax(dy)), _p(ops._amax(x))) if form == "_h3" else ()
        for bias, (acc, queued) in itertools.product((1, 0), modes(big)):
            if not bias and (acc, queued) != (0, 0):
                continue
            dw, db, ws = sink(cout, cin, taps, value=0.5), sink(cout, value=-0.25) if bias else None, workspace(M, cout, cin, taps)
            launch("conv1d_bwd_weight" + form, (f"B{B}_T{T}_cin{cin}_cout{cout}_taps{taps}_bias{bias}", acc, queued),
                   lambda q: fn(_p(dy), _p(x), _p(dw), _p(db), _p(ws), ws.numel() * 4, B, T, cin, cout, taps, acc, *maxima, q, _stream()),
                   dict(dw=dw, dbias=db), [ws])

    def parts(M, L, Np, K, big):
        N = L * Np
        dy, x = rand(M, N, 5, 1e-3), rand(M, K, 6)
        PA = ctypes.c_void_p * L
        for bias, (acc, queued) in itertools.product((1, 0), modes(big)):
            if not bias and (acc, queued) != (0, 0):
                continue
            dws, dbs, ws = [sink(Np, K, value=0.5) for _ in range(L)], [sink(Np, value=-0.25) for _ in range(L)], workspace(M, N, K, 1)
            launch("linear_bwd_weight_h3_parts", (f"M{M}_L{L}_Np{Np}_K{K}_bias{bias}", acc, queued),
                   lambda q: lib.ttts_linear_bwd_weight_h3_parts(_p(dy), _p(x), PA(*[t.data_ptr() for t in dws]),
                                                                 PA(*[t.data_ptr() for t in dbs]) if bias else None, L, _p(ws), ws.numel() * 4,
                                                                 M, N, K, acc, _p(ops._amax(dy)), _p(ops._amax(x)), q, _stream()),
                   dict(dw=torch.cat(dws), dbias=torch.cat(dbs) if bias else None), [ws])

    def group(M, T, members, big):
        n = len(members)
        PA, ZA, LA, IA = ctypes.c_void_p * n, ctypes.c_size_t * n, ctypes.c_int64 * n, ctypes.c_int * n
        ptr = lambda ts: PA(*[(t.data_ptr() if t is not None else None) for t in ts])      # noqa: E731
        dys = [(torch.randn(M, N, generator=torch.Generator().manual_seed(20 + i)) * (3e-7 if i == 0 else 1.0)).to(dev) for i, (N, K, t, s) in enumerate(members)]
        xs = [torch.randn(M, K, generator=torch.Generator().manual_seed(10 + i)).to(dev) for i, (N, K, t, s) in enumerate(members)]
        ams, xms = [ops._amax(t) for t in dys], [ops._amax(t) for t in xs]
        cls = lib.ttts_wgrad_group_ok(M, *members[0][:3])
        for bias, (acc, queued) in itertools.product(("all", "but1"), modes(big)):
            if bias == "but1" and (acc, queued) != (0, 0):
                continue
            dws = [sink(N * K * t, value=0.5) for N, K, t, s in members]
            dbs = [sink(N, value=-0.25) if (bias == "all" or i != min(1, n - 1)) else None for i, (N, K, t, s) in enumerate(members)]
            wss = [workspace(M, N, K, t) for N, K, t, s in members]
            shape = "+".join(f"{N}x{K}x{t}" + (f"s{s}" if s else "") for N, K, t, s in members)
            launch("wgrad_group", (f"class{cls}_M{M}_{shape}_bias{bias}", acc, queued),
                   lambda q: lib.ttts_wgrad_group(n, ptr(dys), ptr(xs), ptr(dws), ptr(dbs), ptr(wss), ZA(*[w.numel() * 4 for w in wss]), LA(*[M] * n),
                                                  IA(*[m[0] for m in members]), IA(*[m[1] for m in members]), IA(*[m[2] for m in members]),
                                                  IA(*[T if (m[2] > 1 or m[3]) else 0 for m in members]), IA(*[m[3] for m in members]), acc,
                                                  ptr(ams), ptr(xms), q, _stream()),
                   {f"dw{i}": t for i, t in enumerate(dws)} | {f"dbias{i}": t for i, t in enumerate(dbs)}, wss)

    for form in ("", "_x6", "_h3"):
        for M, N, K in TEST_LINEAR:
            linear(form, M, N, K, 0, 0, False)
            if M % 10 == 0:
                linear(form, M, N, K, -1, M // 10, True)
        for M, (N, K) in itertools.product(STEP_ROWS, STEP_LINEAR):
            linear(form, M, N, K, 0, 0, True)
        linear(form, 55680, 256, 80, -1, 870, True)               # the decoder pre-net's go-frame shift
        for B, T, cin, cout in TEST_CONV:
            conv(form, B, T, cin, cout, 5, B * T > 20000)
        conv(form, 5, 1, 128, 128, 1, False)
        for (B, T), (cin, cout) in itertools.product(((11, 2330), (64, 870)), STEP_CONV):
            conv(form, B, T, cin, cout, 5, True)
    parts(6400, 3, 512, 256, False)
    for M in STEP_ROWS:
        parts(M, 6, 512, 256, True)
    for M, T, members in GROUPS:
        group(M, T, members, M > 20000)
    emit(None, "")
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
