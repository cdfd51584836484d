"""What `ops._linear_fwd` / `ops._linear_bwd_data` launch, recorded without a GPU over a grid of shapes, options and flags.

    python tools/gemm_route_ab.py > record.txt        (run in two trees, then diff the two records)

The library is replaced by an object whose attributes record their name and return 0, `ops._planes` / `ops._amax` record their
call, so one line of the record is the launch pattern of one call: `planes <mode> <rows>x<cols>` (dimension letters as the caller
names them), `amax` (the operand's maxima are measured: none are handed in), then the entry point.  Each record line holds one combination of direction, options and flags and one letter
per (rows, depth, width) of the grid; the letters are the patterns listed at the end.  tests/test_gemm_entry_host.py runs the same
recorder against `ops._linear_route`; profiles/gemm_route_ab.txt is the record of this tree, identical to its parent's."""
import itertools
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

ROWS = (4096, 8192, 13920, 41760, 65536)
DEPTHS = (80, 250, 256, 512, 1024)
WIDTHS = (80, 81, 256, 512, 1024, 2048)
FLAGS = ({}, {"DMA_GEMMS": False}, {"DMA_BIG_FWD": False}, {"LAYERNORM_IMAGES": True})
FAMILY = {"x6": "x", "h3i": "i", "h3d": "d", "h3": "h"}


class Recorder:
    """`install(setattr-like)` puts the stand-ins into ops; `fwd` / `bwd` make one call and return what it launched"""

    def __init__(self, ops, torch, _lib):
        self.ops, self.torch, self._lib, self.log = ops, torch, _lib, []

    def install(self, setter, capturing: bool = False) -> None:
        rec = self

        class Lib:
            def __getattr__(self, name):
                def entry(*args):
                    rec.log.append(name[len("ttts_"):])
                    rec.args = args
                    return 0
                return entry

        def planes(w, mode, rows, cols, c2=0, taps=0):
            rec.log.append(f"planes {mode} {rec.dims(rows, cols)}")
            return None

        def amax(t):
            rec.log.append("amax")
            return None

        lib = Lib()
        setter(self._lib, "load", lambda: lib)
        setter(self.ops, "_planes", planes)
        setter(self.ops, "_amax", amax)
        setter(self.ops, "_stream", lambda: None)
        setter(self.ops, "_p", lambda t: t)
        setter(self.torch.cuda, "is_current_stream_capturing", lambda: capturing)

    def dims(self, rows: int, cols: int) -> str:
        """(the forward image is the weight's own N x K, the data gradient's its transpose)"""
        want = (self.K, self.N) if self.bwd_call else (self.N, self.K)
        return ("KxN" if self.bwd_call else "NxK") if (rows, cols) == want else f"{rows}x{cols}"

    def call(self, fn, N, K, *args, **kw):
        self.log, self.N, self.K, self.bwd_call = [], N, K, fn is self.ops._linear_bwd_data
        fn(*args, **kw)
        return ", ".join(self.log)

    def fwd(self, M, K, N, image: bool, tiles: bool, shift: int):
        epi = (0, 0.0, 0, None, shift, 64 if shift else 0)
        return self.call(self.ops._linear_fwd, N, K, "x", "w", None, None, "y", M, N, K, None, None, epi,
                         ("x_image", "x_row_inv") if image else None, tiles)

    def bwd(self, M, N, K, image: bool, tiles: bool, gate: bool, skip: bool, w_image: bool):
        return self.call(self.ops._linear_bwd_data, N, K, "dy", None if w_image else "w", "dx", M, N, K, None,
                         "skip" if skip else None, "gate" if gate else None, 1.0, None, ("dy_image", "dy_row_inv") if image else None,
                         tiles, "w_image" if w_image else None)


def combos():
    """-> (direction, label, keyword arguments) of every option combination of the grid"""
    tf = (False, True)
    for image, tiles, shift in itertools.product(tf, tf, (0, 1)):
        yield "fwd", f"image={int(image)} tiles={int(tiles)} shift={shift}", dict(image=image, tiles=tiles, shift=shift)
    for image, tiles, gate, skip, w_image in itertools.product(tf, tf, tf, tf, tf):
        yield ("bwd", f"image={int(image)} tiles={int(tiles)} gate={int(gate)} skip={int(skip)} w_image={int(w_image)}",
               dict(image=image, tiles=tiles, gate=gate, skip=skip, w_image=w_image))


def shapes():
    """(rows, reduction depth, output width) in the order of a line's letters"""
    return itertools.product(ROWS, DEPTHS, WIDTHS)


def launch(rec: Recorder, direction: str, M: int, red: int, out: int, kw) -> str:
    return rec.fwd(M, red, out, **kw) if direction == "fwd" else rec.bwd(M, red, out, **kw)


def main() -> None:
    import torch
    from transformertts_amd import _lib, ops
    rec = Recorder(ops, torch, _lib)
    rec.install(setattr)
    patterns: dict = {}
    print(f"# rows {ROWS} x depth {DEPTHS} x width {WIDTHS}: one letter per shape, width fastest")
    for flags in FLAGS:
        saved = {k: getattr(ops, k) for k in flags}
        for k, v in flags.items():
            setattr(ops, k, v)
        tag = " ".join(f"{k}={v}" for k, v in flags.items()) or "defaults"
        for direction, label, kw in combos():
            letters = ""
            for M, red, out in shapes():
                key = (direction, launch(rec, direction, M, red, out, kw))
                letters += patterns.setdefault(key, chr(ord("a") + len(patterns)))
            print(f"{tag} | {direction} {label} | {letters}")
        for k, v in saved.items():
            setattr(ops, k, v)
    for (direction, pattern), letter in patterns.items():
        print(f"# {letter} = {direction}: {pattern}")


if __name__ == "__main__":
    main()
