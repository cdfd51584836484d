#!/usr/bin/env python3
"""What the variance predictor on the library's kernels costs: one length-masked Conv1d -> ReLU -> LayerNorm ->
Dropout stage of csrc/predictor.hip, forward and backward, against the stock form `VariancePredictor` uses (a `where`, three
shifted `cat`s, `F.linear`, `relu`, `layer_norm`), and the whole `KernelVariancePredictor` against `VariancePredictor`, both sides
alternating round by round in one process.

    python tools/predictor_bench.py [--rounds 5] [--reps 20] [--out profiles/predictor_bench.txt] [--label TEXT]

Shapes: the flagship's B = 64 utterances of 110 phonemes x 256 channels (hidden 256, 3 taps), the same for B = 1, and a ragged
batch of 64 utterances of 20 .. 110 phonemes.  Times: device events around `reps` calls after a warm-up, the median and minimum
over the rounds, in microseconds, twice: `us` with every call issued from Python (forward under `no_grad`, `fwd+bwd` through
autograd with dropout 0.5 in training mode), and `graph_us` with the `reps` calls captured into one HIP graph and replayed, the
device's time alone (forwards under `no_grad`; the kernel side's stage backward as the C entries autograd calls; the stock
backwards are not captured, they need the autograd engine).  Prints one JSON line per shape and appends it to `--out`."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

P, D, HIDDEN, TAPS = 110, 256, 256, 3
SHAPES = [(64, False), (1, False), (64, True)]


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def captured(fn, reps):
    """`reps` calls of fn as one HIP graph -> a callable that replays it (fn must not go through the autograd engine)"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        for _ in range(reps):
            fn()
    torch.cuda.synchronize()
    return graph.replay


def stock_stage(pred, conv, norm, x, valid, drop):
    keep, zero = valid[:, :, None], x.new_zeros(())
    return drop(norm(torch.relu(pred._conv(conv, torch.where(keep, x, zero)))))


def kernel_stage_entries(x, lens, conv, norm, dy):
    """the stage's training forward and its backward as the C entries `ragged_conv_norm` calls, on buffers made once"""
    from transformertts_amd import _lib
    from transformertts_amd.ops import _p, _stream, _ws
    lib = _lib.load()
    B, Pmax, Cin = x.shape
    Cout = conv.out_channels
    dev = x.device
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    y, r, mean, rstd, xm = new(B, Pmax, Cout), new(B, Pmax, Cout), new(B, Pmax), new(B, Pmax), new(B, Pmax, Cin)
    dx, dw, db, dg, dbe = new(B, Pmax, Cin), new(Cout, Cin, TAPS), new(Cout), new(Cout), new(Cout)
    ws = _ws(lib.ttts_ragged_conv_norm_workspace_bytes(B, Pmax, Cin, Cout, TAPS), dev)
    w, bias, gamma, beta = (t.detach() for t in (conv.weight, conv.bias, norm.weight, norm.bias))

    def fwd():
        _lib.check(lib.ttts_ragged_conv_norm_fwd(_p(x), Cin, Pmax * Cin, _p(lens), _p(w), _p(bias), _p(gamma), _p(beta), B, Pmax, Cin, Cout,
                                                 TAPS, norm.eps, 0.5, 12345, None, _p(y), _p(r), _p(mean), _p(rstd), _p(xm), _stream()),
                   "ttts_ragged_conv_norm_fwd")

    def bwd():
        _lib.check(lib.ttts_ragged_conv_norm_bwd(_p(dy), _p(r), _p(mean), _p(rstd), _p(xm), _p(lens), _p(w), _p(gamma), B, Pmax, Cin, Cout,
                                                 TAPS, 0.5, 12345, None, _p(dx), _p(dw), _p(db), _p(dg), _p(dbe), _p(ws), ws.numel() * 4, 0,
                                                 _stream()), "ttts_ragged_conv_norm_bwd")
    return fwd, bwd


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    from transformertts_amd import KernelVariancePredictor, VariancePredictor, ragged_conv_norm
    dev = "cuda:0"
    torch.manual_seed(0)
    stock = VariancePredictor(D, hidden=HIDDEN, kernel_size=TAPS).to(dev)
    ours = KernelVariancePredictor(D, hidden=HIDDEN, kernel_size=TAPS).to(dev)
    ours.load_state_dict(stock.state_dict(), strict=True)
    for B, ragged in SHAPES:
        gen = torch.Generator().manual_seed(7 + B + ragged)
        lens_host = [int(round(20 + (P - 20) * b / max(1, B - 1))) for b in range(B)] if ragged else [P] * B
        lens = torch.tensor(lens_host, device=dev)
        x = torch.randn(B, P, D, generator=gen).to(dev)
        dy, dout = torch.randn(B, P, HIDDEN, generator=gen).to(dev), torch.randn(B, P, generator=gen).to(dev)
        valid = torch.arange(P, device=dev)[None, :] < lens[:, None]
        xg = x.clone().requires_grad_(True)
        c, n = ours.conv1, ours.norm1
        e_fwd, e_bwd = kernel_stage_entries(x, lens, c, n, dy)

        def k_stage_fb():
            ragged_conv_norm(xg, lens, c.weight, c.bias, n.weight, n.bias, eps=n.eps, drop_p=0.5, seed=12345).backward(dy)

        def s_stage_fb():
            stock_stage(stock, stock.conv1, stock.norm1, xg, valid, stock.drop).backward(dy)

        def k_pred_fb():
            ours(xg, lens).backward(dout)

        def s_pred_fb():
            stock(xg, lens).backward(dout)

        def nograd(fn):
            def run():
                with torch.no_grad():
                    fn()
            return run
        k_stage_f = nograd(lambda: ragged_conv_norm(x, lens, c.weight, c.bias, n.weight, n.bias, eps=n.eps))
        s_stage_f = nograd(lambda: stock_stage(stock.eval(), stock.conv1, stock.norm1, x, valid, stock.drop))
        k_pred_f, s_pred_f = nograd(lambda: ours.eval()(x, lens)), nograd(lambda: stock.eval()(x, lens))
        python_side = {"stage_fwd": (k_stage_f, s_stage_f), "stage_fwd+bwd": (lambda: (ours.train(), k_stage_fb()), lambda: (stock.train(), s_stage_fb())),
                       "predictor_fwd": (k_pred_f, s_pred_f),
                       "predictor_fwd+bwd": (lambda: (ours.train(), k_pred_fb()), lambda: (stock.train(), s_pred_fb()))}
        ours.eval(), stock.eval()
        graph_side = {"stage_fwd": (captured(k_stage_f, args.reps), captured(s_stage_f, args.reps)),
                      "predictor_fwd": (captured(k_pred_f, args.reps), captured(s_pred_f, args.reps)),
                      "stage_train_fwd_entries": (captured(e_fwd, args.reps), None),
                      "stage_bwd_entries": (captured(e_bwd, args.reps), None)}
        times = {}
        for _ in range(args.rounds):                                  # the two sides alternate inside every round
            for name, pair in python_side.items():
                for side, fn in zip(("kernel", "stock"), pair):
                    fn()
                    times.setdefault(("us", name, side), []).append(timed(fn, args.reps))
            for name, pair in graph_side.items():
                for side, replay in zip(("kernel", "stock"), pair):
                    if replay is not None:
                        replay()
                        times.setdefault(("graph_us", name, side), []).append(timed(replay, 1) / args.reps)
        row = {"tool": "predictor_bench", "label": args.label, "B": B, "ragged": ragged, "phonemes": P, "rows": sum(lens_host), "d_model": D,
               "hidden": HIDDEN, "taps": TAPS, "rounds": args.rounds, "reps": args.reps, "device": torch.cuda.get_device_name(0)}
        for (base, name, side), v in times.items():
            row[f"{name}.{side}.{base}"] = [round(statistics.median(v), 2), round(min(v), 2)]
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
