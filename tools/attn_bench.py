#!/usr/bin/env python3
"""Self- / cross-attention forward and backward on the step's shapes through the ops layer (fp16x3 kernels), per-kernel
times from HIP events around the forward and the backward call, and a check against fp64 torch (development aid).
A/B two builds with TTTS_LIB=<lib>.

    --head-dim N (default 64): N > 64 runs the `wide` configuration's shapes (B=8, H=8; causal self T=870, self T=100, cross
    870 x 100 WITH weights) on the 128-column fp32-MFMA kernels and, interleaved with them round by round in the same process,
    on ops.masked_attention -- stock torch differentiated by autograd, the route these head widths took before the kernels
    existed -- and prints forward + backward time and peak memory of both.

    --masked: the same three shapes at head_dim 128 and the base model's (B=64, H=4, head_dim 64, padded to 128 columns) under a
    2-D band mask plus a key-padding mask with holes: the masked 128-column kernels (ops.self_attention / ops.cross_attention
    with `dead` / `add_mask`) against ops.masked_attention on the same masks, interleaved the same way."""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from transformertts_amd import ops
dev = torch.device("cuda:0")


def ev():
    return torch.cuda.Event(enable_timing=True)


def run_wide(name, B, H, hd, Tq, Tk, causal, need_w, p=0.1, rounds=5, reps=4, masked=False):
    """kernels against the torch route, alternating (A B A B ...): min and median of forward + backward, peak bytes above what
    was live before the call.  `masked`: a band of half-width Tk / 8 along the diagonal as a shared (Tq, Tk) float mask (the
    band's scores get a random bias) and 10 % dead keys"""
    d = H * hd
    torch.manual_seed(0)
    lens = torch.full((B,), Tk, dtype=torch.int64, device=dev)
    dead = add = add_finite = None
    if masked:
        dead = torch.rand(B, Tk, device=dev) < 0.1
        off = (torch.arange(Tq, device=dev)[:, None] * Tk // Tq - torch.arange(Tk, device=dev)[None, :]).abs()
        add = ops.pad_mask_rows(torch.randn(Tq, Tk, device=dev).masked_fill(off > max(Tk // 8, 1), float("-inf")))
        add_finite = add.clamp_min(torch.finfo(torch.float32).min)[None, None]
    q = torch.randn(B, Tq, 3 * d if Tq == Tk else d, device=dev, requires_grad=True)
    kv = None if Tq == Tk else torch.randn(B, Tk, 2 * d, device=dev, requires_grad=True)
    do = torch.randn(B, Tq, d, device=dev)

    def kernels():
        if kv is None:
            return ops.self_attention(q, lens, H, bool(causal), p, 7, dead=dead, add_mask=add)
        return ops.cross_attention(q, kv, lens, H, p, 7, need_w, dead=dead, add_mask=add)[0]

    def torch_route():
        if kv is None:
            return ops.masked_attention(q[..., :d], q[..., d:2 * d], q[..., 2 * d:], lens, H, bool(causal), p, dead, add_finite)[0]
        return ops.masked_attention(q, kv[..., :d], kv[..., d:], lens, H, False, p, dead, add_finite)[0]

    times, peak = {"kernels": [], "torch": []}, {}
    for rnd in range(rounds + 1):                 # round 0 warms both up
        for tag, fn in (("kernels", kernels), ("torch", torch_route)):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            for _ in range(reps):
                e0, e1 = ev(), ev()
                e0.record()
                fn().backward(do)
                e1.record()
                torch.cuda.synchronize()
                if rnd > 0:
                    times[tag].append(e0.elapsed_time(e1) * 1e3)
            peak[tag] = torch.cuda.max_memory_allocated() - base
            q.grad = None
            if kv is not None:
                kv.grad = None
    for tag in ("kernels", "torch"):
        t = sorted(times[tag])
        print(f"{name:12s} hd {hd} {tag:8s} fwd+bwd min {t[0]:8.1f} us  median {t[len(t) // 2]:8.1f} us   peak {peak[tag] / 2**20:8.1f} MiB",
              flush=True)


def run(name, B, H, Tq, Tk, causal, p=0.1, reps=8):
    d = H * 64
    torch.manual_seed(0)
    lens = torch.full((B,), Tk, dtype=torch.int64, device=dev)
    if Tq == Tk:
        x = torch.randn(B, Tq, 3 * d, device=dev, requires_grad=True)
        x._ttts_amax = None
        fwd = lambda: ops.self_attention(x, lens, H, bool(causal), p, 7)
    else:
        q = torch.randn(B, Tq, d, device=dev, requires_grad=True)
        kv = torch.randn(B, Tk, 2 * d, device=dev, requires_grad=True)
        fwd = lambda: ops.cross_attention(q, kv, lens, H, p, 7, False)[0]
    do = torch.randn(B, Tq, d, device=dev)
    tf, tb = [], []
    for i in range(reps + 2):
        e0, e1, e2 = ev(), ev(), ev()
        e0.record()
        o = fwd()
        e1.record()
        o.backward(do)
        e2.record()
        torch.cuda.synchronize()
        if i >= 2:
            tf.append(e0.elapsed_time(e1) * 1e3); tb.append(e1.elapsed_time(e2) * 1e3)
    # fp64 check of the forward without dropout on a few batch entries
    if Tq == Tk:
        with torch.no_grad():
            o0 = ops.self_attention(x.detach(), lens, H, bool(causal), 0.0, 0)
            xb = x.detach()[:2].double().view(2, Tq, 3, H, 64)
            qq, kk, vv = (xb[:, :, i].transpose(1, 2) for i in range(3))
            s = qq @ kk.transpose(-1, -2) / 8.0
            if causal:
                s = s + torch.full((Tq, Tq), float("-inf"), device=dev, dtype=torch.float64).triu(1)
            ref = (torch.softmax(s, -1) @ vv).transpose(1, 2).reshape(2, Tq, d)
            err = float((o0[:2].double() - ref).norm() / ref.norm())
    else:
        err = float("nan")
    print(f"{name:10s} fwd {min(tf):7.1f} us  bwd {min(tb):7.1f} us   fwd rel err vs fp64 {err:.1e}", flush=True)


ap = argparse.ArgumentParser()
ap.add_argument("--head-dim", type=int, default=64)
ap.add_argument("--masked", action="store_true")
args = ap.parse_args()
if args.masked:
    for B, H, hd in ((8, 8, 128), (64, 4, 64)):
        run_wide("causal self", B, H, hd, 870, 870, 1, False, masked=True)
        run_wide("self", B, H, hd, 100, 100, 0, False, masked=True)
        run_wide("cross+weights", B, H, hd, 870, 100, 0, True, masked=True)
elif args.head_dim > 64:
    run_wide("causal self", 8, 8, args.head_dim, 870, 870, 1, False)
    run_wide("self", 8, 8, args.head_dim, 100, 100, 0, False)
    run_wide("cross+weights", 8, 8, args.head_dim, 870, 100, 0, True)
else:
    run("dec self", 64, 4, 870, 870, 1)
    run("enc self", 64, 4, 100, 100, 0)
    run("cross", 64, 4, 870, 100, 0)
