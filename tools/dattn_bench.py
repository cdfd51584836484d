#!/usr/bin/env python3
"""What differentiable alignment maps cost: one process, the variants alternating round by round.

    python tools/dattn_bench.py --attn            one decoder cross-attention block (MultiheadAttention.cross_attention: q and
                                                  k | v projections, attention with weights, out-projection), B 64, H 4,
                                                  Tq 870, Tk 160, head_dim 64: forward + backward and the backward alone of
                                                    image      today's route (head images, ttts_attention_bwd_img)
                                                    wide       weights_grad=True, gradient on the context only
                                                               (fp32 projections, ttts_attention_bwd_wide on heads padded to 128)
                                                    wide+dA    weights_grad=True, gradients on the context and on the weights
                                                               (ttts_attention_bwd_wide_dattn)
    python tools/dattn_bench.py --step [--batch N]  the whole training step (TrainStep, captured graph, base model, dropout on)
                                                  without and with config['training']['guided_attention']

Prints min / median in microseconds (--attn) or milliseconds per step (--step)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def attn(args):
    from transformertts_amd import ops
    from transformertts_amd.model.layers import MultiheadAttention
    dev = torch.device("cuda:0")
    B, H, Tq, Tk, hd = args.batch or 64, 4, 870, 160, 64
    d = H * hd
    torch.manual_seed(1)
    mha = MultiheadAttention(d, H, dropout=0.1).to(dev).train()
    x = torch.randn(B, Tq, d, device=dev, requires_grad=True)
    mem = torch.randn(B, Tk, d, device=dev, requires_grad=True)
    lens = torch.full((B,), Tk, dtype=torch.int64, device=dev)
    do = torch.randn(B, Tq, d, device=dev)
    G = ops.pad_mask_rows(torch.randn(B, Tq, Tk, device=dev))[:, None].expand(B, H, Tq, Tk)     # what the guided loss hands back

    def variant(name):
        kw = {} if name == "image" else dict(weights_grad=True)

        def fwd():
            return mha.cross_attention(x, mem, lens, residual=x, out_drop=0.0, need_weights=True, **kw)

        def bwd(out):
            y, w = out
            if name == "wide+dA":
                torch.autograd.backward([y, w], [do, G])
            else:
                y.backward(do)
        return fwd, bwd

    names = ("image", "wide", "wide+dA")
    both, back = {n: [] for n in names}, {n: [] for n in names}
    for rnd in range(args.rounds + 1):
        for n in names:
            fwd, bwd = variant(n)
            t_both = timed(lambda: bwd(fwd()), args.reps)
            outs = [fwd() for _ in range(args.reps)]
            it = iter(outs)
            t_back = timed(lambda: bwd(next(it)), args.reps)
            if rnd:                      # round 0 warms up
                both[n].append(t_both * 1e3)
                back[n].append(t_back * 1e3)
    print(f"# cross-attention block B {B} H {H} Tq {Tq} Tk {Tk} head_dim {hd}, dropout 0.1, {args.rounds} rounds x {args.reps} reps, us")
    print("# variant   forward+backward min / median   backward min / median")
    for n in names:
        print(f"{n:9s} {min(both[n]):9.0f} / {statistics.median(both[n]):9.0f}   {min(back[n]):9.0f} / {statistics.median(back[n]):9.0f}")


def step(args):
    from transformertts_amd.lightning_module import LightningModule
    from transformertts_amd.step import TrainStep
    from transformertts_amd.workload import model_config, synth_batch
    B = args.batch or 64
    cfg = model_config("base")
    runs = {}
    for name, ga in (("off", None), ("on", {"weight": 1.0, "sigma": 0.4})):
        training = {"num_epochs": 300, "teacher_forcing_mode": "linear", "warmup_steps": 4000, "sync_loss_every_step": False,
                    "fused_clip_norm": 1.0}
        if ga is not None:
            training["guided_attention"] = ga
        torch.manual_seed(1234)
        lm = LightningModule({"model": dict(cfg, device="cuda"), "loss": {"stop_weight": 8.0}, "training": training}).to("cuda").train()
        oc = lm.configure_optimizers()
        batch = {k: v.to("cuda") for k, v in synth_batch(B, 100, 870, cfg["n_mels"], cfg["n_phon"], seed=1234).items()}
        ts = TrainStep(lm, oc["optimizer"], oc["lr_scheduler"]["scheduler"], batch, graph=True, seed=77)
        for _ in range(4):
            ts()
        torch.cuda.synchronize()
        assert ts.graphed
        runs[name] = ts
    times = {n: [] for n in runs}
    for _ in range(args.rounds):
        for n, ts in runs.items():
            times[n].append(timed(ts, args.reps))
    print(f"# training step, base model, B {B}, Tp 100, Tm 870, captured graph, {args.rounds} rounds x {args.reps} steps alternating, ms/step")
    for n in runs:
        print(f"guided attention {n:3s}  min {min(times[n]):8.3f}  median {statistics.median(times[n]):8.3f}")
    print(f"on / off (medians): {statistics.median(times['on']) / statistics.median(times['off']):.3f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--attn", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4)
    a = ap.parse_args()
    if a.attn:
        attn(a)
    if a.step:
        step(a)
