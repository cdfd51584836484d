#!/usr/bin/env python3
"""What training the FastSpeech-2 student costs on the library's kernels, each cell against its stock-torch
restatement, both sides alternating round by round in one process.

    python tools/student_step_bench.py [--rounds 5] [--reps 10] [--out profiles/student_step_bench.txt] [--label TEXT]

Group 1, `mel_loss` of csrc/student_loss.hip forward and forward + backward against the `where` / `abs` / `sum` / `div`
restatement (tests/student_reference.py `mel_loss_stock`), weights (1, 1) so that both sums are wanted: 64 x 870 x 80 dense, 1 x 870
x 80, and 64 utterances of 95 .. 870 frames.  Group 2, one `StudentTrainStep` of the default student (d_model 256, 4 + 4 layers,
hidden 1024, 80 mels, dropout 0.2) on 64 utterances of 110 phonemes whose durations (1 .. 15 frames) land near 870 frames, against
the same student in stock torch: tests/fft_reference.py `student_ref` in fp32 (dropout off: it has none), the restated losses,
`clip_grad_norm_` and `torch.optim.Adam`.  Times: device events around `reps` calls after a warm-up, the median and minimum over
the rounds, in microseconds, every call issued from Python.  No ratio is promised: every cell is printed, `slower_than_stock`
lists the cells whose median is above stock's.  Prints one JSON line per shape and appends it to `--out`."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

M = 80
LOSS_SHAPES = [("mel_64x870x80", 64, 870, False), ("mel_1x870x80", 1, 870, False), ("mel_64x95..870x80", 64, 870, True)]
STUDENT = dict(n_vocab=64, d_model=256, encoder_layers=4, decoder_layers=4, n_head=2, d_hidden=1024, n_mels=M)
STEP_SHAPE = ("step_64x110", 64, 110, 15)                             # name, B, phonemes, longest duration
MEL_W, VAR_W = (1.0, 1.0), (1.0, 1.0, 1.0)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def measure(cells, rounds, reps):
    times = {}
    for _ in range(rounds):                                           # the two sides alternate inside every round
        for cell, pair in cells.items():
            for side, fn in zip(("kernel", "stock"), pair):
                fn()
                times.setdefault((cell, side), []).append(timed(fn, reps))
    return times


def emit(row, cells, times, args):
    row.update({"label": args.label, "rounds": args.rounds, "reps": args.reps, "device": torch.cuda.get_device_name(0)})
    for (cell, side), v in times.items():
        row[f"{cell}.{side}.us"] = [round(statistics.median(v), 2), round(min(v), 2)]
    row["slower_than_stock"] = [c for c in cells if statistics.median(times[(c, "kernel")]) > statistics.median(times[(c, "stock")])]
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


def stock_variance(out, dur, pitch, energy, valid):
    dt = out["melspec"].dtype
    zero, n = out["melspec"].new_zeros(()), valid.sum().to(dt)
    terms = [(torch.where(valid, out[k] - t, zero) ** 2).sum() / n
             for k, t in (("log_duration", torch.log(dur.to(dt) + 1)), ("pitch", pitch), ("energy", energy))]
    return (VAR_W[0] * terms[0] + VAR_W[1] * terms[1]) + VAR_W[2] * terms[2]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    from fft_reference import student_ref
    from student_reference import mel_loss_stock
    from transformertts_amd import FastSpeech2Loss, FastSpeech2Student, StudentTrainStep, mel_loss, synth_student_batch
    from transformertts_amd.optim import FlatAdam
    dev = "cuda:0"
    torch.manual_seed(0)

    # ---- group 1: the loss alone
    for name, B, T, ragged in LOSS_SHAPES:
        gen = torch.Generator().manual_seed(11 + B + ragged)
        lens_host = [int(round(95 + (T - 95) * b / max(1, B - 1))) for b in range(B)] if ragged else [T] * B
        lens = torch.tensor(lens_host, device=dev)
        pred, target = torch.randn(B, T, M, generator=gen).to(dev), torch.randn(B, T, M, generator=gen).to(dev)
        pg = pred.clone().requires_grad_(True)

        def k_fwd():
            with torch.no_grad():
                mel_loss(pred, lens, target, lens, MEL_W)

        def s_fwd():
            with torch.no_grad():
                mel_loss_stock(pred, lens, target, lens, MEL_W)
        cells = {"loss_fwd": (k_fwd, s_fwd),
                 "loss_fwd+bwd": (lambda: mel_loss(pg, lens, target, lens, MEL_W)["total"].backward(),
                                  lambda: mel_loss_stock(pg, lens, target, lens, MEL_W)["total"].backward())}
        times = measure(cells, args.rounds, args.reps)
        emit({"tool": "student_step_bench", "shape": name, "B": B, "frames": T, "valid_frames": sum(lens_host), "n_mels": M,
              "bytes_read": 2 * sum(lens_host) * M * 4}, cells, times, args)

    # ---- group 2: one training step of the default student
    name, B, P, longest = STEP_SHAPE
    host = synth_student_batch(B, P, n_mels=M, n_vocab=STUDENT["n_vocab"], max_duration=longest, ragged=False, seed=3)
    batch = {k: v.to(dev) for k, v in host.items()}
    T = batch["melspec"].size(1)
    student = FastSpeech2Student(**STUDENT, dropout=0.2).to(dev).train()
    sd = {k: v.detach().clone() for k, v in student.state_dict().items()}
    opt = FlatAdam(student.parameters(), lr=1e-3, max_grad_norm=1.0)
    step = StudentTrainStep(student, opt, None, FastSpeech2Loss(MEL_W, VAR_W), seed=0)
    names = [k for k, _ in student.named_parameters()]
    p = {k: v.clone() for k, v in sd.items()}
    for k in names:
        p[k].requires_grad_(True)
    leaves = [p[k] for k in names]
    s_opt = torch.optim.Adam(leaves, lr=1e-3, betas=(0.9, 0.98), eps=1e-9)
    valid = torch.arange(P, device=dev)[None, :] < batch["phoneme_lens"][:, None]
    lens_host = host["phoneme_lens"].tolist()

    def stock_step():
        s_opt.zero_grad(set_to_none=False)
        out = student_ref(p, STUDENT, batch["phoneme"], lens_host, batch["durations"], batch["pitch"], batch["energy"], T)
        var = stock_variance(out, batch["durations"], batch["pitch"], batch["energy"], valid)
        mel_loss_stock(out["melspec"], out["mel_lens"], batch["melspec"], batch["melspec_lens"], MEL_W, var)["total"].backward()
        torch.nn.utils.clip_grad_norm_(leaves, 1.0)
        s_opt.step()
    cells = {"train_step": (lambda: step(batch), stock_step)}
    times = measure(cells, args.rounds, max(1, args.reps // 2))
    emit({"tool": "student_step_bench", "shape": name, "B": B, "phonemes": P, "frames": T, "valid_frames": int(host["melspec_lens"].sum()),
          "parameters": int(opt.bucket.flat.numel()), "dropout": 0.2, "stock_dropout": 0.0, **{k: v for k, v in STUDENT.items()}},
         cells, times, args)


if __name__ == "__main__":
    main()
