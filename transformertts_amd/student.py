"""Training a FastSpeech-2-style student: the masked mel loss on the kernels of csrc/student_loss.hip (`mel_loss`),
the loss module that ties it to `VarianceLoss` (`FastSpeech2Loss`), one eager optimizer step of `FastSpeech2Student` on `FlatAdam`
(`StudentTrainStep`) and the call that turns a teacher batch into the student's targets (`distillation_targets`).  Every sum is
taken in a fixed order, so the same inputs give the same bits on every call; a step reads nothing back to the host once its first
call has built the lazy caches.  There is no CPU fallback."""
from __future__ import annotations

import math

import torch
from torch import nn

from .variance import VarianceLoss, _lens

MAX_FRAMES = 1 << 20         # ML_MAX_T of csrc/student_loss.hip
MAX_MELS = 4096              # ML_MAX_M
BATCH_KEYS = ("phoneme", "phoneme_lens", "melspec", "melspec_lens", "durations", "pitch", "energy")

__all__ = ["mel_loss", "FastSpeech2Loss", "StudentTrainStep", "distillation_targets"]


# ------------------------------------------------------------------------------------------------ checks
def _mels(x, fn, name):
    """(B, T, M) fp32 on the device, handed on through its strides when they allow float4 rows (the rule of `variance._rows`)
    -> x, ld_row, ld_batch"""
    if x.dim() != 3 or min(x.shape) < 1:
        raise ValueError(f"{fn}: {name} must be (B, T, M), got {tuple(x.shape)}")
    if not x.is_cuda:
        raise ValueError(f"{fn}.{name}: expected a CUDA/HIP tensor (the HIP path has no CPU fallback), got {x.device}")
    if x.dtype != torch.float32:
        raise ValueError(f"{fn}.{name}: expected dtype {torch.float32}, got {x.dtype}")
    B, T, M = x.shape
    if M % 4 != 0 or M > MAX_MELS:
        raise ValueError(f"{fn}: M must be a multiple of 4 in [4, {MAX_MELS}], got {M} ({name})")
    if T > MAX_FRAMES:
        raise ValueError(f"{fn}: {name} must hold [1, 2^20] frames, got {T}")
    if B > 65535:
        raise ValueError(f"{fn}: B must be in [1, 65535], got {B}")
    ok = x.stride(2) == 1 and x.data_ptr() % 16 == 0
    ok = ok and (T == 1 or (x.stride(1) >= M and x.stride(1) % 4 == 0))
    ld_row = x.stride(1) if T > 1 else M
    ok = ok and (B == 1 or (x.stride(0) % 4 == 0 and x.stride(0) >= (T - 1) * ld_row + M))
    if not ok:
        x = x.contiguous()
        ld_row = M
    return x, ld_row, (x.stride(0) if B > 1 else T * ld_row)


def _target_like(target, B, M, fn):
    if target.dim() != 3 or target.size(0) != B or target.size(2) != M:
        raise ValueError(f"{fn}: target must be ({B}, Tt, {M}) like pred, got {tuple(target.shape)}")
    return target


def _extra(extra, device, fn):
    """None, or one fp32 value on the device -> None or a 0-dim tensor (its place in the autograd graph kept)"""
    if extra is None:
        return None
    if not isinstance(extra, torch.Tensor) or extra.numel() != 1 or extra.dtype != torch.float32 or extra.device != torch.device(device):
        what = type(extra).__name__ if not isinstance(extra, torch.Tensor) else f"{tuple(extra.shape)} {extra.dtype} on {extra.device}"
        raise ValueError(f"{fn}: extra must be one {torch.float32} value on {device} (no CPU fallback), got {what}")
    return extra.reshape(())


def _two_weights(weights, fn):
    try:
        weights = tuple(float(w) for w in weights)
    except TypeError:
        weights = ()
    if len(weights) != 2 or not all(math.isfinite(w) for w in weights):
        raise ValueError(f"{fn}: weights must be two finite numbers (mae, mse), got {weights}")
    return weights


# ------------------------------------------------------------------------------------------------ the mel loss
class _MelLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, ld_p, target, ld_t, pred_lens, target_lens, weights, extra):
        from . import _lib
        from .ops import _p, _stream
        lib = _lib.load()
        B, T, M = pred.shape
        Tt = target.size(1)
        out = torch.empty(4, dtype=torch.float32, device=pred.device)
        frames = torch.empty(1, dtype=torch.int64, device=pred.device)
        nbytes = lib.ttts_mel_loss_workspace_bytes(B, T, Tt, M)
        ws = torch.empty(max(nbytes // 4, 4), dtype=torch.float32, device=pred.device)
        _lib.check(lib.ttts_mel_loss_fwd(_p(pred), *ld_p, _p(target), *ld_t, _p(pred_lens), _p(target_lens), B, T, Tt, M, *weights,
                                         _p(extra), _p(out), _p(frames), _p(ws), nbytes, _stream()), "ttts_mel_loss_fwd")
        ctx.save_for_backward(pred, target, pred_lens, target_lens)
        ctx.geometry = (ld_p, ld_t, weights)
        ctx.set_materialize_grads(False)                  # an output nobody differentiates hands the kernel a NULL, not a zero
        frames = frames[0]
        ctx.mark_non_differentiable(frames)
        return out[0], out[1], out[2], out[3], frames

    @staticmethod
    def backward(ctx, g_mae, g_mse, g_mel, g_total, _frames):
        from . import _lib
        from .ops import _p, _stream
        pred, target, pred_lens, target_lens = ctx.saved_tensors
        ld_p, ld_t, weights = ctx.geometry
        B, T, M = pred.shape
        dpred = None
        if ctx.needs_input_grad[0]:
            gs = [None if g is None else g.to(torch.float32).contiguous() for g in (g_mae, g_mse, g_mel, g_total)]
            dpred = torch.empty(B, T, M, dtype=torch.float32, device=pred.device)
            _lib.check(_lib.load().ttts_mel_loss_bwd(_p(pred), *ld_p, _p(target), *ld_t, _p(pred_lens), _p(target_lens), B, T,
                                                     target.size(1), M, *weights, *[_p(g) for g in gs], _p(dpred), _stream()),
                       "ttts_mel_loss_bwd")
        return dpred, None, None, None, None, None, None, (g_total if ctx.needs_input_grad[7] else None)


def mel_loss(pred, pred_lens, target, target_lens, weights=(1.0, 0.0), extra=None):
    """The masked mean absolute and mean squared error between two ragged mel batches (csrc/student_loss.hip: two launches
    forward, one backward).  pred (B, T, M) and target (B, Tt, M) fp32, M a multiple of 4, Tt need not be T; strided views go
    through their strides, a view that breaks the float4-row rule is made contiguous.  pred_lens, target_lens (B,) integers.  Frame
    t of utterance b counts for t < n_b = min(pred_lens[b], target_lens[b]) clipped to [0, min(T, Tt)]; nothing at or behind
    n_b is read in either operand.  weights = (w_mae, w_mse); extra: an optional device scalar added to the total (the variance
    loss's total, so the student's total leaves the kernel).
    -> {'mae', 'mse', 'mel' = w_mae mae + w_mse mse, 'total' = mel + extra, 'frames' = sum n_b (int64)}, all 0-dim device
    tensors, the four losses exactly 0 when frames is 0.  The gradient reaches pred (exact zeros at and behind n_b) and extra."""
    fn = "mel_loss"
    pred, ldr_p, ldb_p = _mels(pred, fn, "pred")
    B, T, M = pred.shape
    target, ldr_t, ldb_t = _mels(_target_like(target, B, M, fn).detach(), fn, "target")
    if target.device != pred.device:
        raise ValueError(f"{fn}: pred and target must share a device, got {pred.device} and {target.device}")
    weights = _two_weights(weights, fn)
    pl = _lens(pred_lens, B, fn, "pred_lens", pred.device)
    tl = _lens(target_lens, B, fn, "target_lens", pred.device)
    extra = _extra(extra, pred.device, fn)
    mae, mse, mel, total, frames = _MelLoss.apply(pred, (ldr_p, ldb_p), target, (ldr_t, ldb_t), pl, tl, weights, extra)
    return {"mae": mae, "mse": mse, "mel": mel, "total": total, "frames": frames}


class FastSpeech2Loss(nn.Module):
    """The student's training loss: `VarianceLoss` (unchanged) on the adaptor's three predictions, and `mel_loss` between
    out['melspec'] under out['mel_lens'] and the target mel under melspec_lens, which takes the variance total as its `extra`: the
    sum of the two leaves the kernel, and no 0-dim torch arithmetic sits between the losses and `backward`.
    forward(out, melspec, melspec_lens, durations, pitch, energy, phoneme_lens), `out` what `FastSpeech2Student` returns
    -> {'total', 'mel', 'mae', 'mse', 'duration', 'pitch', 'energy', 'frames'}."""

    def __init__(self, mel_weights=(1.0, 0.0), variance_weights=(1.0, 1.0, 1.0)):
        super().__init__()
        self.mel_weights = _two_weights(mel_weights, "FastSpeech2Loss")
        self.variance = VarianceLoss(variance_weights)

    def forward(self, out, melspec, melspec_lens, durations, pitch, energy, phoneme_lens):
        var = self.variance(out, durations, pitch, energy, phoneme_lens)
        mel = mel_loss(out["melspec"], out["mel_lens"], melspec, melspec_lens, self.mel_weights, extra=var["total"])
        return {"total": mel["total"], "mel": mel["mel"], "mae": mel["mae"], "mse": mel["mse"], "duration": var["duration"],
                "pitch": var["pitch"], "energy": var["energy"], "frames": mel["frames"]}


# ------------------------------------------------------------------------------------------------ one training step
def _check_batch(batch, device):
    missing = [k for k in BATCH_KEYS if k not in batch]
    if missing:
        raise KeyError(f"StudentTrainStep: the batch lacks {', '.join(repr(k) for k in missing)} (it needs {', '.join(BATCH_KEYS)})")
    for k in BATCH_KEYS:
        if batch[k].device != device:
            raise ValueError(f"StudentTrainStep: batch[{k!r}] must live on the student's HIP device {device} (no CPU fallback), "
                             f"got {batch[k].device}")


class StudentTrainStep:
    """One eager micro-batch of the student per call, the optimizer (and the scheduler) stepping on every `accumulate`-th: the
    eager branch of `step.TrainStep` around `FastSpeech2Student` and `FastSpeech2Loss`.

        opt = FlatAdam(student.parameters(), lr=1.0, max_grad_norm=1.0)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, noam_lambda(d_model, warmup))
        step = StudentTrainStep(student, opt, sched, seed=0)
        losses = step(batch)      # phoneme, phoneme_lens, melspec, melspec_lens, durations, pitch, energy: device tensors

    The state block carries the step's seed word (`_step_seed(seed, index)`: dropout is fresh every micro-batch and the same
    for the same seed), the learning rate and the Adam step count; the dropout site seeds are numbered from zero per micro-batch.
    The student is called with max_len = melspec.size(1), so the durations are never read back.  `index` counts micro-batches,
    `micro` the position inside the accumulation window; each micro-batch's gradient is scaled by 1 / accumulate.
    -> the loss dict of `FastSpeech2Loss`, detached; every value a device tensor."""

    def __init__(self, student, optimizer, scheduler=None, loss=None, *, seed=0, accumulate=1):
        from . import ops
        from .optim import FlatAdam
        if not isinstance(optimizer, FlatAdam):
            raise TypeError("StudentTrainStep drives FlatAdam (flat parameter / gradient / moment buffers)")
        self.student, self.opt, self.sched = student, optimizer, scheduler
        self.loss = FastSpeech2Loss() if loss is None else loss
        self.bucket = optimizer.bucket
        self.device = self.bucket.flat.device
        self.state = ops.StepState(self.device)
        self.accumulate = max(1, int(accumulate))
        self._grad_seed = torch.full((), 1.0 / self.accumulate, dtype=torch.float32, device=self.device)   # resident d(loss)
        self.base_seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.index = 0                       # micro-batches taken
        self.micro = 0                       # position inside the accumulation window

    def __call__(self, batch):
        from . import ops
        from .step import _step_seed
        _check_batch(batch, self.device)
        dev = self.device
        first, last = self.micro == 0, self.micro == self.accumulate - 1
        ops.seeds.ensure_seeded()
        self.state.push(seed=_step_seed(self.base_seed, self.index), lr=float(self.opt.param_groups[0]["lr"]), p_tf=0.0,
                        step=self.opt._step + 1)
        with self.state:
            ops.seeds.counter = 0                # site seeds are numbered per micro-batch; the seed word makes them fresh
            ops.amax_arena_reset(dev)
            try:
                if first:
                    self.opt.zero_grad()
                out = self.student(batch["phoneme"], batch["phoneme_lens"], batch["durations"], batch["pitch"], batch["energy"],
                                   max_len=batch["melspec"].size(1))
                losses = self.loss(out, batch["melspec"], batch["melspec_lens"], batch["durations"], batch["pitch"],
                                   batch["energy"], batch["phoneme_lens"])
                losses["total"].backward(gradient=self._grad_seed)
                self.bucket.flush_reductions()
            finally:
                ops.amax_arena_release(dev)
            if last:
                self.opt.step()
        if last and self.sched is not None:
            self.sched.step()
        self.index += 1
        self.micro = 0 if last else self.micro + 1
        return {k: v.detach() for k, v in losses.items()}


# ------------------------------------------------------------------------------------------------ targets from a teacher
def distillation_targets(teacher, phoneme, melspec, phoneme_lens, melspec_lens, wave, wave_lens, pitch_energy, **kw):
    """A teacher batch -> the student's targets: `teacher_durations(teacher, phoneme, melspec, phoneme_lens, melspec_lens, **kw)`,
    `pitch_energy(wave, wave_lens)` (a `PitchEnergy`), then `phoneme_average` of the F0 over the voiced frames and of the frame
    energy, both under frames = min(the front end's frame count, melspec_lens) element by element.
    -> {'durations' (B, Pmax) int64, 'pitch', 'energy' (B, Pmax) fp32, 'valid' (B,) bool, 'focus_rate'}.  Where `valid`, the
    durations of an utterance sum to its melspec_lens.  NO normalisation is done here: pitch is in Hz (0 for a phoneme without a
    voiced frame) and energy is the STFT frame norm, as the kernels give them; scale them to your data's statistics (and choose
    `variance_bins` to match) before they reach the student."""
    from .alignment import teacher_durations
    from .audio import phoneme_average
    d = teacher_durations(teacher, phoneme, melspec, phoneme_lens, melspec_lens, **kw)
    pe = pitch_energy(wave, wave_lens)
    frames = torch.minimum(pe["frames"], melspec_lens.to(pe["frames"].device).to(torch.int64))
    pitch = phoneme_average(pe["f0"], d["durations"], phoneme_lens, frames, mask=pe["voiced"])["mean"]
    energy = phoneme_average(pe["energy"], d["durations"], phoneme_lens, frames)["mean"]
    return {"durations": d["durations"], "pitch": pitch, "energy": energy, "valid": d["valid"], "focus_rate": d["focus_rate"]}
