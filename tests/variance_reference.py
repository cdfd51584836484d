"""Oracles of the variance adaptor (csrc/variance.hip, transformertts_amd/variance.py), written from the definitions of DESIGN.md
26 in numpy: fp64 oracles (`*_ref`) and the stock fp32 forms in the kernels' stated order (`*_stock`), which the kernels must
meet bit for bit.  No torch, no device."""
import numpy as np

LOSS_THREADS = 1024          # the loss kernel's workgroup: thread i adds the flat elements i, i + 1024, ...
DUR_MAX = 2 ** 31 - 1
HUGE = np.int64(0x7FF8000000000000)      # a NaN's bit pattern as an int64: what the tests put behind the lengths of durations


def spans_ref(durations, phoneme_lens, Tmax):
    """per utterance: (c_p, min(c_p + dur'_p, frames_b)) clipped to frames_b for every p < Pmax, and frames_b"""
    B, Pmax = durations.shape
    a, e, frames = np.zeros((B, Pmax), np.int64), np.zeros((B, Pmax), np.int64), np.zeros(B, np.int64)
    for b in range(B):
        pl = min(max(int(phoneme_lens[b]), 0), Pmax)
        c = 0
        for p in range(Pmax):
            d = max(int(durations[b, p]), 0) if p < pl else 0
            a[b, p], e[b, p] = min(c, Tmax), min(c + d, Tmax)
            c += d
        frames[b] = min(c, Tmax)
    return a, e, frames


def length_regulate_ref(x, durations, phoneme_lens, Tmax):
    """y (B, Tmax, D) in x's dtype (a copy has no rounding), mel_lens int64, index int32"""
    B, Pmax, D = x.shape
    a, e, frames = spans_ref(durations, phoneme_lens, Tmax)
    y = np.zeros((B, Tmax, D), x.dtype)
    index = np.full((B, Tmax), -1, np.int32)
    for b in range(B):
        for p in range(Pmax):
            y[b, a[b, p]:e[b, p]] = x[b, p]
            index[b, a[b, p]:e[b, p]] = p
    return y, frames, index


def length_regulate_naive(x, durations, phoneme_lens, Tmax):
    """the usual repeat_interleave + pad loop"""
    B, Pmax, D = x.shape
    y = np.zeros((B, Tmax, D), x.dtype)
    for b in range(B):
        pl = int(phoneme_lens[b])
        rows = np.repeat(x[b, :pl], np.maximum(durations[b, :pl], 0), axis=0)[:Tmax]
        y[b, :len(rows)] = rows
    return y


def length_regulate_transpose_ref(dy, durations, phoneme_lens, Pmax):
    """dx (B, Pmax, D) in fp64"""
    B, Tmax, D = dy.shape
    a, e, _ = spans_ref(durations, phoneme_lens, Tmax)
    dx = np.zeros((B, Pmax, D), np.float64)
    for b in range(B):
        for p in range(Pmax):
            dx[b, p] = dy[b, a[b, p]:e[b, p]].astype(np.float64).sum(axis=0)
    return dx


def length_regulate_bwd_stock(dy, durations, phoneme_lens, Pmax, into=None):
    """the kernel's order: one fp32 add per frame in ascending t from 0.f; `into`: dx = into + that sum"""
    B, Tmax, D = dy.shape
    a, e, _ = spans_ref(durations, phoneme_lens, Tmax)
    dx = np.zeros((B, Pmax, D), np.float32)
    for b in range(B):
        for p in range(Pmax):
            acc = np.zeros(D, np.float32)
            for t in range(a[b, p], e[b, p]):
                acc = acc + dy[b, t]
            dx[b, p] = acc
    return dx if into is None else into + dx


def round_half_even_ref(v):
    return np.rint(np.asarray(v, np.float64))


def durations_from_log_ref(log_d, phoneme_lens, alpha=1.0, min_duration=0):
    """d = max(0, rint((exp(log_d) - 1) alpha)) in fp64, 0 for a NaN or infinite input, clamped to 2^31 - 1, at least min_duration
    for p < len, 0 behind it"""
    log_d = np.asarray(log_d)
    B, Pmax = log_d.shape
    out = np.zeros((B, Pmax), np.int64)
    for b in range(B):
        pl = min(max(int(phoneme_lens[b]), 0), Pmax)
        for p in range(pl):
            v = np.float64(log_d[b, p])
            d = 0
            if np.isfinite(v):
                with np.errstate(over="ignore"):
                    r = round_half_even_ref((np.exp(v) - 1.0) * np.float64(alpha))
                d = DUR_MAX if r >= DUR_MAX else 0 if r <= 0 else int(r)
            out[b, p] = max(d, int(min_duration))
    return out


def bucket_ref(values, bins):
    """the number of boundaries strictly below each value (torch.bucketize, right=False; a NaN counts none)"""
    return (np.asarray(bins)[None, :] < np.asarray(values).reshape(-1, 1)).sum(axis=1).reshape(np.shape(values)).astype(np.int64)


def variance_embed_ref(x, phoneme_lens, pitch=None, pitch_bins=None, Ep=None, energy=None, energy_bins=None, Ee=None, dtype=np.float64):
    """y = (x + Ep[i]) + Ee[j] for p < len, x behind it, and the ids (-1 behind it; None for an absent feature).  dtype float64:
    the oracle; float32: the stock form in the kernel's order."""
    B, Pmax, D = x.shape
    y = x.astype(dtype).copy()
    ids = []
    valid = np.arange(Pmax)[None, :] < np.clip(np.asarray(phoneme_lens), 0, Pmax)[:, None]
    for v, bins, table in ((pitch, pitch_bins, Ep), (energy, energy_bins, Ee)):
        if table is None:
            ids.append(None)
            continue
        i = np.where(valid, bucket_ref(np.where(valid, v, 0.0), bins), -1)
        y[valid] = y[valid] + table.astype(dtype)[i[valid]]
        ids.append(i)
    return y, ids[0], ids[1]


def embedding_bwd_ref(ids, dout, n):
    """fp64 table gradient: row v sums dout over the positions whose id is v"""
    flat, g = ids.reshape(-1), dout.reshape(ids.size, -1).astype(np.float64)
    return np.stack([g[flat == v].sum(axis=0) for v in range(n)])


def embedding_bwd_stock(ids, dout, n):
    """ttts_embedding_bwd's own order: the matching rows added one by one in ascending flat position, fp32 from 0.f"""
    flat, g = ids.reshape(-1), dout.reshape(ids.size, -1)
    out = np.zeros((n, g.shape[1]), np.float32)
    for k in range(flat.size):
        if 0 <= flat[k] < n:
            out[flat[k]] = out[flat[k]] + g[k]
    return out


def _targets(durations, valid):
    d = np.where(valid, np.maximum(durations, 0), 0).astype(np.float64)
    return np.log(d + 1.0)


def variance_loss_ref(log_d, durations, pitch_pred, pitch, energy_pred, energy, phoneme_lens, weights=(1.0, 1.0, 1.0)):
    """fp64: the three masked means and the weighted total"""
    B, Pmax = log_d.shape
    valid = np.arange(Pmax)[None, :] < np.clip(np.asarray(phoneme_lens), 0, Pmax)[:, None]
    n = int(valid.sum())
    if n == 0:
        return np.zeros(4)
    tgt = _targets(durations, valid).astype(np.float32)              # (the target is defined as the fp32 rounding of the fp64 log)
    L = [float((((p.astype(np.float64) - t.astype(np.float64)) ** 2)[valid]).sum() / n)
         for p, t in ((log_d, tgt), (pitch_pred, pitch), (energy_pred, energy))]
    return np.array(L + [weights[0] * L[0] + weights[1] * L[1] + weights[2] * L[2]])


def _diffs_stock(log_d, durations, pitch_pred, pitch, energy_pred, energy, valid):
    tgt = _targets(durations, valid).astype(np.float32)
    with np.errstate(invalid="ignore"):
        return [np.where(valid, p, 0).astype(np.float32) - np.where(valid, t, 0).astype(np.float32)
                for p, t in ((log_d, tgt), (pitch_pred, pitch), (energy_pred, energy))]


def variance_loss_stock(log_d, durations, pitch_pred, pitch, energy_pred, energy, phoneme_lens, weights=(1.0, 1.0, 1.0)):
    """fp32 in the kernel's order: thread i of 1024 adds the squares of the valid flat elements i, i + 1024, ... in ascending
    order; a wave's 64 lanes meet in the butterfly 32, 16, ... 1; the 16 wave sums are added in ascending order; / (float)n"""
    B, Pmax = log_d.shape
    valid = np.arange(Pmax)[None, :] < np.clip(np.asarray(phoneme_lens), 0, Pmax)[:, None]
    n = int(valid.sum())
    if n == 0:
        return np.zeros(4, np.float32)
    flat_valid = valid.reshape(-1)
    L = []
    for diff in _diffs_stock(log_d, durations, pitch_pred, pitch, energy_pred, energy, valid):
        sq = (diff * diff).reshape(-1)
        acc = np.zeros(LOSS_THREADS, np.float32)
        for base in range(0, sq.size, LOSS_THREADS):
            m = min(LOSS_THREADS, sq.size - base)
            chunk, ok = sq[base:base + m], flat_valid[base:base + m]
            acc[:m] = np.where(ok, acc[:m] + chunk, acc[:m])
        lanes = acc.reshape(LOSS_THREADS // 64, 64)
        for o in (32, 16, 8, 4, 2, 1):
            lanes = lanes[:, :o] + lanes[:, o:2 * o]
        s = np.float32(0)
        for w in range(LOSS_THREADS // 64):
            s = s + lanes[w, 0]
        L.append(s / np.float32(n))
    w = [np.float32(v) for v in weights]
    return np.array(L + [(w[0] * L[0] + w[1] * L[1]) + w[2] * L[2]], np.float32)


def variance_loss_grad_stock(log_d, durations, pitch_pred, pitch, energy_pred, energy, phoneme_lens, weights, gout):
    """fp32 in the kernel's order: s_k = (2 / (float)n) * (gout[k] + w_k * gout[3]); grad_k = s_k * (pred_k - target_k)"""
    B, Pmax = log_d.shape
    valid = np.arange(Pmax)[None, :] < np.clip(np.asarray(phoneme_lens), 0, Pmax)[:, None]
    n = int(valid.sum())
    if n == 0:
        return [np.zeros((B, Pmax), np.float32) for _ in range(3)]
    gout = np.asarray(gout, np.float32)
    two_n = np.float32(2) / np.float32(n)
    out = []
    for k, diff in enumerate(_diffs_stock(log_d, durations, pitch_pred, pitch, energy_pred, energy, valid)):
        s = two_n * (gout[k] + np.float32(weights[k]) * gout[3])
        out.append(np.where(valid, s * diff, np.float32(0)).astype(np.float32))
    return out


def variance_loss_grad_ref(log_d, durations, pitch_pred, pitch, energy_pred, energy, phoneme_lens, weights, gout):
    B, Pmax = log_d.shape
    valid = np.arange(Pmax)[None, :] < np.clip(np.asarray(phoneme_lens), 0, Pmax)[:, None]
    n = int(valid.sum())
    tgt = _targets(durations, valid).astype(np.float32)
    out = []
    for k, (p, t) in enumerate(((log_d, tgt), (pitch_pred, pitch), (energy_pred, energy))):
        coef = float(gout[k]) + float(weights[k]) * float(gout[3])
        diff = np.where(valid, p, 0).astype(np.float64) - np.where(valid, t, 0).astype(np.float64)
        out.append(np.where(valid, 2.0 * coef * diff / max(n, 1), 0.0))
    return out


# ------------------------------------------------------------------------------------------------ shared cases
def poison(rng, B, Pmax, D, lens):
    """a ragged batch with NaN in x and the targets, and a NaN's bits in the durations, behind every length"""
    x = rng.standard_normal((B, Pmax, D)).astype(np.float32)
    dur = rng.integers(0, 9, (B, Pmax)).astype(np.int64)
    pitch = rng.uniform(50.0, 650.0, (B, Pmax)).astype(np.float32)
    energy = rng.uniform(-0.2, 1.2, (B, Pmax)).astype(np.float32)
    for b, pl in enumerate(lens):
        x[b, pl:], dur[b, pl:], pitch[b, pl:], energy[b, pl:] = np.nan, HUGE, np.nan, np.nan
    return x, dur, pitch, energy
