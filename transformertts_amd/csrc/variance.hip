// Variance adaptor of a FastSpeech-2-style student (gfx950): the length regulator and its transpose, durations from predicted
// log-durations, the quantised pitch / energy embeddings and the three masked regression losses.
//   regulator   dur'_p = max(durations[b, p], 0) for p < pl_b = clamp(phoneme_lens[b], 0, Pmax), else 0; c the exclusive prefix
//               sum of dur'; frames_b = min(sum dur', Tmax); y[b, t, :] = x[b, p(t), :] for t < frames_b with c_p <= t < c_p +
//               dur'_p, exact zeros from frames_b on; index[b, t] = p(t) or -1; mel_lens[b] = frames_b.
//   transpose   dx[b, p, :] = the fp32 sum of dy[b, t, :] over t in [c_p, min(c_p + dur'_p, frames_b)) in ascending t, one plain
//               add per frame starting from 0.f; exact zeros for a phoneme without a frame and for p >= pl_b.
//   durations   d = rint((exp(log_d) - 1) alpha) evaluated in fp64 from the fp32 input (rint: half to even), clamped to
//               [0, 2^31 - 1]; 0 for a NaN or infinite log_d; then max(d, min_duration) for p < pl_b; 0 for p >= pl_b.
//   embedding   i = #{k : pitch_bins[k] < pitch[b, p]} (torch.bucketize, right=False; a NaN value gives 0), j alike for the energy;
//               y = (x + Ep[i]) + Ee[j] in that order for p < pl_b, y = x behind it; ids -1 behind it.
//   loss        three means of squared differences over the n = sum_b pl_b valid phonemes: prediction of the log-duration
//               against fp32(log_fp64(dur' + 1)), of the pitch and of the energy against their targets.  Thread i of one
//               workgroup of LOSS_THREADS threads adds the squares (a plain multiply, a plain add, from 0.f) of the flat
//               elements i, i + LOSS_THREADS, ... of (B, Pmax) in ascending order, skipping those behind a length; the 64 lanes
//               of a wave meet in a butterfly (lane l adds lane l ^ 32, then ^ 16, ... ^ 1); thread 0 adds the wave partials in
//               ascending wave order; term = sum / (float)n, 0 when n = 0; total = (w_d L_d + w_p L_p) + w_e L_e.
//   its grads   coef_k = gout[k] + w_k gout[3]; s_k = (2 / (float)n) coef_k; d pred = s_k (pred - target) for p < pl_b, exact
//               0 behind it (and everywhere when n = 0); every product and sum rounded on its own.
// Every kernel starts from the same scan: a workgroup takes the inclusive prefix sum of its utterance's dur' over tiles of 64
// phonemes (shuffle scan inside a tile, the tile totals scanned by wave 0), clamps it to Tmax (which changes no frame below
// Tmax) and keeps it in LDS as int32.  p(t) is the number of entries <= t: a bisection.  Integer sums: the order is free.
// No atomics, no allocation, no host read; nothing at or behind a length is read, except x rows the embedding passes through.
#include "ttts_common.h"

#include <math.h>

namespace ttts {

constexpr int VAR_THREADS = 256;
constexpr int VAR_WAVES = VAR_THREADS / 64;
constexpr int VAR_MAX_P = 4096;            // phonemes of an utterance: the prefix sums of one fit 16 KB of LDS
constexpr int VAR_MAX_T = 1 << 20;
constexpr int VAR_MAX_D = 4096;
constexpr int VAR_MAX_BINS = 4096;         // embedding rows per feature: Np - 1 boundaries in LDS
#ifndef TTTS_LR_FRAMES
#define TTTS_LR_FRAMES 32                  // frames a workgroup of the regulator's forward owns
#endif
constexpr int LR_FRAMES = TTTS_LR_FRAMES;
constexpr int VE_ROWS = 32;                // phoneme rows a workgroup of the embedding owns
constexpr int LOSS_THREADS = 1024;
constexpr int64_t DUR_MAX = 2147483647;
static_assert(LR_FRAMES >= 4 && LR_FRAMES <= VAR_THREADS && LR_FRAMES % 4 == 0, "four rows in flight per thread");

// lanes that share a row of d4 float4: the power of two at or above min(d4, 64), as a shift
static inline int lanes_log2(int d4) {
    int s = 0;
    while ((1 << s) < d4 && s < 6) ++s;
    return s;
}

// cs[p] = min(sum_{q <= p} dur'_q, Tmax) for p < n (n <= min(pl_b, Pmax)); all VAR_THREADS threads call it; ends on a barrier
__device__ __forceinline__ void scan_durations(const int64_t* __restrict__ dur_b, int n, int Tmax, int* __restrict__ cs,
                                               long* __restrict__ tile_off) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles = (n + 63) >> 6;
    for (int tile = wave; tile < tiles; tile += VAR_WAVES) {
        const int p = (tile << 6) + lane;
        long d = p < n ? dur_b[p] : 0;
        d = d < 0 ? 0 : d > Tmax ? Tmax : d;                                 // (a longer one is clipped to frames_b anyway)
        long s = d;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long u = __shfl_up(s, o, 64);
            s = lane >= o ? s + u : s;
        }
        if (p < n) cs[p] = (int)s;                                           // <= 64 Tmax = 2^26
        if (lane == 63) tile_off[tile] = s;
    }
    __syncthreads();
    if (wave == 0) {                                                         // exclusive scan of the (at most 64) tile totals
        const long v = lane < tiles ? tile_off[lane] : 0;
        long s = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long u = __shfl_up(s, o, 64);
            s = lane >= o ? s + u : s;
        }
        if (lane < tiles) tile_off[lane] = s - v;
    }
    __syncthreads();
    for (int p = tid; p < n; p += VAR_THREADS) {
        const long s = cs[p] + tile_off[p >> 6];
        cs[p] = s > Tmax ? Tmax : (int)s;
    }
    __syncthreads();
}

// the number of entries of the ascending cs[0 .. n) that are <= t
__device__ __forceinline__ int count_le(const int* __restrict__ cs, int n, int t) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cs[mid] <= t) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the number of entries of the ascending bins[0 .. n) that are < v (a NaN compares false everywhere: 0)
__device__ __forceinline__ int count_below(const float* __restrict__ bins, int n, float v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (bins[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int clamp_len(long v, int hi) { return v < 0 ? 0 : v > hi ? hi : (int)v; }

// grid (ceil(Tmax / LR_FRAMES), B).  After the scan the first LR_FRAMES threads bisect one frame each; then 2^lg lanes share a
// row, four rows in flight per thread.
__global__ __launch_bounds__(VAR_THREADS) void length_regulate_fwd_kernel(const float* __restrict__ x, long ld_row, long ld_batch,
                                                                          const int64_t* __restrict__ durations,
                                                                          const int64_t* __restrict__ phoneme_lens, int Pmax, int Tmax,
                                                                          int d4, int lg, float* __restrict__ y,
                                                                          int64_t* __restrict__ mel_lens, int32_t* __restrict__ index) {
    __shared__ int cs[VAR_MAX_P];
    __shared__ long tile_off[64];
    __shared__ int src[LR_FRAMES];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int t0 = blockIdx.x * LR_FRAMES;
    const int n = clamp_len(phoneme_lens[b], Pmax);
    scan_durations(durations + (long)b * Pmax, n, Tmax, cs, tile_off);
    const int frames = n > 0 ? cs[n - 1] : 0;
    if (blockIdx.x == 0 && tid == 0) mel_lens[b] = frames;
    if (tid < LR_FRAMES) {
        const int t = t0 + tid;
        const int p = t < frames ? count_le(cs, n, t) : -1;
        src[tid] = p;
        if (t < Tmax) index[(long)b * Tmax + t] = p;
    }
    __syncthreads();
    const int rows = Tmax - t0 < LR_FRAMES ? Tmax - t0 : LR_FRAMES;
    const int lanes = 1 << lg, r0 = tid >> lg, step = VAR_THREADS >> lg;
    const float4* xb = reinterpret_cast<const float4*>(x + (long)b * ld_batch);
    const long ld4 = ld_row >> 2;
    float4* yb = reinterpret_cast<float4*>(y) + ((long)b * Tmax + t0) * d4;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int c = tid & (lanes - 1); c < d4; c += lanes)
        for (int r = r0; r < rows; r += 4 * step) {
            const int r1 = r + step, r2 = r + 2 * step, r3 = r + 3 * step;
            const int q0 = src[r], q1 = r1 < rows ? src[r1] : -1, q2 = r2 < rows ? src[r2] : -1, q3 = r3 < rows ? src[r3] : -1;
            float4 v0 = zero, v1 = zero, v2 = zero, v3 = zero;
            if (q0 >= 0) v0 = xb[q0 * ld4 + c];
            if (q1 >= 0) v1 = xb[q1 * ld4 + c];
            if (q2 >= 0) v2 = xb[q2 * ld4 + c];
            if (q3 >= 0) v3 = xb[q3 * ld4 + c];
            yb[(long)r * d4 + c] = v0;
            if (r1 < rows) yb[(long)r1 * d4 + c] = v1;
            if (r2 < rows) yb[(long)r2 * d4 + c] = v2;
            if (r3 < rows) yb[(long)r3 * d4 + c] = v3;
        }
}

// grid (ceil(Pmax / (VAR_THREADS >> lg)), B): 2^lg lanes share a phoneme, a lane walks the phoneme's frames in ascending order
__global__ __launch_bounds__(VAR_THREADS) void length_regulate_bwd_kernel(const float* __restrict__ dy,
                                                                          const int64_t* __restrict__ durations,
                                                                          const int64_t* __restrict__ phoneme_lens, int Pmax, int Tmax,
                                                                          int d4, int lg, float* __restrict__ dx, int accumulate) {
    __shared__ int cs[VAR_MAX_P];
    __shared__ long tile_off[64];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int per = VAR_THREADS >> lg, lanes = 1 << lg;
    const int p = blockIdx.x * per + (tid >> lg);
    const int pl = clamp_len(phoneme_lens[b], Pmax);
    const int last = (blockIdx.x + 1) * per;
    const int n = pl < last ? pl : last;                                     // (the prefix up to this workgroup's phonemes)
    scan_durations(durations + (long)b * Pmax, n, Tmax, cs, tile_off);
    if (p >= Pmax) return;
    int a = 0, e = 0;
    if (p < n) {
        a = p > 0 ? cs[p - 1] : 0;
        e = cs[p];
    }
    const float4* dyb = reinterpret_cast<const float4*>(dy) + (long)b * Tmax * d4;
    float4* dxr = reinterpret_cast<float4*>(dx) + ((long)b * Pmax + p) * d4;
    for (int c = tid & (lanes - 1); c < d4; c += lanes) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        int t = a;
        for (; t + 4 <= e; t += 4) {                                         // four loads in flight, added in ascending t
            float4 g[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) g[u] = dyb[(long)(t + u) * d4 + c];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                acc.x += g[u].x; acc.y += g[u].y; acc.z += g[u].z; acc.w += g[u].w;
            }
        }
        for (; t < e; ++t) {
            const float4 g = dyb[(long)t * d4 + c];
            acc.x += g.x; acc.y += g.y; acc.z += g.z; acc.w += g.w;
        }
        if (accumulate) {
            const float4 o = dxr[c];
            acc.x = o.x + acc.x; acc.y = o.y + acc.y; acc.z = o.z + acc.z; acc.w = o.w + acc.w;
        }
        dxr[c] = acc;
    }
}

__global__ __launch_bounds__(VAR_THREADS) void durations_from_log_kernel(const float* __restrict__ log_d,
                                                                         const int64_t* __restrict__ phoneme_lens, int Pmax, double alpha,
                                                                         long min_duration, int64_t* __restrict__ out) {
    const int b = blockIdx.y;
    const int p = blockIdx.x * VAR_THREADS + threadIdx.x;
    if (p >= Pmax) return;
    const int pl = clamp_len(phoneme_lens[b], Pmax);
    long d = 0;
    if (p < pl) {
        const float v = log_d[(long)b * Pmax + p];
        if (v - v == 0.f) {                                                  // finite
            const double r = rint((exp((double)v) - 1.0) * alpha);           // (never NaN: exp is finite or +inf, alpha finite > 0)
            d = r >= (double)DUR_MAX ? DUR_MAX : r <= 0.0 ? 0 : (long)r;
        }
        d = d < min_duration ? min_duration : d;
    }
    out[(long)b * Pmax + p] = d;
}

// grid (ceil(Pmax / VE_ROWS), B).  The boundaries go to LDS, the first VE_ROWS threads bisect one row each, then the rows are
// added like the regulator copies them.
__global__ __launch_bounds__(VAR_THREADS) void variance_embed_fwd_kernel(const float* __restrict__ x, long ld_row, long ld_batch,
                                                                         const float* __restrict__ pitch, const float* __restrict__ energy,
                                                                         const float* __restrict__ pitch_bins, int nbp,
                                                                         const float* __restrict__ energy_bins, int nbe,
                                                                         const float* __restrict__ Ep, const float* __restrict__ Ee,
                                                                         const int64_t* __restrict__ phoneme_lens, int Pmax, int d4, int lg,
                                                                         float* __restrict__ y, int64_t* __restrict__ pitch_ids,
                                                                         int64_t* __restrict__ energy_ids) {
    __shared__ float bins[2 * (VAR_MAX_BINS - 1)];
    __shared__ int ids[2][VE_ROWS];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int p0 = blockIdx.x * VE_ROWS;
    const int pl = clamp_len(phoneme_lens[b], Pmax);
    float* pb = bins;
    float* eb = bins + (Ep ? nbp : 0);
    if (p0 < pl) {
        if (Ep) for (int i = tid; i < nbp; i += VAR_THREADS) pb[i] = pitch_bins[i];
        if (Ee) for (int i = tid; i < nbe; i += VAR_THREADS) eb[i] = energy_bins[i];
    }
    __syncthreads();
    if (tid < VE_ROWS) {
        const int p = p0 + tid;
        const long at = (long)b * Pmax + p;
        int i = -1, j = -1;
        if (p < pl) {
            if (Ep) i = count_below(pb, nbp, pitch[at]);
            if (Ee) j = count_below(eb, nbe, energy[at]);
        }
        ids[0][tid] = i;
        ids[1][tid] = j;
        if (p < Pmax) {
            if (Ep) pitch_ids[at] = i;
            if (Ee) energy_ids[at] = j;
        }
    }
    __syncthreads();
    const int rows = Pmax - p0 < VE_ROWS ? Pmax - p0 : VE_ROWS;
    const int lanes = 1 << lg, step = VAR_THREADS >> lg;
    const float4* xb = reinterpret_cast<const float4*>(x + (long)b * ld_batch);
    const long ld4 = ld_row >> 2;
    const float4* ep4 = reinterpret_cast<const float4*>(Ep);
    const float4* ee4 = reinterpret_cast<const float4*>(Ee);
    float4* yb = reinterpret_cast<float4*>(y) + ((long)b * Pmax + p0) * d4;
    for (int c = tid & (lanes - 1); c < d4; c += lanes)
        for (int r = tid >> lg; r < rows; r += step) {
            float4 v = xb[(long)(p0 + r) * ld4 + c];
            const int i = ids[0][r], j = ids[1][r];
            if (i >= 0) {
                const float4 e = ep4[(long)i * d4 + c];
                v.x += e.x; v.y += e.y; v.z += e.z; v.w += e.w;
            }
            if (j >= 0) {
                const float4 e = ee4[(long)j * d4 + c];
                v.x += e.x; v.y += e.y; v.z += e.z; v.w += e.w;
            }
            yb[(long)r * d4 + c] = v;
        }
}

__device__ __forceinline__ float log_duration_target(long d) {
    d = d < 0 ? 0 : d;
    return (float)log((double)d + 1.0);
}

__device__ __forceinline__ float butterfly_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = __fadd_rn(v, __shfl_xor(v, o, 64));
    return v;
}

// one workgroup of LOSS_THREADS threads; the order of its sums is the one stated at the top of the file
__global__ __launch_bounds__(LOSS_THREADS) void variance_loss_fwd_kernel(const float* __restrict__ log_d_pred,
                                                                         const int64_t* __restrict__ durations,
                                                                         const float* __restrict__ pitch_pred, const float* __restrict__ pitch_tgt,
                                                                         const float* __restrict__ energy_pred,
                                                                         const float* __restrict__ energy_tgt,
                                                                         const int64_t* __restrict__ phoneme_lens, int B, int Pmax, float w_d,
                                                                         float w_p, float w_e, float* __restrict__ out) {
    __shared__ float part[3][LOSS_THREADS / 64];
    __shared__ int cnt[LOSS_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long total = (long)B * Pmax;
    float sd = 0.f, sp = 0.f, se = 0.f;
    int n = 0;
    for (long i = tid; i < total; i += LOSS_THREADS) {
        const int b = (int)(i / Pmax), p = (int)(i - (long)b * Pmax);
        if (p >= clamp_len(phoneme_lens[b], Pmax)) continue;
        const float dd = __fsub_rn(log_d_pred[i], log_duration_target(durations[i]));
        const float dp = __fsub_rn(pitch_pred[i], pitch_tgt[i]);
        const float de = __fsub_rn(energy_pred[i], energy_tgt[i]);
        sd = __fadd_rn(sd, __fmul_rn(dd, dd));
        sp = __fadd_rn(sp, __fmul_rn(dp, dp));
        se = __fadd_rn(se, __fmul_rn(de, de));
        ++n;
    }
    sd = butterfly_sum(sd);
    sp = butterfly_sum(sp);
    se = butterfly_sum(se);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (lane == 0) {
        part[0][wave] = sd;
        part[1][wave] = sp;
        part[2][wave] = se;
        cnt[wave] = n;
    }
    __syncthreads();
    if (tid == 0) {
        float s[3] = {0.f, 0.f, 0.f};
        int m = 0;
        for (int w = 0; w < LOSS_THREADS / 64; ++w) {
#pragma unroll
            for (int k = 0; k < 3; ++k) s[k] = __fadd_rn(s[k], part[k][w]);
            m += cnt[w];
        }
        float L[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) L[k] = m > 0 ? __fdiv_rn(s[k], (float)m) : 0.f;
        out[0] = L[0];
        out[1] = L[1];
        out[2] = L[2];
        out[3] = __fadd_rn(__fadd_rn(__fmul_rn(w_d, L[0]), __fmul_rn(w_p, L[1])), __fmul_rn(w_e, L[2]));
    }
}

// grid-stride over (B, Pmax); every workgroup counts the valid phonemes itself (an integer sum over B lengths)
__global__ __launch_bounds__(VAR_THREADS) void variance_loss_bwd_kernel(const float* __restrict__ log_d_pred,
                                                                        const int64_t* __restrict__ durations,
                                                                        const float* __restrict__ pitch_pred, const float* __restrict__ pitch_tgt,
                                                                        const float* __restrict__ energy_pred,
                                                                        const float* __restrict__ energy_tgt,
                                                                        const int64_t* __restrict__ phoneme_lens, int B, int Pmax, float w_d,
                                                                        float w_p, float w_e, const float* __restrict__ gout,
                                                                        float* __restrict__ d_log_d, float* __restrict__ d_pitch,
                                                                        float* __restrict__ d_energy) {
    __shared__ long wsum[VAR_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long n = 0;
    for (int b = tid; b < B; b += VAR_THREADS) n += clamp_len(phoneme_lens[b], Pmax);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (lane == 0) wsum[wave] = n;
    __syncthreads();
    n = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    const float g3 = gout[3];
    const float two_n = n > 0 ? __fdiv_rn(2.f, (float)n) : 0.f;
    const float s_d = __fmul_rn(two_n, __fadd_rn(gout[0], __fmul_rn(w_d, g3)));
    const float s_p = __fmul_rn(two_n, __fadd_rn(gout[1], __fmul_rn(w_p, g3)));
    const float s_e = __fmul_rn(two_n, __fadd_rn(gout[2], __fmul_rn(w_e, g3)));
    const long total = (long)B * Pmax;
    for (long i = (long)blockIdx.x * VAR_THREADS + tid; i < total; i += (long)gridDim.x * VAR_THREADS) {
        const int b = (int)(i / Pmax), p = (int)(i - (long)b * Pmax);
        float gd = 0.f, gp = 0.f, ge = 0.f;
        if (n > 0 && p < clamp_len(phoneme_lens[b], Pmax)) {
            gd = __fmul_rn(s_d, __fsub_rn(log_d_pred[i], log_duration_target(durations[i])));
            gp = __fmul_rn(s_p, __fsub_rn(pitch_pred[i], pitch_tgt[i]));
            ge = __fmul_rn(s_e, __fsub_rn(energy_pred[i], energy_tgt[i]));
        }
        d_log_d[i] = gd;
        d_pitch[i] = gp;
        d_energy[i] = ge;
    }
}

static inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace ttts

using namespace ttts;

#define VAR_REQUIRE_SHAPE(name, B, Pmax)                                                                                      \
    TTTS_REQUIRE(B >= 1 && B <= 65535, "%s: B must be in [1, 65535] (one grid row per utterance), got %d", name, B);          \
    TTTS_REQUIRE(Pmax >= 1 && Pmax <= VAR_MAX_P, "%s: Pmax must be in [1, %d] phonemes, got %d", name, VAR_MAX_P, Pmax)
#define VAR_REQUIRE_D(name, D) \
    TTTS_REQUIRE(D >= 4 && D <= VAR_MAX_D && D % 4 == 0, "%s: D must be a multiple of 4 in [4, %d], got %d", name, VAR_MAX_D, D)
#define VAR_REQUIRE_T(name, Tmax) \
    TTTS_REQUIRE(Tmax >= 1 && Tmax <= VAR_MAX_T, "%s: Tmax must be in [1, 2^20] frames, got %d", name, Tmax)
#define VAR_REQUIRE_X(name, ld_row, ld_batch, B, Pmax, D)                                                                      \
    TTTS_REQUIRE(ld_row >= D && ld_row % 4 == 0, "%s: the row stride must be a multiple of 4 and >= D (ld_row %lld, D %d)", name, \
                 (long long)ld_row, D);                                                                                        \
    TTTS_REQUIRE((B == 1 && ld_batch >= 0) || (ld_batch % 4 == 0 && ld_batch >= (int64_t)(Pmax - 1) * ld_row + D),             \
                 "%s: the batch stride must be a multiple of 4 and cover an utterance (ld_batch %lld, ld_row %lld, Pmax %d, D %d)", \
                 name, (long long)ld_batch, (long long)ld_row, Pmax, D)

extern "C" {

int ttts_length_regulate_frames(void) { return LR_FRAMES; }

int ttts_length_regulate_fwd(const float* x, int64_t ld_row, int64_t ld_batch, const int64_t* durations, const int64_t* phoneme_lens,
                             int B, int Pmax, int Tmax, int D, float* y, int64_t* mel_lens, int32_t* index, void* stream) {
    const char* name = "length_regulate_fwd";
    TTTS_REQUIRE(x && durations && phoneme_lens && y && mel_lens && index, "%s: null pointer", name);
    VAR_REQUIRE_SHAPE(name, B, Pmax);
    VAR_REQUIRE_T(name, Tmax);
    VAR_REQUIRE_D(name, D);
    VAR_REQUIRE_X(name, ld_row, ld_batch, B, Pmax, D);
    TTTS_REQUIRE(aligned(x, 16) && aligned(y, 16), "%s: x and y must be 16-byte aligned", name);
    TTTS_REQUIRE(aligned(durations, 8) && aligned(phoneme_lens, 8) && aligned(mel_lens, 8),
                 "%s: durations, phoneme_lens and mel_lens must be 8-byte aligned", name);
    TTTS_REQUIRE(aligned(index, 4), "%s: index must be 4-byte aligned", name);
    const dim3 grid((unsigned)cdiv(Tmax, LR_FRAMES), (unsigned)B);
    hipLaunchKernelGGL(length_regulate_fwd_kernel, grid, dim3(VAR_THREADS), 0, (hipStream_t)stream, x, (long)ld_row, (long)ld_batch,
                       durations, phoneme_lens, Pmax, Tmax, D / 4, lanes_log2(D / 4), y, mel_lens, index);
    TTTS_LAUNCH_CHECK("length_regulate_fwd_kernel");
    return TTTS_OK;
}

int ttts_length_regulate_bwd(const float* dy, const int64_t* durations, const int64_t* phoneme_lens, int B, int Pmax, int Tmax, int D,
                             float* dx, int accumulate, void* stream) {
    const char* name = "length_regulate_bwd";
    TTTS_REQUIRE(dy && durations && phoneme_lens && dx, "%s: null pointer", name);
    VAR_REQUIRE_SHAPE(name, B, Pmax);
    VAR_REQUIRE_T(name, Tmax);
    VAR_REQUIRE_D(name, D);
    TTTS_REQUIRE(aligned(dy, 16) && aligned(dx, 16), "%s: dy and dx must be 16-byte aligned", name);
    TTTS_REQUIRE(aligned(durations, 8) && aligned(phoneme_lens, 8), "%s: durations and phoneme_lens must be 8-byte aligned", name);
    const int lg = lanes_log2(D / 4);
    const dim3 grid((unsigned)cdiv(Pmax, VAR_THREADS >> lg), (unsigned)B);
    hipLaunchKernelGGL(length_regulate_bwd_kernel, grid, dim3(VAR_THREADS), 0, (hipStream_t)stream, dy, durations, phoneme_lens, Pmax,
                       Tmax, D / 4, lg, dx, accumulate);
    TTTS_LAUNCH_CHECK("length_regulate_bwd_kernel");
    return TTTS_OK;
}

int ttts_durations_from_log(const float* log_d, const int64_t* phoneme_lens, int B, int Pmax, float alpha, int64_t min_duration,
                            int64_t* durations, void* stream) {
    const char* name = "durations_from_log";
    TTTS_REQUIRE(log_d && phoneme_lens && durations, "%s: null pointer", name);
    VAR_REQUIRE_SHAPE(name, B, Pmax);
    TTTS_REQUIRE(alpha > 0.f && alpha - alpha == 0.f, "%s: alpha must be positive and finite, got %g", name, (double)alpha);
    TTTS_REQUIRE(min_duration >= 0 && min_duration <= DUR_MAX, "%s: min_duration must be in [0, 2^31 - 1], got %lld", name,
                 (long long)min_duration);
    TTTS_REQUIRE(aligned(log_d, 4), "%s: log_d must be 4-byte aligned", name);
    TTTS_REQUIRE(aligned(phoneme_lens, 8) && aligned(durations, 8), "%s: phoneme_lens and durations must be 8-byte aligned", name);
    const dim3 grid((unsigned)cdiv(Pmax, VAR_THREADS), (unsigned)B);
    hipLaunchKernelGGL(durations_from_log_kernel, grid, dim3(VAR_THREADS), 0, (hipStream_t)stream, log_d, phoneme_lens, Pmax,
                       (double)alpha, (long)min_duration, durations);
    TTTS_LAUNCH_CHECK("durations_from_log_kernel");
    return TTTS_OK;
}

int ttts_variance_embed_fwd(const float* x, int64_t ld_row, int64_t ld_batch, const float* pitch, const float* energy,
                            const float* pitch_bins, int n_pitch, const float* energy_bins, int n_energy, const float* pitch_table,
                            const float* energy_table, const int64_t* phoneme_lens, int B, int Pmax, int D, float* y,
                            int64_t* pitch_ids, int64_t* energy_ids, void* stream) {
    const char* name = "variance_embed_fwd";
    TTTS_REQUIRE(x && phoneme_lens && y, "%s: null pointer", name);
    TTTS_REQUIRE(!pitch_table || (pitch && pitch_bins && pitch_ids), "%s: null pointer (a pitch table needs pitch, pitch_bins and pitch_ids)",
                 name);
    TTTS_REQUIRE(!energy_table || (energy && energy_bins && energy_ids),
                 "%s: null pointer (an energy table needs energy, energy_bins and energy_ids)", name);
    VAR_REQUIRE_SHAPE(name, B, Pmax);
    VAR_REQUIRE_D(name, D);
    TTTS_REQUIRE(!pitch_table || (n_pitch >= 2 && n_pitch <= VAR_MAX_BINS), "%s: n_pitch must be in [2, %d] table rows, got %d", name,
                 VAR_MAX_BINS, n_pitch);
    TTTS_REQUIRE(!energy_table || (n_energy >= 2 && n_energy <= VAR_MAX_BINS), "%s: n_energy must be in [2, %d] table rows, got %d", name,
                 VAR_MAX_BINS, n_energy);
    VAR_REQUIRE_X(name, ld_row, ld_batch, B, Pmax, D);
    TTTS_REQUIRE(aligned(x, 16) && aligned(y, 16) && aligned(pitch_table, 16) && aligned(energy_table, 16),
                 "%s: x, y and the tables must be 16-byte aligned", name);
    TTTS_REQUIRE(aligned(pitch, 4) && aligned(energy, 4) && aligned(pitch_bins, 4) && aligned(energy_bins, 4),
                 "%s: pitch, energy and the boundaries must be 4-byte aligned", name);
    TTTS_REQUIRE(aligned(phoneme_lens, 8) && aligned(pitch_ids, 8) && aligned(energy_ids, 8),
                 "%s: phoneme_lens and the ids must be 8-byte aligned", name);
    const dim3 grid((unsigned)cdiv(Pmax, VE_ROWS), (unsigned)B);
    hipLaunchKernelGGL(variance_embed_fwd_kernel, grid, dim3(VAR_THREADS), 0, (hipStream_t)stream, x, (long)ld_row, (long)ld_batch, pitch,
                       energy, pitch_bins, n_pitch - 1, energy_bins, n_energy - 1, pitch_table, energy_table, phoneme_lens, Pmax, D / 4,
                       lanes_log2(D / 4), y, pitch_ids, energy_ids);
    TTTS_LAUNCH_CHECK("variance_embed_fwd_kernel");
    return TTTS_OK;
}

#define VAR_REQUIRE_LOSS(name)                                                                                                  \
    VAR_REQUIRE_SHAPE(name, B, Pmax);                                                                                           \
    TTTS_REQUIRE(w_d - w_d == 0.f && w_p - w_p == 0.f && w_e - w_e == 0.f, "%s: the weights must be finite, got %g, %g, %g", name, \
                 (double)w_d, (double)w_p, (double)w_e);                                                                        \
    TTTS_REQUIRE(aligned(log_d_pred, 4) && aligned(pitch_pred, 4) && aligned(pitch_target, 4) && aligned(energy_pred, 4) &&    \
                     aligned(energy_target, 4),                                                                                 \
                 "%s: the predictions and targets must be 4-byte aligned", name);                                               \
    TTTS_REQUIRE(aligned(durations, 8) && aligned(phoneme_lens, 8), "%s: durations and phoneme_lens must be 8-byte aligned", name)

int ttts_variance_loss_fwd(const float* log_d_pred, const int64_t* durations, const float* pitch_pred, const float* pitch_target,
                           const float* energy_pred, const float* energy_target, const int64_t* phoneme_lens, int B, int Pmax, float w_d,
                           float w_p, float w_e, float* out, void* stream) {
    const char* name = "variance_loss_fwd";
    TTTS_REQUIRE(log_d_pred && durations && pitch_pred && pitch_target && energy_pred && energy_target && phoneme_lens && out,
                 "%s: null pointer", name);
    VAR_REQUIRE_LOSS(name);
    TTTS_REQUIRE(aligned(out, 4), "%s: out must be 4-byte aligned", name);
    hipLaunchKernelGGL(variance_loss_fwd_kernel, dim3(1), dim3(LOSS_THREADS), 0, (hipStream_t)stream, log_d_pred, durations, pitch_pred,
                       pitch_target, energy_pred, energy_target, phoneme_lens, B, Pmax, w_d, w_p, w_e, out);
    TTTS_LAUNCH_CHECK("variance_loss_fwd_kernel");
    return TTTS_OK;
}

int ttts_variance_loss_bwd(const float* log_d_pred, const int64_t* durations, const float* pitch_pred, const float* pitch_target,
                           const float* energy_pred, const float* energy_target, const int64_t* phoneme_lens, int B, int Pmax, float w_d,
                           float w_p, float w_e, const float* gout, float* d_log_d, float* d_pitch, float* d_energy, void* stream) {
    const char* name = "variance_loss_bwd";
    TTTS_REQUIRE(log_d_pred && durations && pitch_pred && pitch_target && energy_pred && energy_target && phoneme_lens && gout &&
                     d_log_d && d_pitch && d_energy,
                 "%s: null pointer", name);
    VAR_REQUIRE_LOSS(name);
    TTTS_REQUIRE(aligned(gout, 4) && aligned(d_log_d, 4) && aligned(d_pitch, 4) && aligned(d_energy, 4),
                 "%s: gout and the gradients must be 4-byte aligned", name);
    int grid = cdiv((long)B * Pmax, VAR_THREADS);
    if (grid > 1024) grid = 1024;
    hipLaunchKernelGGL(variance_loss_bwd_kernel, dim3(grid), dim3(VAR_THREADS), 0, (hipStream_t)stream, log_d_pred, durations, pitch_pred,
                       pitch_target, energy_pred, energy_target, phoneme_lens, B, Pmax, w_d, w_p, w_e, gout, d_log_d, d_pitch, d_energy);
    TTTS_LAUNCH_CHECK("variance_loss_bwd_kernel");
    return TTTS_OK;
}

}  // extern "C"
