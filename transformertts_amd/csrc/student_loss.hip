// Mel loss of a FastSpeech-2-style student (gfx950): the masked mean absolute and mean squared error between two ragged mel
// batches, their weighted sum, the sum with one further device scalar (the variance loss's total), and the gradient of pred.
//   lengths     n_b = clamp(min(pred_lens[b], target_lens[b]), 0, min(T, Tt)); N = sum_b n_b, an integer sum (the order is free);
//               den = (float)(N M), the integer product rounded once.
//   chunks      utterance b is cut into nblk = ceil(min(T, Tt) / ML_ROWS) chunks of ML_ROWS frames; chunk c = b nblk + r holds
//               the frames [r ML_ROWS, min((r + 1) ML_ROWS, n_b)) of b, possibly none.  G = min(B nblk, ML_MAX_WG) workgroups of
//               ML_THREADS threads run; workgroup w owns the chunks w, w + G, w + 2 G, ... -- the grid follows from the shapes alone.
//   partials    thread i of workgroup w keeps two fp32 sums, both from 0.f.  It walks its workgroup's chunks in ascending order
//               and in each the float4s i, i + ML_THREADS, ... of the chunk's valid frames (row-major over (frame, M / 4)), and in
//               each float4 the elements x, y, z, w: d = pred - tgt; s_abs += |d|; s_sq += d d, the product rounded on its own.
//               The 64 lanes of a wave meet in a butterfly (lane l adds lane l ^ 32, then ^ 16, ... ^ 1); thread 0 adds the wave
//               sums in ascending wave order from 0.f and stores ws[2 w], ws[2 w + 1].  Every workgroup stores, whatever it saw.
//   finish      one workgroup of ML_SWEEP threads: thread i adds the partials i, i + ML_SWEEP, ... < G in ascending order from
//               0.f; the same butterfly, the same ascending sum of the wave sums; mae = S_abs / den, mse = S_sq / den, both
//               exactly 0 when N = 0; mel = w_mae mae + w_mse mse (two products, one sum); total = mel + extra[0], or mel itself
//               when extra is NULL; frames = N.
//   gradient    G' = g_total + g_mel; a = ((G' w_mae) + g_mae) / den; q = (2 ((G' w_mse) + g_mse)) / den; for t < n_b
//               dpred = sign(d) a + q d with sign(0) = 0 (a product, then one sum), exact 0 at and behind n_b and everywhere
//               when N = 0.  A NULL upstream pointer counts as 0.f.  Every workgroup takes N itself from the 2 B lengths.
// Every product, sum and quotient is rounded on its own (no contraction).  No atomics, no allocation, no host read: the same
// bits on every call, capturable into a HIP graph.  Nothing at or behind n_b is read in either operand.
#include "ttts_common.h"

namespace ttts {

constexpr int ML_THREADS = 256;
constexpr int ML_WAVES = ML_THREADS / 64;
constexpr int ML_ROWS = 32;                // frames of one chunk
constexpr int ML_MAX_WG = 2048;            // workgroups of the partial-sum launch at the most: the workspace stays 16 KB
constexpr int ML_SWEEP = 256;              // threads of the finishing workgroup: partials it takes in one sweep
constexpr int ML_BWD_MAX_X = 1024;         // workgroups per utterance of the gradient launch at the most
constexpr int ML_MAX_T = 1 << 20;
constexpr int ML_MAX_M = 4096;

__device__ __forceinline__ float ml_butterfly(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = __fadd_rn(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ int ml_len(long a, long b, int hi) {
    const long v = a < b ? a : b;
    return v < 0 ? 0 : v > hi ? hi : (int)v;
}

// |d| and d d of one float4 onto the two running sums, x y z w in that order
__device__ __forceinline__ void ml_accumulate(const float4 p, const float4 t, float& s_abs, float& s_sq) {
    const float d0 = __fsub_rn(p.x, t.x), d1 = __fsub_rn(p.y, t.y), d2 = __fsub_rn(p.z, t.z), d3 = __fsub_rn(p.w, t.w);
    s_abs = __fadd_rn(s_abs, fabsf(d0));
    s_sq = __fadd_rn(s_sq, __fmul_rn(d0, d0));
    s_abs = __fadd_rn(s_abs, fabsf(d1));
    s_sq = __fadd_rn(s_sq, __fmul_rn(d1, d1));
    s_abs = __fadd_rn(s_abs, fabsf(d2));
    s_sq = __fadd_rn(s_sq, __fmul_rn(d2, d2));
    s_abs = __fadd_rn(s_abs, fabsf(d3));
    s_sq = __fadd_rn(s_sq, __fmul_rn(d3, d3));
}

__global__ __launch_bounds__(ML_THREADS) void mel_loss_partial_kernel(const float* __restrict__ pred, long ldr_p, long ldb_p,
                                                                      const float* __restrict__ tgt, long ldr_t, long ldb_t,
                                                                      const int64_t* __restrict__ pred_lens,
                                                                      const int64_t* __restrict__ tgt_lens, int Tmin, int d4, int nblk,
                                                                      long chunks, float* __restrict__ ws) {
    __shared__ float part[2][ML_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float s_abs = 0.f, s_sq = 0.f;
    for (long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int b = (int)(c / nblk), r0 = (int)(c - (long)b * nblk) * ML_ROWS;
        const int n = ml_len(pred_lens[b], tgt_lens[b], Tmin);
        int rows = n - r0;
        rows = rows > ML_ROWS ? ML_ROWS : rows;
        if (rows <= 0) continue;                                            // (wave-uniform: b and r0 are the workgroup's)
        const float* pb = pred + (long)b * ldb_p + (long)r0 * ldr_p;
        const float* tb = tgt + (long)b * ldb_t + (long)r0 * ldr_t;
        const int n4 = rows * d4;
        for (int j = tid; j < n4; j += ML_THREADS) {
            const int row = j / d4, col = (j - row * d4) * 4;
            const float4 p = *reinterpret_cast<const float4*>(pb + (long)row * ldr_p + col);
            const float4 t = *reinterpret_cast<const float4*>(tb + (long)row * ldr_t + col);
            ml_accumulate(p, t, s_abs, s_sq);
        }
    }
    s_abs = ml_butterfly(s_abs);
    s_sq = ml_butterfly(s_sq);
    if (lane == 0) {
        part[0][wave] = s_abs;
        part[1][wave] = s_sq;
    }
    __syncthreads();
    if (tid == 0) {
        float a = 0.f, q = 0.f;
#pragma unroll
        for (int w = 0; w < ML_WAVES; ++w) {
            a = __fadd_rn(a, part[0][w]);
            q = __fadd_rn(q, part[1][w]);
        }
        ws[2 * blockIdx.x] = a;
        ws[2 * blockIdx.x + 1] = q;
    }
}

// N = sum_b n_b for all threads of a workgroup of THREADS threads (ends on a barrier; `wsum` holds THREADS / 64 longs)
template <int THREADS>
__device__ __forceinline__ long ml_frames(const int64_t* __restrict__ pred_lens, const int64_t* __restrict__ tgt_lens, int B, int Tmin,
                                          long* __restrict__ wsum) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long n = 0;
    for (int b = tid; b < B; b += THREADS) n += ml_len(pred_lens[b], tgt_lens[b], Tmin);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (lane == 0) wsum[wave] = n;
    __syncthreads();
    n = 0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) n += wsum[w];
    return n;
}

__global__ __launch_bounds__(ML_SWEEP) void mel_loss_finish_kernel(const float* __restrict__ ws, int G,
                                                                   const int64_t* __restrict__ pred_lens,
                                                                   const int64_t* __restrict__ tgt_lens, int B, int Tmin, int M, float w_mae,
                                                                   float w_mse, const float* __restrict__ extra, float* __restrict__ out,
                                                                   int64_t* __restrict__ frames) {
    __shared__ float part[2][ML_SWEEP / 64];
    __shared__ long wsum[ML_SWEEP / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long N = ml_frames<ML_SWEEP>(pred_lens, tgt_lens, B, Tmin, wsum);
    float s_abs = 0.f, s_sq = 0.f;
    for (int i = tid; i < G; i += ML_SWEEP) {
        s_abs = __fadd_rn(s_abs, ws[2 * i]);
        s_sq = __fadd_rn(s_sq, ws[2 * i + 1]);
    }
    s_abs = ml_butterfly(s_abs);
    s_sq = ml_butterfly(s_sq);
    if (lane == 0) {
        part[0][wave] = s_abs;
        part[1][wave] = s_sq;
    }
    __syncthreads();
    if (tid == 0) {
        float a = 0.f, q = 0.f;
#pragma unroll
        for (int w = 0; w < ML_SWEEP / 64; ++w) {
            a = __fadd_rn(a, part[0][w]);
            q = __fadd_rn(q, part[1][w]);
        }
        const float den = (float)(N * (long)M);
        const float mae = N > 0 ? __fdiv_rn(a, den) : 0.f;
        const float mse = N > 0 ? __fdiv_rn(q, den) : 0.f;
        const float mel = __fadd_rn(__fmul_rn(w_mae, mae), __fmul_rn(w_mse, mse));
        out[0] = mae;
        out[1] = mse;
        out[2] = mel;
        out[3] = extra != nullptr ? __fadd_rn(mel, extra[0]) : mel;
        frames[0] = N;
    }
}

// grid (x, B): the workgroups of a row of the grid stride over the T M / 4 float4s of utterance b
__global__ __launch_bounds__(ML_THREADS) void mel_loss_bwd_kernel(const float* __restrict__ pred, long ldr_p, long ldb_p,
                                                                  const float* __restrict__ tgt, long ldr_t, long ldb_t,
                                                                  const int64_t* __restrict__ pred_lens, const int64_t* __restrict__ tgt_lens,
                                                                  int B, int T, int Tmin, int d4, float w_mae, float w_mse,
                                                                  const float* __restrict__ g_mae, const float* __restrict__ g_mse,
                                                                  const float* __restrict__ g_mel, const float* __restrict__ g_total,
                                                                  float* __restrict__ dpred) {
    __shared__ long wsum[ML_WAVES];
    const int tid = threadIdx.x, b = blockIdx.y;
    const long N = ml_frames<ML_THREADS>(pred_lens, tgt_lens, B, Tmin, wsum);
    const int n = N > 0 ? ml_len(pred_lens[b], tgt_lens[b], Tmin) : 0;
    float a = 0.f, q = 0.f;
    if (N > 0) {
        const float up = __fadd_rn(g_total != nullptr ? g_total[0] : 0.f, g_mel != nullptr ? g_mel[0] : 0.f);
        const float den = (float)(N * (long)(d4 * 4));
        a = __fdiv_rn(__fadd_rn(__fmul_rn(up, w_mae), g_mae != nullptr ? g_mae[0] : 0.f), den);
        q = __fdiv_rn(__fmul_rn(2.f, __fadd_rn(__fmul_rn(up, w_mse), g_mse != nullptr ? g_mse[0] : 0.f)), den);
    }
    const int valid4 = n * d4, total4 = T * d4;                              // T M / 4 <= 2^30
    const float* pb = pred + (long)b * ldb_p;
    const float* tb = tgt + (long)b * ldb_t;
    float4* ob = reinterpret_cast<float4*>(dpred) + (long)b * total4;
    for (int j = blockIdx.x * ML_THREADS + tid; j < total4; j += gridDim.x * ML_THREADS) {
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j < valid4) {
            const int row = j / d4, col = (j - row * d4) * 4;
            const float4 p = *reinterpret_cast<const float4*>(pb + (long)row * ldr_p + col);
            const float4 t = *reinterpret_cast<const float4*>(tb + (long)row * ldr_t + col);
            const float d0 = __fsub_rn(p.x, t.x), d1 = __fsub_rn(p.y, t.y), d2 = __fsub_rn(p.z, t.z), d3 = __fsub_rn(p.w, t.w);
            g.x = __fadd_rn(d0 > 0.f ? a : d0 < 0.f ? -a : 0.f, __fmul_rn(q, d0));
            g.y = __fadd_rn(d1 > 0.f ? a : d1 < 0.f ? -a : 0.f, __fmul_rn(q, d1));
            g.z = __fadd_rn(d2 > 0.f ? a : d2 < 0.f ? -a : 0.f, __fmul_rn(q, d2));
            g.w = __fadd_rn(d3 > 0.f ? a : d3 < 0.f ? -a : 0.f, __fmul_rn(q, d3));
        }
        ob[j] = g;
    }
}

static inline bool ml_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

static inline long ml_chunks(int B, int T, int Tt) { return (long)B * cdiv(T < Tt ? T : Tt, ML_ROWS); }

static inline int ml_workgroups(int B, int T, int Tt) {
    const long c = ml_chunks(B, T, Tt);
    return c > ML_MAX_WG ? ML_MAX_WG : (int)c;
}

}  // namespace ttts

using namespace ttts;

#define ML_REQUIRE_X(name, what, ld_row, ld_batch, B, rows, M)                                                                 \
    TTTS_REQUIRE(ld_row >= M && ld_row % 4 == 0, "%s: the row stride of %s must be a multiple of 4 and >= M (ld_row %lld, M %d)", \
                 name, what, (long long)ld_row, M);                                                                            \
    TTTS_REQUIRE((B == 1 && ld_batch >= 0) || (ld_batch % 4 == 0 && ld_batch >= (int64_t)(rows - 1) * ld_row + M),             \
                 "%s: the batch stride of %s must be a multiple of 4 and cover an utterance (ld_batch %lld, ld_row %lld, frames %d, " \
                 "M %d)", name, what, (long long)ld_batch, (long long)ld_row, rows, M)

#define ML_REQUIRE_COMMON(name)                                                                                                \
    TTTS_REQUIRE(B >= 1 && B <= 65535, "%s: B must be in [1, 65535] (one grid row per utterance), got %d", name, B);          \
    TTTS_REQUIRE(T >= 1 && T <= ML_MAX_T, "%s: T must be in [1, 2^20] frames, got %d", name, T);                              \
    TTTS_REQUIRE(Tt >= 1 && Tt <= ML_MAX_T, "%s: Tt must be in [1, 2^20] frames, got %d", name, Tt);                          \
    TTTS_REQUIRE(M >= 4 && M <= ML_MAX_M && M % 4 == 0, "%s: M must be a multiple of 4 in [4, %d], got %d", name, ML_MAX_M, M); \
    ML_REQUIRE_X(name, "pred", ld_row_pred, ld_batch_pred, B, T, M);                                                           \
    ML_REQUIRE_X(name, "target", ld_row_target, ld_batch_target, B, Tt, M);                                                    \
    TTTS_REQUIRE(w_mae - w_mae == 0.f && w_mse - w_mse == 0.f, "%s: the weights must be finite, got %g, %g", name, (double)w_mae, \
                 (double)w_mse);                                                                                               \
    TTTS_REQUIRE(ml_aligned(pred, 16) && ml_aligned(target, 16), "%s: pred and target must be 16-byte aligned", name);        \
    TTTS_REQUIRE(ml_aligned(pred_lens, 8) && ml_aligned(target_lens, 8), "%s: pred_lens and target_lens must be 8-byte aligned", name)

extern "C" {

int ttts_mel_loss_rows(void) { return ML_ROWS; }
int ttts_mel_loss_sweep(void) { return ML_SWEEP; }
int ttts_mel_loss_max_workgroups(void) { return ML_MAX_WG; }

size_t ttts_mel_loss_workspace_bytes(int B, int T, int Tt, int M) {
    if (B < 1 || B > 65535 || T < 1 || T > ML_MAX_T || Tt < 1 || Tt > ML_MAX_T || M < 4 || M > ML_MAX_M || M % 4 != 0) return 0;
    return (size_t)ml_workgroups(B, T, Tt) * 2 * sizeof(float);
}

int ttts_mel_loss_fwd(const float* pred, int64_t ld_row_pred, int64_t ld_batch_pred, const float* target, int64_t ld_row_target,
                      int64_t ld_batch_target, const int64_t* pred_lens, const int64_t* target_lens, int B, int T, int Tt, int M,
                      float w_mae, float w_mse, const float* extra, float* out, int64_t* frames, void* workspace,
                      size_t workspace_bytes, void* stream) {
    const char* name = "mel_loss_fwd";
    TTTS_REQUIRE(pred && target && pred_lens && target_lens && out && frames && workspace, "%s: null pointer", name);
    ML_REQUIRE_COMMON(name);
    TTTS_REQUIRE(ml_aligned(extra, 4) && ml_aligned(out, 4) && ml_aligned(workspace, 4), "%s: extra, out and the workspace must be "
                 "4-byte aligned", name);
    TTTS_REQUIRE(ml_aligned(frames, 8), "%s: frames must be 8-byte aligned", name);
    const size_t need = ttts_mel_loss_workspace_bytes(B, T, Tt, M);
    TTTS_REQUIRE(workspace_bytes >= need, "%s: the workspace holds %zu bytes, ttts_mel_loss_workspace_bytes asks for %zu", name,
                 workspace_bytes, need);
    const int Tmin = T < Tt ? T : Tt, G = ml_workgroups(B, T, Tt);
    float* ws = static_cast<float*>(workspace);
    hipLaunchKernelGGL(mel_loss_partial_kernel, dim3(G), dim3(ML_THREADS), 0, (hipStream_t)stream, pred, (long)ld_row_pred,
                       (long)ld_batch_pred, target, (long)ld_row_target, (long)ld_batch_target, pred_lens, target_lens, Tmin, M / 4,
                       cdiv(Tmin, ML_ROWS), ml_chunks(B, T, Tt), ws);
    TTTS_LAUNCH_CHECK("mel_loss_partial_kernel");
    hipLaunchKernelGGL(mel_loss_finish_kernel, dim3(1), dim3(ML_SWEEP), 0, (hipStream_t)stream, ws, G, pred_lens, target_lens, B, Tmin, M,
                       w_mae, w_mse, extra, out, frames);
    TTTS_LAUNCH_CHECK("mel_loss_finish_kernel");
    return TTTS_OK;
}

int ttts_mel_loss_bwd(const float* pred, int64_t ld_row_pred, int64_t ld_batch_pred, const float* target, int64_t ld_row_target,
                      int64_t ld_batch_target, const int64_t* pred_lens, const int64_t* target_lens, int B, int T, int Tt, int M,
                      float w_mae, float w_mse, const float* g_mae, const float* g_mse, const float* g_mel, const float* g_total,
                      float* dpred, void* stream) {
    const char* name = "mel_loss_bwd";
    TTTS_REQUIRE(pred && target && pred_lens && target_lens && dpred, "%s: null pointer", name);
    ML_REQUIRE_COMMON(name);
    TTTS_REQUIRE(ml_aligned(g_mae, 4) && ml_aligned(g_mse, 4) && ml_aligned(g_mel, 4) && ml_aligned(g_total, 4),
                 "%s: the upstream gradients must be 4-byte aligned", name);
    TTTS_REQUIRE(ml_aligned(dpred, 16), "%s: dpred must be 16-byte aligned", name);
    int gx = cdiv((long)T * (M / 4), ML_THREADS);
    if (gx > ML_BWD_MAX_X) gx = ML_BWD_MAX_X;
    hipLaunchKernelGGL(mel_loss_bwd_kernel, dim3((unsigned)gx, (unsigned)B), dim3(ML_THREADS), 0, (hipStream_t)stream, pred,
                       (long)ld_row_pred, (long)ld_batch_pred, target, (long)ld_row_target, (long)ld_batch_target, pred_lens,
                       target_lens, B, T, T < Tt ? T : Tt, M / 4, w_mae, w_mse, g_mae, g_mse, g_mel, g_total, dpred);
    TTTS_LAUNCH_CHECK("mel_loss_bwd_kernel");
    return TTTS_OK;
}

}  // extern "C"
