// A length-masked Conv1d -> ReLU -> LayerNorm -> Dropout stage on ragged (B, Pmax, C) rows (gfx950): the building block of
// FastSpeech 2's variance predictors.  pl_b = clamp(lens[b], 0, Pmax); x' = x below pl_b, exact zeros elsewhere.
//   forward     z[b, p, co] = bias[co] + sum_j sum_ci w[co, ci, j] x'[b, p + j - taps / 2, ci];  r = max(z, 0);  mean and rstd = 1 /
//               sqrt(var + eps) of r over co (biased variance, two passes);  y = fma((r - mean) rstd, gamma, beta), times keep / (1 -
//               drop_p) when drop_p > 0;  y, r, mean, rstd exact zeros for p >= pl_b.
//   backward    g = dy keep / (1 - drop_p);  dgamma = sum g x_hat, dbeta = sum g;  gg = g gamma;  dr = rstd (gg - mean_co(gg) - x_hat
//               mean_co(gg x_hat));  dz = dr [r > 0];  dbias = sum dz;  dx = the plain convolution of dz with the flipped, transposed
//               weight, zeros behind the lengths;  dw = ttts_conv1d_bwd_weight(dz, x').
// ragged_conv_kernel is an implicit GEMM on v_mfma_f32_32x32x2_f32, compiled per tap count.  A workgroup of eight waves owns
// RC_ROWS = 32 rows of ONE utterance (grid (ceil(Pmax / 32), B, blocks of 256 output columns)) and up to 256 output columns: wave
// v the 32-column block v, one 32 x 32 accumulator.  The reduction runs over chunks of kc input channels (kc taps <= 48 floats of a
// weight row, which are contiguous in nn.Conv1d's layout: no re-laid weight), inside a chunk over the taps in ascending order,
// inside a tap over the channels in ascending order; every accumulator is one fma chain in that order.  The next two chunks are
// in flight in registers while one is multiplied out of LDS.  The loader substitutes zeros for p < 0, p >= pl_b and channels
// behind Cin; a workgroup wholly behind pl_b writes zeros and returns.  NORM = false is the plain mode: no epilogue but the
// length mask, output columns in blocks of 256 (dx from dz and the flipped, transposed weight).
// Sums over a row's columns (NORM): the 32 lanes of a half wave meet in a butterfly (xor 16, 8, 4, 2, 1), and the eight waves'
// partials are added in ascending wave order; the mean first, then the squared deviations the same way.  Sums over rows (the row
// kernel): a wave walks rows v, v + 4, ... of its workgroup's 32 in ascending order, a lane adding into its own columns; the four
// waves' partials are added in ascending wave order; the finish kernel adds the workgroups' partials ((b, tile) ascending) in
// eight contiguous slices, each in ascending order, then the slices in ascending order.
// No atomics, no allocation, no host read; nothing at or behind a length is read.
// The conv feed-forward sublayer of an FFT block runs on the same main loop under four more epilogues:
//   forward     h = max(conv_k1(x') + b1, 0) (RC_RELU, the plain layout: Chid up to 1024 in column blocks of 256; the workgroups of
//               column block 0 leave x' behind);  z = conv_k2(h) + b2;  s = x' + z keep / (1 - drop_p);  y = LayerNorm(s) gamma +
//               beta (RC_RESNORM: a workgroup owns whole rows, the residual is read in the epilogue through x's strides)
//   backward    ds = LayerNorm's backward of dy (the row kernel, RES form: also dgamma, dbeta);  dz2 = ds keep / (1 - drop_p);
//               dz1 = conv(dz2, flipped w2) [h > 0] (RC_GATE);  dx = conv(dz1, flipped w1) + ds (RC_ADD);  dw1, db1 =
//               ttts_conv1d_bwd_weight(dz1, x');  dw2, db2 = ttts_conv1d_bwd_weight(dz2, h)
#include "ttts_common.h"

#include <math.h>

namespace ttts {

#ifndef TTTS_RC_ROWS
#define TTTS_RC_ROWS 32                    // rows of one utterance a workgroup of the convolution owns: 32, or 64 (measured: slower)
#endif
constexpr int RC_THREADS = 512;            // the convolution: eight waves, one 32-column block each
constexpr int RC_WAVES = RC_THREADS / 64;
constexpr int RC_ROWS = TTTS_RC_ROWS;
constexpr int RC_RT = RC_ROWS / 32;        // 32-row tiles of a wave
constexpr int RC_COLS = 256;               // output columns a workgroup owns
constexpr int RC_MAX_TAPS = 9;
constexpr int RC_WFLOATS = 48;             // floats of one weight row in a chunk: kc * taps
constexpr int RC_WP = RC_WFLOATS + 1;      // odd pitches: the 32 rows (columns) an MFMA operand reads fall into 32 banks
constexpr int RC_XP = 33;
constexpr int RC_XROWS = RC_ROWS + RC_MAX_TAPS - 1;
constexpr int RC_WREGS = RC_COLS * (RC_WFLOATS / 4) / RC_THREADS;            // float4 of the next chunk a thread holds
constexpr int RC_XREGS = (RC_XROWS * 8 + RC_THREADS - 1) / RC_THREADS;
constexpr int RC_MAX_P = 4096;
constexpr int RC_MAX_CIN = 1024;
constexpr int RB_THREADS = 256;            // the row kernel and the small ones
constexpr int RB_ROWS = 32;                // rows a workgroup of the row kernel owns
constexpr int RF_SLICES = 8;               // the finish: slices of the workgroups' partials, added slice by slice
static_assert(RC_ROWS == 32 || RC_ROWS == 64, "one or two 32-row MFMA tiles per wave");
static_assert(RC_COLS == 32 * RC_WAVES && RC_COLS * (RC_WFLOATS / 4) % RC_THREADS == 0, "a wave per 32-column block");

// input channels per chunk: the multiple of 4 with kc * taps <= RC_WFLOATS, at most 32 (taps 1, 3, 5, 7, 9: 32, 16, 8, 4, 4)
constexpr int rc_chunk(int taps) { return ((RC_WFLOATS / taps) & ~3) > 32 ? 32 : ((RC_WFLOATS / taps) & ~3); }

__device__ __forceinline__ int rc_clamp_len(long v, int hi) { return v < 0 ? 0 : v > hi ? hi : (int)v; }

// what follows the main loop.  RC_PLAIN: the length mask.  RC_NORM: bias, ReLU, LayerNorm, dropout (a workgroup owns whole rows).
// RC_RELU: bias, ReLU.  RC_RESNORM: bias, dropout, + aux (the residual, through its strides), LayerNorm (whole rows; r receives
// the LayerNorm's input).  RC_GATE: times [aux > 0].  RC_ADD: + aux.  aux is read at the output element, below the length only.
enum RaggedMode { RC_PLAIN = 0, RC_NORM = 1, RC_RELU = 2, RC_RESNORM = 3, RC_GATE = 4, RC_ADD = 5 };

struct RaggedConvArgs {
    const float* x; long ld_row, ld_batch;     // (B, Pmax, C) through its strides
    const int64_t* lens;
    const float* w;                             // (N, C, taps)
    const float* bias; const float* gamma; const float* beta;
    int Pmax, C, N;
    float eps, drop_scale; uint32_t drop_thr; uint64_t seed; const uint64_t* step_seed;
    float* y; float* r; float* mean; float* rstd; float* x_masked;
    const float* aux = nullptr; long aux_ld_row = 0, aux_ld_batch = 0;      // (B, Pmax, N) through its strides
};

// sum over the 32 lanes of a half wave, in every lane of it
__device__ __forceinline__ float half_wave_sum(float v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v = __fadd_rn(v, __shfl_xor(v, o, 64));
    return v;
}

// per-row sums of val[rt][i] (this lane's contribution to row rt * 32 + acc_row(i, half)) over all columns of the workgroup
// -> out[row] for every row of the tile; ends on a barrier
__device__ __forceinline__ void row_sums(float (&val)[RC_RT][16], float (*red)[RC_ROWS], float* out, int wave, int lane) {
    const int half = lane >> 5;
#pragma unroll
    for (int rt = 0; rt < RC_RT; ++rt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float s = half_wave_sum(val[rt][i]);
            if ((lane & 31) == 0) red[wave][rt * 32 + acc_row(i, half)] = s;
        }
    __syncthreads();
    if (threadIdx.x < RC_ROWS) {
        const int t = threadIdx.x;
        float s = red[0][t];
#pragma unroll
        for (int v = 1; v < RC_WAVES; ++v) s = __fadd_rn(s, red[v][t]);
        out[t] = s;
    }
    __syncthreads();
}

template <int MODE, int TAPS>
__global__ __launch_bounds__(RC_THREADS) void ragged_conv_kernel(const RaggedConvArgs a) {
    constexpr bool NORM = MODE == RC_NORM || MODE == RC_RESNORM;             // a workgroup owns whole rows and normalises them
    constexpr bool XM = MODE == RC_NORM || MODE == RC_RELU;                  // the loader may leave x' behind
    // the feed-forward's modes (reductions up to 9 x 1024 deep) close the fma chain after every chunk and add the chunks' sums in
    // ascending order: a chain of at most 24 MFMAs, then one fp32 add per chunk.  The two modes of the stage keep their one chain.
    constexpr bool FOLD = MODE >= RC_RELU;
    __shared__ float Ws[RC_COLS * RC_WP];
    __shared__ float Xs[RC_XROWS * RC_XP];
    __shared__ float red[RC_WAVES][RC_ROWS];
    __shared__ float stat[2][RC_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, lr = lane & 31;
    const int b = blockIdx.y, p0 = blockIdx.x * RC_ROWS, n0 = blockIdx.z * RC_COLS;
    constexpr int taps = TAPS, kc = rc_chunk(TAPS), pad = TAPS >> 1;    // (compile-time: the loader divides by constants, the taps unroll)
    const int Pmax = a.Pmax, C = a.C, N = a.N;
    const int pl = rc_clamp_len(a.lens[b], Pmax);
    const int rows = Pmax - p0 < RC_ROWS ? Pmax - p0 : RC_ROWS;
    const int ncols = N - n0 < RC_COLS ? N - n0 : RC_COLS;
    const long row0 = (long)b * Pmax + p0;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    if (p0 >= pl) {                                                          // wholly behind the length: zeros, nothing read
        const int n4 = ncols >> 2;
        for (int i = tid; i < rows * n4; i += RC_THREADS) {
            const int rr = i / n4, c4 = i - rr * n4;
            const long at = (row0 + rr) * N + n0 + 4 * c4;
            *reinterpret_cast<float4*>(a.y + at) = zero4;
            if (NORM && a.r) *reinterpret_cast<float4*>(a.r + at) = zero4;
        }
        if (NORM && a.r && tid < rows) {
            a.mean[row0 + tid] = 0.f;
            a.rstd[row0 + tid] = 0.f;
        }
        if (XM && a.x_masked && (MODE == RC_NORM || blockIdx.z == 0)) {
            const int c4n = C >> 2;
            for (int i = tid; i < rows * c4n; i += RC_THREADS) reinterpret_cast<float4*>(a.x_masked + row0 * C)[i] = zero4;
        }
        return;
    }

    const int nblk = (ncols + 31) >> 5;
    const bool has = wave < nblk;                                            // this wave's block: columns n0 + 32 wave ..
    f32x16 acc[RC_RT];
#pragma unroll
    for (int rt = 0; rt < RC_RT; ++rt)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[rt][i] = 0.f;
    f32x16 tot[FOLD ? RC_RT : 1];
    if (FOLD) {
#pragma unroll
        for (int rt = 0; rt < RC_RT; ++rt)
#pragma unroll
            for (int i = 0; i < 16; ++i) tot[rt][i] = 0.f;
    }

    const float* xb = a.x + (long)b * a.ld_batch;
    constexpr int kc4 = kc >> 2, xn = (RC_ROWS + taps - 1) * kc4;                // float4 of a chunk of x': rows p0 - pad .. p0 + ROWS - 1 + pad
    constexpr int wq = (kc * taps) >> 2;
    const int wn = nblk * 32 * wq;                    // float4 per weight row and chunk, and of a chunk of w
    // the next TWO chunks are in flight while this one is multiplied (a weight chunk comes from L2 or beyond: one chunk's
    // MFMAs do not cover that latency), in two register sets that take turns
    float4 xr0[RC_XREGS], wr0[RC_WREGS], xr1[RC_XREGS], wr1[RC_WREGS];
    auto load_chunk = [&](int ci0, float4 (&xr)[RC_XREGS], float4 (&wr)[RC_WREGS]) {
#pragma unroll
        for (int u = 0; u < RC_XREGS; ++u) {
            const int i = tid + u * RC_THREADS;
            xr[u] = zero4;
            if (i < xn) {
                const int rr = i / kc4, c4 = i - rr * kc4;
                const int p = p0 - pad + rr, ci = ci0 + 4 * c4;
                if (p >= 0 && p < pl && ci < C) xr[u] = *reinterpret_cast<const float4*>(xb + (long)p * a.ld_row + ci);
            }
        }
        const int nq = ((C - ci0 < kc ? C - ci0 : kc) * taps) >> 2;
#pragma unroll
        for (int u = 0; u < RC_WREGS; ++u) {                                 // w[n0 + col][ci0 .. ci0 + kcw)[0 .. taps): contiguous
            const int i = tid + u * RC_THREADS;
            wr[u] = zero4;
            if (i < wn) {
                const int col = i / wq, q = i - col * wq;
                if (col < ncols && q < nq) wr[u] = *reinterpret_cast<const float4*>(a.w + ((long)(n0 + col) * C + ci0) * taps + 4 * q);
            }
        }
    };
    auto store_chunk = [&](int ci0, const float4 (&xr)[RC_XREGS], const float4 (&wr)[RC_WREGS]) {
#pragma unroll
        for (int u = 0; u < RC_XREGS; ++u) {
            const int i = tid + u * RC_THREADS;
            if (i < xn) {
                const int rr = i / kc4, c4 = i - rr * kc4;
                const float4 v = xr[u];
                float* s = Xs + rr * RC_XP + 4 * c4;
                s[0] = v.x; s[1] = v.y; s[2] = v.z; s[3] = v.w;
                const int ci = ci0 + 4 * c4;
                if (XM && a.x_masked && (MODE == RC_NORM || blockIdx.z == 0) && rr >= pad && rr < pad + rows && ci < C)
                    *reinterpret_cast<float4*>(a.x_masked + (row0 + rr - pad) * C + ci) = v;
            }
        }
#pragma unroll
        for (int u = 0; u < RC_WREGS; ++u) {
            const int i = tid + u * RC_THREADS;
            if (i < wn) {
                const int col = i / wq, q = i - col * wq;
                const float4 v = wr[u];
                float* s = Ws + col * RC_WP + 4 * q;
                s[0] = v.x; s[1] = v.y; s[2] = v.z; s[3] = v.w;
            }
        }
    };
    const float* xa = Xs + lr * RC_XP + half;
    const float* wb = Ws + ((has ? wave : 0) * 32 + lr) * RC_WP + half * taps;
    auto multiply = [&]() {
#pragma unroll
        for (int j = 0; j < taps; ++j)                                       // (a last, partial chunk multiplies the loader's zeros)
#pragma unroll
            for (int k = 0; k < kc; k += 2) {
                const float bv = wb[k * taps + j];
#pragma unroll
                for (int rt = 0; rt < RC_RT; ++rt)
                    if (rt * 32 < rows) acc[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[(rt * 32 + j) * RC_XP + k], bv, acc[rt], 0, 0, 0);
            }
        if (FOLD) {
#pragma unroll
            for (int rt = 0; rt < RC_RT; ++rt)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    tot[rt][i] = __fadd_rn(tot[rt][i], acc[rt][i]);
                    acc[rt][i] = 0.f;
                }
        }
    };
    load_chunk(0, xr0, wr0);
    if (kc < C) load_chunk(kc, xr1, wr1);
    for (int ci0 = 0; ci0 < C; ci0 += 2 * kc) {
        __syncthreads();
        store_chunk(ci0, xr0, wr0);
        __syncthreads();
        if (ci0 + 2 * kc < C) load_chunk(ci0 + 2 * kc, xr0, wr0);
        if (has) multiply();
        if (ci0 + kc >= C) break;
        __syncthreads();
        store_chunk(ci0 + kc, xr1, wr1);
        __syncthreads();
        if (ci0 + 3 * kc < C) load_chunk(ci0 + 3 * kc, xr1, wr1);
        if (has) multiply();
    }
    if (FOLD) {
#pragma unroll
        for (int rt = 0; rt < RC_RT; ++rt) acc[rt] = tot[rt];
    }

    const int c = n0 + wave * 32 + lr;                                       // this lane's column
    if (!NORM) {                                                             // plain: the length mask is the whole epilogue
        if (has && c < N) {
            const float b1 = MODE == RC_RELU ? a.bias[c] : 0.f;
            const float* aux = MODE == RC_GATE || MODE == RC_ADD ? a.aux + (long)b * a.aux_ld_batch + c : nullptr;
#pragma unroll
            for (int rt = 0; rt < RC_RT; ++rt)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int rr = rt * 32 + acc_row(i, half);
                    if (rr >= rows) continue;
                    float v = acc[rt][i];
                    if (MODE == RC_RELU) v = fmaxf(__fadd_rn(v, b1), 0.f);
                    if (MODE == RC_GATE || MODE == RC_ADD) {                 // aux at the output element, never behind the length
                        const float u = p0 + rr < pl ? aux[(long)(p0 + rr) * a.aux_ld_row] : 0.f;
                        v = MODE == RC_GATE ? (u > 0.f ? v : 0.f) : __fadd_rn(v, u);
                    }
                    a.y[(row0 + rr) * N + c] = p0 + rr < pl ? v : 0.f;
                }
        }
        return;
    }

    // NORM: N is a multiple of 32, so a block a wave has is whole
    const float bias = has ? a.bias[c] : 0.f;
    const uint64_t seed = site_seed(a.seed, a.step_seed);
    float val[RC_RT][16];
#pragma unroll
    for (int rt = 0; rt < RC_RT; ++rt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            float rv;
            if (MODE == RC_NORM) {
                rv = has ? fmaxf(__fadd_rn(acc[rt][i], bias), 0.f) : 0.f;
            } else {                                                         // s = x' + (z + b2) keep / (1 - p); rows behind the length: 0
                const int rr = rt * 32 + acc_row(i, half);
                rv = 0.f;
                if (has && p0 + rr < pl) {
                    float zv = __fadd_rn(acc[rt][i], bias);
                    if (a.drop_thr) zv = keep_elem(seed, (uint64_t)((row0 + rr) * N + c), a.drop_thr) ? __fmul_rn(zv, a.drop_scale) : 0.f;
                    rv = __fadd_rn(a.aux[(long)b * a.aux_ld_batch + (long)(p0 + rr) * a.aux_ld_row + c], zv);
                }
            }
            acc[rt][i] = rv;
            val[rt][i] = rv;
        }
    row_sums(val, red, stat[0], wave, lane);
    const float inv_n = 1.f / (float)N;
#pragma unroll
    for (int rt = 0; rt < RC_RT; ++rt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float d = has ? __fsub_rn(acc[rt][i], __fmul_rn(stat[0][rt * 32 + acc_row(i, half)], inv_n)) : 0.f;
            val[rt][i] = __fmul_rn(d, d);
        }
    row_sums(val, red, stat[1], wave, lane);
    const float gam = has ? a.gamma[c] : 0.f, bet = has ? a.beta[c] : 0.f;
#pragma unroll
    for (int rt = 0; rt < RC_RT; ++rt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int rr = rt * 32 + acc_row(i, half);
            if (rr >= rows) continue;
            const bool valid = p0 + rr < pl;
            const float m = __fmul_rn(stat[0][rr], inv_n);
            const float rs = 1.f / sqrtf(__fadd_rn(__fmul_rn(stat[1][rr], inv_n), a.eps));
            if (a.r && wave == 0 && lr == 0) {
                a.mean[row0 + rr] = valid ? m : 0.f;
                a.rstd[row0 + rr] = valid ? rs : 0.f;
            }
            if (!has) continue;
            const long at = (row0 + rr) * N + c;
            const float rv = acc[rt][i];
            float yv = __fmaf_rn(__fmul_rn(__fsub_rn(rv, m), rs), gam, bet);
            if (MODE == RC_NORM && a.drop_thr) yv = keep_elem(seed, (uint64_t)at, a.drop_thr) ? __fmul_rn(yv, a.drop_scale) : 0.f;
            a.y[at] = valid ? yv : 0.f;
            if (a.r) a.r[at] = valid ? rv : 0.f;
        }
}

// grid (ceil(Pmax / RB_ROWS), B): dz from dy, r, mean, rstd, gamma; the workgroup's column sums of g x_hat, g and dz go to
// part[(b * gridDim.x + tile) * 3 + k][N].  RES (the feed-forward sublayer: r is the LayerNorm's input s, no gate, the dropout sits
// on the branch): dz receives ds = the LayerNorm's input gradient, dz2 (NULL with drop_thr == 0: ds itself serves) ds keep / (1 -
// drop_p); two column sums (g x_hat, g) go to part[(b * gridDim.x + tile) * 2 + k][N].
template <bool RES>
__global__ __launch_bounds__(RB_THREADS) void ragged_norm_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ r,
                                                                     const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                     const float* __restrict__ gamma, const int64_t* __restrict__ lens,
                                                                     int Pmax, int N, float drop_scale, uint32_t drop_thr, uint64_t seed0,
                                                                     const uint64_t* __restrict__ step_seed, float* __restrict__ dz,
                                                                     float* __restrict__ dz2, float* __restrict__ part) {
    constexpr int NK = RES ? 2 : 3;
    __shared__ float wsum[4][3][RC_COLS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, p0 = blockIdx.x * RB_ROWS;
    const int pl = rc_clamp_len(lens[b], Pmax);
    const int rows = Pmax - p0 < RB_ROWS ? Pmax - p0 : RB_ROWS;
    const uint64_t seed = site_seed(seed0, step_seed);
    const float inv_n = 1.f / (float)N;
    float ga[4], sg[4], sb[4], sz[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + 64 * i;
        ga[i] = c < N ? gamma[c] : 0.f;
        sg[i] = sb[i] = sz[i] = 0.f;
    }
    for (int rr = wave; rr < rows; rr += 4) {
        const int p = p0 + rr;
        const long base = ((long)b * Pmax + p) * N;
        if (p >= pl) {                                                       // behind the length: zeros, nothing read
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (lane + 64 * i < N) {
                    dz[base + lane + 64 * i] = 0.f;
                    if (RES && dz2) dz2[base + lane + 64 * i] = 0.f;
                }
            continue;
        }
        const float m = mean[(long)b * Pmax + p], rs = rstd[(long)b * Pmax + p];
        float rv[4], xh[4], gg[4], s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = lane + 64 * i;
            rv[i] = xh[i] = gg[i] = 0.f;
            if (c < N) {
                float g = dy[base + c];
                if (!RES && drop_thr) g = keep_elem(seed, (uint64_t)(base + c), drop_thr) ? __fmul_rn(g, drop_scale) : 0.f;
                rv[i] = r[base + c];
                xh[i] = __fmul_rn(__fsub_rn(rv[i], m), rs);
                sg[i] = __fmaf_rn(g, xh[i], sg[i]);
                sb[i] = __fadd_rn(sb[i], g);
                gg[i] = __fmul_rn(g, ga[i]);
                s1 = __fadd_rn(s1, gg[i]);
                s2 = __fmaf_rn(gg[i], xh[i], s2);
            }
        }
        const float m1 = __fmul_rn(wave_sum(s1), inv_n), m2 = __fmul_rn(wave_sum(s2), inv_n);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = lane + 64 * i;
            if (c < N) {
                const float dr = __fmul_rn(rs, __fsub_rn(__fsub_rn(gg[i], m1), __fmul_rn(xh[i], m2)));
                const float d = RES || rv[i] > 0.f ? dr : 0.f;
                sz[i] = __fadd_rn(sz[i], d);
                dz[base + c] = d;
                if (RES && dz2) dz2[base + c] = keep_elem(seed, (uint64_t)(base + c), drop_thr) ? __fmul_rn(d, drop_scale) : 0.f;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        wsum[wave][0][lane + 64 * i] = sg[i];
        wsum[wave][1][lane + 64 * i] = sb[i];
        wsum[wave][2][lane + 64 * i] = sz[i];
    }
    __syncthreads();
    float* out = part + ((long)b * gridDim.x + blockIdx.x) * NK * N;
    for (int t = tid; t < NK * N; t += RB_THREADS) {
        const int k = t / N, c = t - k * N;
        out[t] = __fadd_rn(__fadd_rn(__fadd_rn(wsum[0][k][c], wsum[1][k][c]), wsum[2][k][c]), wsum[3][k][c]);
    }
}

// out_k[c] (+)= the sum of the nwg workgroups' partials: slice s of RF_SLICES adds the workgroups [s nwg / 8, (s + 1) nwg / 8) in
// ascending order, then the slices are added in ascending order.  A workgroup owns 32 of the nk N (k, c) pairs (nk = 3, or 2: no dbias).
__global__ __launch_bounds__(RB_THREADS) void ragged_norm_bwd_finish_kernel(const float* __restrict__ part, int nwg, int N, int nk,
                                                                            float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                            float* __restrict__ dbias, int accumulate) {
    __shared__ float sl[RF_SLICES][32];
    const int col = threadIdx.x & 31, slice = threadIdx.x >> 5;
    const int t = blockIdx.x * 32 + col;                                     // nk N is a multiple of 32
    const int g0 = (int)((long)slice * nwg / RF_SLICES), g1 = (int)((long)(slice + 1) * nwg / RF_SLICES);
    float s = 0.f;
    int g = g0;
    for (; g + 4 <= g1; g += 4) {                                            // four loads in flight, added in ascending order
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = part[(long)(g + u) * nk * N + t];
#pragma unroll
        for (int u = 0; u < 4; ++u) s = __fadd_rn(s, v[u]);
    }
    for (; g < g1; ++g) s = __fadd_rn(s, part[(long)g * nk * N + t]);
    sl[slice][col] = s;
    __syncthreads();
    if (slice != 0) return;
    s = sl[0][col];
#pragma unroll
    for (int v = 1; v < RF_SLICES; ++v) s = __fadd_rn(s, sl[v][col]);
    const int k = t / N, c = t - k * N;
    float* out = k == 0 ? dgamma : k == 1 ? dbeta : dbias;
    out[c] = accumulate ? __fadd_rn(out[c], s) : s;
}

// wt[ci][co][j] = w[co][ci][taps - 1 - j]: the weight of the convolution that takes dz to dx
__global__ __launch_bounds__(RB_THREADS) void ragged_conv_flip_weight_kernel(const float* __restrict__ w, float* __restrict__ wt, int cout,
                                                                             int cin, int taps) {
    const long total = (long)cout * cin * taps;
    for (long i = (long)blockIdx.x * RB_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * RB_THREADS) {
        const int j = (int)(i % taps);
        const long rest = i / taps;
        const int co = (int)(rest % cout), ci = (int)(rest / cout);
        wt[i] = w[((long)co * cin + ci) * taps + (taps - 1 - j)];
    }
}

template <int MODE>
static void launch_ragged_conv(int taps, dim3 grid, hipStream_t stream, const RaggedConvArgs& a) {
    switch (taps) {
        case 1: hipLaunchKernelGGL((ragged_conv_kernel<MODE, 1>), grid, dim3(RC_THREADS), 0, stream, a); break;
        case 3: hipLaunchKernelGGL((ragged_conv_kernel<MODE, 3>), grid, dim3(RC_THREADS), 0, stream, a); break;
        case 5: hipLaunchKernelGGL((ragged_conv_kernel<MODE, 5>), grid, dim3(RC_THREADS), 0, stream, a); break;
        case 7: hipLaunchKernelGGL((ragged_conv_kernel<MODE, 7>), grid, dim3(RC_THREADS), 0, stream, a); break;
        default: hipLaunchKernelGGL((ragged_conv_kernel<MODE, 9>), grid, dim3(RC_THREADS), 0, stream, a); break;
    }
}

static inline bool rc_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
static inline size_t rc_round4(size_t n) { return (n + 3) & ~(size_t)3; }

struct RaggedWs { size_t dz, wt, part, wgrad, floats; };
static RaggedWs ragged_ws_layout(int B, int Pmax, int Cin, int Cout, int taps) {
    RaggedWs l;
    l.dz = 0;
    l.wt = l.dz + rc_round4((size_t)B * Pmax * Cout);
    l.part = l.wt + rc_round4((size_t)Cin * Cout * taps);
    l.wgrad = l.part + rc_round4((size_t)B * cdiv(Pmax, RB_ROWS) * 3 * Cout);
    l.floats = l.wgrad + rc_round4(ttts_wgrad_workspace_bytes((int64_t)B * Pmax, Cout, Cin, taps) / sizeof(float) + 1);
    return l;
}

// the feed-forward sublayer's backward: ds and dz2 (B, Pmax, D), dz1 (B, Pmax, Chid), one flipped weight at a time, the row
// kernel's partials, one weight gradient's workspace at a time
struct FfnWs { size_t ds, dz2, dz1, wt, part, wgrad, wgrad_bytes, floats; };
static FfnWs ffn_ws_layout(int B, int Pmax, int D, int Chid, int k1, int k2) {
    FfnWs l;
    const size_t w1 = ttts_wgrad_workspace_bytes((int64_t)B * Pmax, Chid, D, k1), w2 = ttts_wgrad_workspace_bytes((int64_t)B * Pmax, D, Chid, k2);
    l.ds = 0;
    l.dz2 = l.ds + rc_round4((size_t)B * Pmax * D);
    l.dz1 = l.dz2 + rc_round4((size_t)B * Pmax * D);
    l.wt = l.dz1 + rc_round4((size_t)B * Pmax * Chid);
    l.part = l.wt + rc_round4((size_t)D * Chid * (k1 > k2 ? k1 : k2));
    l.wgrad = l.part + rc_round4((size_t)B * cdiv(Pmax, RB_ROWS) * 2 * D);
    l.wgrad_bytes = w1 > w2 ? w1 : w2;
    l.floats = l.wgrad + rc_round4(l.wgrad_bytes / sizeof(float) + 1);
    return l;
}

}  // namespace ttts

using namespace ttts;

#define RC_REQUIRE_SHAPE(name)                                                                                                   \
    TTTS_REQUIRE(B >= 1 && B <= 65535, "%s: B must be in [1, 65535] (one grid row per utterance), got %d", name, B);             \
    TTTS_REQUIRE(Pmax >= 1 && Pmax <= RC_MAX_P, "%s: Pmax must be in [1, %d] phonemes, got %d", name, RC_MAX_P, Pmax);           \
    TTTS_REQUIRE(Cin >= 4 && Cin <= RC_MAX_CIN && Cin % 4 == 0, "%s: Cin must be a multiple of 4 in [4, %d], got %d", name,      \
                 RC_MAX_CIN, Cin);                                                                                               \
    TTTS_REQUIRE(Cout >= 32 && Cout <= RC_COLS && Cout % 32 == 0, "%s: Cout must be a multiple of 32 in [32, %d], got %d", name, \
                 RC_COLS, Cout);                                                                                                 \
    TTTS_REQUIRE(taps >= 1 && taps <= RC_MAX_TAPS && (taps & 1), "%s: taps must be odd in [1, %d], got %d", name, RC_MAX_TAPS, taps); \
    TTTS_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "%s: drop_p must be in [0, 1), got %g", name, (double)drop_p)

extern "C" {

int ttts_ragged_conv_norm_fwd(const float* x, int64_t ld_row, int64_t ld_batch, const int64_t* lens, const float* w, const float* bias,
                              const float* gamma, const float* beta, int B, int Pmax, int Cin, int Cout, int taps, float eps,
                              float drop_p, uint64_t seed, const uint64_t* step_seed, float* y, float* r, float* mean, float* rstd,
                              float* x_masked, void* stream) {
    const char* name = "ragged_conv_norm_fwd";
    TTTS_REQUIRE(x && lens && w && bias && gamma && beta && y, "%s: null pointer", name);
    TTTS_REQUIRE((r && mean && rstd) || (!r && !mean && !rstd), "%s: null pointer (r, mean and rstd go together: all three or none)", name);
    RC_REQUIRE_SHAPE(name);
    TTTS_REQUIRE(eps > 0.f && eps - eps == 0.f, "%s: eps must be positive and finite, got %g", name, (double)eps);
    TTTS_REQUIRE(ld_row >= Cin && ld_row % 4 == 0, "%s: the row stride must be a multiple of 4 and >= Cin (ld_row %lld, Cin %d)", name,
                 (long long)ld_row, Cin);
    TTTS_REQUIRE((B == 1 && ld_batch >= 0) || (ld_batch % 4 == 0 && ld_batch >= (int64_t)(Pmax - 1) * ld_row + Cin),
                 "%s: the batch stride must be a multiple of 4 and cover an utterance (ld_batch %lld, ld_row %lld, Pmax %d, Cin %d)", name,
                 (long long)ld_batch, (long long)ld_row, Pmax, Cin);
    TTTS_REQUIRE(rc_aligned(x, 16) && rc_aligned(w, 16) && rc_aligned(y, 16) && rc_aligned(r, 16) && rc_aligned(x_masked, 16),
                 "%s: x, w, y, r and x_masked must be 16-byte aligned", name);
    TTTS_REQUIRE(rc_aligned(bias, 4) && rc_aligned(gamma, 4) && rc_aligned(beta, 4) && rc_aligned(mean, 4) && rc_aligned(rstd, 4),
                 "%s: bias, gamma, beta, mean and rstd must be 4-byte aligned", name);
    TTTS_REQUIRE(rc_aligned(lens, 8) && rc_aligned(step_seed, 8), "%s: lens and step_seed must be 8-byte aligned", name);
    RaggedConvArgs a;
    a.x = x; a.ld_row = (long)ld_row; a.ld_batch = (long)ld_batch; a.lens = lens; a.w = w; a.bias = bias; a.gamma = gamma; a.beta = beta;
    a.Pmax = Pmax; a.C = Cin; a.N = Cout;
    a.eps = eps; a.drop_thr = drop_p > 0.f ? drop_threshold(drop_p) : 0u; a.drop_scale = 1.f / (1.f - drop_p);
    a.seed = seed; a.step_seed = step_seed;
    a.y = y; a.r = r; a.mean = mean; a.rstd = rstd; a.x_masked = x_masked;
    const dim3 grid((unsigned)cdiv(Pmax, RC_ROWS), (unsigned)B, 1u);
    launch_ragged_conv<RC_NORM>(taps, grid, (hipStream_t)stream, a);
    TTTS_LAUNCH_CHECK("ragged_conv_kernel<norm>");
    return TTTS_OK;
}

size_t ttts_ragged_conv_norm_workspace_bytes(int B, int Pmax, int Cin, int Cout, int taps) {
    if (!(B > 0 && Pmax > 0 && Cin > 0 && Cout > 0 && taps > 0)) return 0;
    return ragged_ws_layout(B, Pmax, Cin, Cout, taps).floats * sizeof(float);
}

int ttts_ragged_conv_norm_bwd(const float* dy, const float* r, const float* mean, const float* rstd, const float* x_masked,
                              const int64_t* lens, const float* w, const float* gamma, int B, int Pmax, int Cin, int Cout, int taps,
                              float drop_p, uint64_t seed, const uint64_t* step_seed, float* dx, float* dw, float* dbias,
                              float* dgamma, float* dbeta, float* ws, size_t ws_bytes, int accumulate, void* stream_) {
    const char* name = "ragged_conv_norm_bwd";
    hipStream_t stream = (hipStream_t)stream_;
    TTTS_REQUIRE(dy && r && mean && rstd && lens && w && gamma && dbias && dgamma && dbeta && ws, "%s: null pointer", name);
    TTTS_REQUIRE(!dw || x_masked, "%s: null pointer (the weight gradient needs x_masked)", name);
    RC_REQUIRE_SHAPE(name);
    TTTS_REQUIRE(rc_aligned(dy, 16) && rc_aligned(r, 16) && rc_aligned(x_masked, 16) && rc_aligned(w, 16) && rc_aligned(dx, 16) &&
                     rc_aligned(dw, 16) && rc_aligned(ws, 16),
                 "%s: dy, r, x_masked, w, dx, dw and ws must be 16-byte aligned", name);
    TTTS_REQUIRE(rc_aligned(mean, 4) && rc_aligned(rstd, 4) && rc_aligned(gamma, 4) && rc_aligned(dbias, 4) && rc_aligned(dgamma, 4) &&
                     rc_aligned(dbeta, 4),
                 "%s: mean, rstd, gamma, dbias, dgamma and dbeta must be 4-byte aligned", name);
    TTTS_REQUIRE(rc_aligned(lens, 8) && rc_aligned(step_seed, 8), "%s: lens and step_seed must be 8-byte aligned", name);
    const RaggedWs l = ragged_ws_layout(B, Pmax, Cin, Cout, taps);
    TTTS_REQUIRE(ws_bytes >= l.floats * sizeof(float), "%s: workspace too small (%zu bytes, need %zu)", name, ws_bytes,
                 l.floats * sizeof(float));
    float* dz = ws + l.dz;
    float* part = ws + l.part;
    const int tiles = cdiv(Pmax, RB_ROWS);
    hipLaunchKernelGGL(ragged_norm_bwd_kernel<false>, dim3((unsigned)tiles, (unsigned)B), dim3(RB_THREADS), 0, stream, dy, r, mean, rstd,
                       gamma, lens, Pmax, Cout, 1.f / (1.f - drop_p), drop_p > 0.f ? drop_threshold(drop_p) : 0u, seed, step_seed, dz,
                       (float*)nullptr, part);
    TTTS_LAUNCH_CHECK("ragged_norm_bwd_kernel");
    hipLaunchKernelGGL(ragged_norm_bwd_finish_kernel, dim3((unsigned)(3 * Cout / 32)), dim3(RB_THREADS), 0, stream, part,
                       tiles * B, Cout, 3, dgamma, dbeta, dbias, accumulate);
    TTTS_LAUNCH_CHECK("ragged_norm_bwd_finish_kernel");
    if (dx) {
        float* wt = ws + l.wt;
        const long total = (long)Cin * Cout * taps;
        hipLaunchKernelGGL(ragged_conv_flip_weight_kernel, dim3((unsigned)(cdiv(total, RB_THREADS) > 1024 ? 1024 : cdiv(total, RB_THREADS))),
                           dim3(RB_THREADS), 0, stream, w, wt, Cout, Cin, taps);
        TTTS_LAUNCH_CHECK("ragged_conv_flip_weight_kernel");
        RaggedConvArgs a;
        a.x = dz; a.ld_row = Cout; a.ld_batch = (long)Pmax * Cout; a.lens = lens; a.w = wt; a.bias = nullptr; a.gamma = nullptr; a.beta = nullptr;
        a.Pmax = Pmax; a.C = Cout; a.N = Cin;
        a.eps = 0.f; a.drop_thr = 0u; a.drop_scale = 1.f; a.seed = 0; a.step_seed = nullptr;
        a.y = dx; a.r = nullptr; a.mean = nullptr; a.rstd = nullptr; a.x_masked = nullptr;
        const dim3 grid((unsigned)cdiv(Pmax, RC_ROWS), (unsigned)B, (unsigned)cdiv(Cin, RC_COLS));
        launch_ragged_conv<RC_PLAIN>(taps, grid, stream, a);
        TTTS_LAUNCH_CHECK("ragged_conv_kernel<plain>");
    }
    if (dw) {
        const size_t wbytes = ttts_wgrad_workspace_bytes((int64_t)B * Pmax, Cout, Cin, taps);
        const int rc = ttts_conv1d_bwd_weight(dz, x_masked, dw, nullptr, ws + l.wgrad, wbytes, B, Pmax, Cin, Cout, taps, accumulate, nullptr,
                                              stream_);
        if (rc) return rc;
    }
    return TTTS_OK;
}

}  // extern "C"

#define FFN_REQUIRE_SHAPE(name)                                                                                                  \
    TTTS_REQUIRE(B >= 1 && B <= 65535, "%s: B must be in [1, 65535] (one grid row per utterance), got %d", name, B);             \
    TTTS_REQUIRE(Pmax >= 1 && Pmax <= RC_MAX_P, "%s: Pmax must be in [1, %d] rows, got %d", name, RC_MAX_P, Pmax);               \
    TTTS_REQUIRE(D >= 32 && D <= RC_COLS && D % 32 == 0, "%s: D must be a multiple of 32 in [32, %d], got %d", name, RC_COLS, D); \
    TTTS_REQUIRE(Chid >= 32 && Chid <= RC_MAX_CIN && Chid % 32 == 0, "%s: Chid must be a multiple of 32 in [32, %d], got %d", name, \
                 RC_MAX_CIN, Chid);                                                                                              \
    TTTS_REQUIRE(k1 >= 1 && k1 <= RC_MAX_TAPS && (k1 & 1), "%s: k1 must be odd in [1, %d], got %d", name, RC_MAX_TAPS, k1);       \
    TTTS_REQUIRE(k2 >= 1 && k2 <= RC_MAX_TAPS && (k2 & 1), "%s: k2 must be odd in [1, %d], got %d", name, RC_MAX_TAPS, k2);       \
    TTTS_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "%s: drop_p must be in [0, 1), got %g", name, (double)drop_p)

extern "C" {

int ttts_ragged_conv_ffn_fwd(const float* x, int64_t ld_row, int64_t ld_batch, const int64_t* lens, const float* w1, const float* b1,
                             const float* w2, const float* b2, const float* gamma, const float* beta, int B, int Pmax, int D, int Chid,
                             int k1, int k2, float eps, float drop_p, uint64_t seed, const uint64_t* step_seed, float* h, float* y,
                             float* s, float* mean, float* rstd, float* x_masked, void* stream) {
    const char* name = "ragged_conv_ffn_fwd";
    TTTS_REQUIRE(x && lens && w1 && b1 && w2 && b2 && gamma && beta && h && y, "%s: null pointer", name);
    TTTS_REQUIRE((s && mean && rstd) || (!s && !mean && !rstd), "%s: null pointer (s, mean and rstd go together: all three or none)", name);
    FFN_REQUIRE_SHAPE(name);
    TTTS_REQUIRE(eps > 0.f && eps - eps == 0.f, "%s: eps must be positive and finite, got %g", name, (double)eps);
    TTTS_REQUIRE(ld_row >= D && ld_row % 4 == 0, "%s: the row stride must be a multiple of 4 and >= D (ld_row %lld, D %d)", name,
                 (long long)ld_row, D);
    TTTS_REQUIRE((B == 1 && ld_batch >= 0) || (ld_batch % 4 == 0 && ld_batch >= (int64_t)(Pmax - 1) * ld_row + D),
                 "%s: the batch stride must be a multiple of 4 and cover an utterance (ld_batch %lld, ld_row %lld, Pmax %d, D %d)", name,
                 (long long)ld_batch, (long long)ld_row, Pmax, D);
    TTTS_REQUIRE(rc_aligned(x, 16) && rc_aligned(w1, 16) && rc_aligned(w2, 16) && rc_aligned(h, 16) && rc_aligned(y, 16) && rc_aligned(s, 16) &&
                     rc_aligned(x_masked, 16),
                 "%s: x, w1, w2, h, y, s and x_masked must be 16-byte aligned", name);
    TTTS_REQUIRE(rc_aligned(b1, 4) && rc_aligned(b2, 4) && rc_aligned(gamma, 4) && rc_aligned(beta, 4) && rc_aligned(mean, 4) && rc_aligned(rstd, 4),
                 "%s: b1, b2, gamma, beta, mean and rstd must be 4-byte aligned", name);
    TTTS_REQUIRE(rc_aligned(lens, 8) && rc_aligned(step_seed, 8), "%s: lens and step_seed must be 8-byte aligned", name);
    RaggedConvArgs a;
    a.x = x; a.ld_row = (long)ld_row; a.ld_batch = (long)ld_batch; a.lens = lens; a.w = w1; a.bias = b1; a.gamma = nullptr; a.beta = nullptr;
    a.Pmax = Pmax; a.C = D; a.N = Chid;
    a.eps = eps; a.drop_thr = 0u; a.drop_scale = 1.f; a.seed = 0; a.step_seed = nullptr;
    a.y = h; a.r = nullptr; a.mean = nullptr; a.rstd = nullptr; a.x_masked = x_masked;
    launch_ragged_conv<RC_RELU>(k1, dim3((unsigned)cdiv(Pmax, RC_ROWS), (unsigned)B, (unsigned)cdiv(Chid, RC_COLS)), (hipStream_t)stream, a);
    TTTS_LAUNCH_CHECK("ragged_conv_kernel<relu>");
    a.x = h; a.ld_row = Chid; a.ld_batch = (long)Pmax * Chid; a.w = w2; a.bias = b2; a.gamma = gamma; a.beta = beta;
    a.C = Chid; a.N = D;
    a.drop_thr = drop_p > 0.f ? drop_threshold(drop_p) : 0u; a.drop_scale = 1.f / (1.f - drop_p); a.seed = seed; a.step_seed = step_seed;
    a.y = y; a.r = s; a.mean = mean; a.rstd = rstd; a.x_masked = nullptr;
    a.aux = x; a.aux_ld_row = (long)ld_row; a.aux_ld_batch = (long)ld_batch;
    launch_ragged_conv<RC_RESNORM>(k2, dim3((unsigned)cdiv(Pmax, RC_ROWS), (unsigned)B, 1u), (hipStream_t)stream, a);
    TTTS_LAUNCH_CHECK("ragged_conv_kernel<resnorm>");
    return TTTS_OK;
}

size_t ttts_ragged_conv_ffn_workspace_bytes(int B, int Pmax, int D, int Chid, int k1, int k2) {
    if (!(B > 0 && Pmax > 0 && D > 0 && Chid > 0 && k1 > 0 && k2 > 0)) return 0;
    return ffn_ws_layout(B, Pmax, D, Chid, k1, k2).floats * sizeof(float);
}

int ttts_ragged_conv_ffn_bwd(const float* dy, const float* s, const float* mean, const float* rstd, const float* h, const float* x_masked,
                             const int64_t* lens, const float* w1, const float* w2, const float* gamma, int B, int Pmax, int D, int Chid,
                             int k1, int k2, float drop_p, uint64_t seed, const uint64_t* step_seed, float* dx, float* dw1, float* db1,
                             float* dw2, float* db2, float* dgamma, float* dbeta, float* ws, size_t ws_bytes, int accumulate,
                             void* stream_) {
    const char* name = "ragged_conv_ffn_bwd";
    hipStream_t stream = (hipStream_t)stream_;
    TTTS_REQUIRE(dy && s && mean && rstd && h && lens && w1 && w2 && gamma && dgamma && dbeta && ws, "%s: null pointer", name);
    TTTS_REQUIRE((dw1 && db1 && dw2 && db2) || (!dw1 && !db1 && !dw2 && !db2),
                 "%s: null pointer (dw1, db1, dw2 and db2 go together: all four or none)", name);
    TTTS_REQUIRE(!dw1 || x_masked, "%s: null pointer (the weight gradient needs x_masked)", name);
    FFN_REQUIRE_SHAPE(name);
    TTTS_REQUIRE(!dw1 || (uint64_t)B * Pmax * (Chid > D ? Chid : D) * 4 < (1ull << 32),
                 "%s: the weight gradient takes operands below 4 GiB (B %d, Pmax %d, D %d, Chid %d)", name, B, Pmax, D, Chid);
    TTTS_REQUIRE(rc_aligned(dy, 16) && rc_aligned(s, 16) && rc_aligned(h, 16) && rc_aligned(x_masked, 16) && rc_aligned(w1, 16) &&
                     rc_aligned(w2, 16) && rc_aligned(dx, 16) && rc_aligned(dw1, 16) && rc_aligned(dw2, 16) && rc_aligned(ws, 16),
                 "%s: dy, s, h, x_masked, w1, w2, dx, dw1, dw2 and ws must be 16-byte aligned", name);
    TTTS_REQUIRE(rc_aligned(mean, 4) && rc_aligned(rstd, 4) && rc_aligned(gamma, 4) && rc_aligned(db1, 4) && rc_aligned(db2, 4) &&
                     rc_aligned(dgamma, 4) && rc_aligned(dbeta, 4),
                 "%s: mean, rstd, gamma, db1, db2, dgamma and dbeta must be 4-byte aligned", name);
    TTTS_REQUIRE(rc_aligned(lens, 8) && rc_aligned(step_seed, 8), "%s: lens and step_seed must be 8-byte aligned", name);
    const FfnWs l = ffn_ws_layout(B, Pmax, D, Chid, k1, k2);
    TTTS_REQUIRE(ws_bytes >= l.floats * sizeof(float), "%s: workspace too small (%zu bytes, need %zu)", name, ws_bytes,
                 l.floats * sizeof(float));
    float* ds = ws + l.ds;
    float* dz2 = drop_p > 0.f ? ws + l.dz2 : ds;                             // without dropout ds is the branch's gradient too
    float* dz1 = ws + l.dz1;
    float* wt = ws + l.wt;
    float* part = ws + l.part;
    const int tiles = cdiv(Pmax, RB_ROWS);
    hipLaunchKernelGGL(ragged_norm_bwd_kernel<true>, dim3((unsigned)tiles, (unsigned)B), dim3(RB_THREADS), 0, stream, dy, s, mean, rstd, gamma,
                       lens, Pmax, D, 1.f / (1.f - drop_p), drop_p > 0.f ? drop_threshold(drop_p) : 0u, seed, step_seed, ds,
                       drop_p > 0.f ? dz2 : (float*)nullptr, part);
    TTTS_LAUNCH_CHECK("ragged_norm_bwd_kernel<res>");
    hipLaunchKernelGGL(ragged_norm_bwd_finish_kernel, dim3((unsigned)(2 * D / 32)), dim3(RB_THREADS), 0, stream, part, tiles * B, D, 2, dgamma,
                       dbeta, (float*)nullptr, accumulate);
    TTTS_LAUNCH_CHECK("ragged_norm_bwd_finish_kernel");
    if (!dx && !dw1) return TTTS_OK;
    if (dw2) {
        const int rc = ttts_conv1d_bwd_weight(dz2, h, dw2, db2, ws + l.wgrad, l.wgrad_bytes, B, Pmax, Chid, D, k2, accumulate, nullptr, stream_);
        if (rc) return rc;
    }
    auto flip = [&](const float* w, int cout, int cin, int taps) {
        const long total = (long)cin * cout * taps;
        hipLaunchKernelGGL(ragged_conv_flip_weight_kernel, dim3((unsigned)(cdiv(total, RB_THREADS) > 1024 ? 1024 : cdiv(total, RB_THREADS))),
                           dim3(RB_THREADS), 0, stream, w, wt, cout, cin, taps);
    };
    RaggedConvArgs a;
    a.lens = lens; a.w = wt; a.bias = nullptr; a.gamma = nullptr; a.beta = nullptr; a.Pmax = Pmax;
    a.eps = 0.f; a.drop_thr = 0u; a.drop_scale = 1.f; a.seed = 0; a.step_seed = nullptr;
    a.r = nullptr; a.mean = nullptr; a.rstd = nullptr; a.x_masked = nullptr;
    flip(w2, D, Chid, k2);                                                   // dz1 = conv(dz2, flipped w2) [h > 0]
    TTTS_LAUNCH_CHECK("ragged_conv_flip_weight_kernel");
    a.x = dz2; a.ld_row = D; a.ld_batch = (long)Pmax * D; a.C = D; a.N = Chid;
    a.y = dz1; a.aux = h; a.aux_ld_row = Chid; a.aux_ld_batch = (long)Pmax * Chid;
    launch_ragged_conv<RC_GATE>(k2, dim3((unsigned)cdiv(Pmax, RC_ROWS), (unsigned)B, (unsigned)cdiv(Chid, RC_COLS)), stream, a);
    TTTS_LAUNCH_CHECK("ragged_conv_kernel<gate>");
    if (dw1) {
        const int rc = ttts_conv1d_bwd_weight(dz1, x_masked, dw1, db1, ws + l.wgrad, l.wgrad_bytes, B, Pmax, D, Chid, k1, accumulate, nullptr,
                                              stream_);
        if (rc) return rc;
    }
    if (dx) {
        flip(w1, Chid, D, k1);                                               // dx = conv(dz1, flipped w1) + ds
        TTTS_LAUNCH_CHECK("ragged_conv_flip_weight_kernel");
        a.x = dz1; a.ld_row = Chid; a.ld_batch = (long)Pmax * Chid; a.C = Chid; a.N = D;
        a.y = dx; a.aux = ds; a.aux_ld_row = D; a.aux_ld_batch = (long)Pmax * D;
        launch_ragged_conv<RC_ADD>(k1, dim3((unsigned)cdiv(Pmax, RC_ROWS), (unsigned)B, 1u), stream, a);
        TTTS_LAUNCH_CHECK("ragged_conv_kernel<add>");
    }
    return TTTS_OK;
}

}  // extern "C"
