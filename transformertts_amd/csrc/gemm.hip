// fp32 MFMA GEMM family for gfx950: linear / 1x1-conv FFN / k-tap Conv1d as implicit GEMM,
// forward (x.W^T), data-gradient (dy.W) and weight-gradient (dy^T.x, split over rows).
//
// One workgroup = 4 waves (256 threads) computes a BM x BN tile with v_mfma_f32_32x32x2_f32
// (exact fp32, k-ordered fma chain).  Operand tiles are staged global -> registers -> LDS
// (double-buffered, one barrier per 16-deep k-tile); each wave owns a (BM/WM) x (BN/WN) sub-tile
// made of 32x32 MFMA accumulators.
//
// Operand addressing modes (template flags):
//   A_KC  : A is [M][K] row-major, K contiguous ("activation rows").  Supports an implicit
//           im2col: K = taps*cin, k-tile -> (tap, channel block), source row = m + shift(tap),
//           zero outside the utterance [0,T) the row belongs to.  This serves Conv1d forward,
//           Conv1d data-gradient (flipped taps) and the decoder's go-frame shift (one tap, shift -1).
//   !A_KC : A is stored [K][M] (reduction index is the row) -- dy^T for weight gradients.
//   B_KC  : B is [N][K] row-major, K contiguous (nn.Linear weight layout, packed conv weight).
//   !B_KC : B is stored [K][N] (reduction index is the row) -- W for data-gradients, x for weight
//           gradients (with the same per-tap row shift / utterance clipping as above).
#include <stdlib.h>

#include "gemm_common.h"

namespace ttts {

#ifndef TTTS_GEMM_BK
#define TTTS_GEMM_BK 16
#endif
#ifndef TTTS_X6_XCD
#define TTTS_X6_XCD 1
#endif
#ifndef TTTS_GEMM_MINWAVES
#define TTTS_GEMM_MINWAVES 3
#endif
constexpr int BK = TTTS_GEMM_BK;          // k-tile depth (floats)
constexpr int KC_LD = BK + 1;   // LDS row stride for K-contiguous tiles (odd -> conflict-free b32 reads)


template <int BM, int BN, int WM, int WN, bool A_KC, bool B_KC>
__global__ __launch_bounds__(256, TTTS_GEMM_MINWAVES) void gemm_f32_kernel(GemmArgs g) {
    const uint64_t seed_eff = site_seed(g.seed, g.step_seed);
    constexpr int WTM = BM / WM, WTN = BN / WN;
    constexpr int TM = WTM / 32, TN = WTN / 32;
    static_assert(WM * WN == 4, "4 waves per workgroup");
    static_assert(WTM % 32 == 0 && WTN % 32 == 0, "wave tile must be a multiple of 32x32");
    constexpr int A_ELEMS = A_KC ? BM * KC_LD : BK * BM;
    constexpr int B_ELEMS = B_KC ? BN * KC_LD : BK * BN;
    constexpr int NLA = (BM * 4 + 255) / 256;   // float4 loads per thread for the A tile
    constexpr int NLB = (BN * 4 + 255) / 256;

    __shared__ __attribute__((aligned(16))) float lds[2 * (A_ELEMS + B_ELEMS)];
    constexpr int STAGE = A_ELEMS + B_ELEMS;   // stage `buf`: A at lds + buf*STAGE, B right behind it

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const int wm = wave / WN, wn = wave % WN;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    const int z = blockIdx.z;
    const int ztap = (g.ztaps > 1) ? (z % g.ztaps) : 0;
    const int zsplit = (g.ztaps > 1) ? (z / g.ztaps) : z;

    const int nkt = g.K / BK + ((g.K % BK) ? 1 : 0);
    const int kt_begin = zsplit * g.kt_per_split;
    int kt_end = kt_begin + g.kt_per_split;
    if (kt_end > nkt) kt_end = nkt;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const __amdgpu_buffer_rsrc_t rsrcA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.A), 0, g.a_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrcB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.B), 0, g.b_bytes, 0x00020000);

    float4 ra[NLA], rb[NLB];
    float4 csum[NLA];   // running sum of this thread's A elements over the k-tiles (bias gradient, !A_KC form)
#pragma unroll
    for (int i = 0; i < NLA; ++i) csum[i] = make_float4(0.f, 0.f, 0.f, 0.f);

    // ---- per-thread static parts of the loaders: byte offsets of this thread's float4s at k-tile 0
    // K-contiguous tiles: thread -> (row = idx>>2, chunk = idx&3); natural tiles: (krow = idx / (X/4), col4)
    int a_t[NLA];          // A_KC: t index of the row inside its utterance (for shift clipping)
    uint32_t a_off[NLA];   // OOB when the row / column is outside the matrix
    uint32_t b_off[NLB];
#pragma unroll
    for (int i = 0; i < NLA; ++i) {
        int idx = tid + i * 256;
        if (A_KC) {
            int row = idx >> 2, ch = idx & 3;
            int m = m0 + row;
            a_off[i] = (row < BM && m < g.M) ? (uint32_t)(((long)m * g.lda + ch * 4) * 4) : OOB;
            a_t[i] = (g.T > 0) ? (m % g.T) : 0;
        } else {
            int kr = idx / (BM / 4), c4 = idx % (BM / 4);
            int m = m0 + c4 * 4;
            a_off[i] = (idx < BK * (BM / 4) && m < g.M) ? (uint32_t)(((long)kr * g.lda + m) * 4) : OOB;
            a_t[i] = kr;
        }
    }
#pragma unroll
    for (int i = 0; i < NLB; ++i) {
        int idx = tid + i * 256;
        if (B_KC) {
            int row = idx >> 2, ch = idx & 3;
            int n = n0 + row;
            b_off[i] = (row < BN && n < g.N) ? (uint32_t)(((long)n * g.ldb + ch * 4) * 4) : OOB;
        } else {
            int kr = idx / (BN / 4), c4 = idx % (BN / 4);
            int n = n0 + c4 * 4;
            b_off[i] = (idx < BK * (BN / 4) && n < g.N) ? (uint32_t)(((long)kr * g.ldb + n) * 4) : OOB;
        }
    }

    auto load_tiles = [&](int kt) {
        const int k0 = kt * BK;
        // ---------------- A
        if (A_KC) {
            const int tap = k0 / g.cin;
            const int c0 = k0 - tap * g.cin;
            const int shift = g.shift0 + tap * g.shift_step;
            const uint32_t koff = (uint32_t)(((long)shift * g.lda + c0) * 4);
#pragma unroll
            for (int i = 0; i < NLA; ++i) {
                bool ok = a_off[i] != OOB;
                if (g.T > 0) ok = ok && ((unsigned)(a_t[i] + shift) < (unsigned)g.T);
                ra[i] = buf_load4(rsrcA, ok ? a_off[i] + koff : OOB);
            }
        } else {
            const uint32_t koff = (uint32_t)((long)k0 * g.lda * 4);
#pragma unroll
            for (int i = 0; i < NLA; ++i) {
                bool ok = a_off[i] != OOB && (k0 + a_t[i]) < g.K;
                ra[i] = buf_load4(rsrcA, ok ? a_off[i] + koff : OOB);
                csum[i].x += ra[i].x; csum[i].y += ra[i].y; csum[i].z += ra[i].z; csum[i].w += ra[i].w;
            }
        }
        // ---------------- B
        if (B_KC) {
            const uint32_t koff = (uint32_t)(k0 * 4);
#pragma unroll
            for (int i = 0; i < NLB; ++i) rb[i] = buf_load4(rsrcB, b_off[i] != OOB ? b_off[i] + koff : OOB);
        } else {
            const int shift = g.shift0 + ztap * g.shift_step;
            const uint32_t koff = (uint32_t)((long)(k0 + shift) * g.ldb * 4);
#pragma unroll
            for (int i = 0; i < NLB; ++i) {
                int idx = tid + i * 256;
                int k = k0 + idx / (BN / 4);
                bool ok = b_off[i] != OOB && k < g.K;
                if (g.T > 0) ok = ok && ((unsigned)((k % g.T) + shift) < (unsigned)g.T);
                rb[i] = buf_load4(rsrcB, ok ? b_off[i] + koff : OOB);
            }
        }
    };

    auto store_tiles = [&](int buf) {
        float* as = lds + buf * STAGE;
        float* bs = as + A_ELEMS;
        if (A_KC) {
#pragma unroll
            for (int i = 0; i < NLA; ++i) {
                int idx = tid + i * 256;
                int row = idx >> 2, ch = idx & 3;
                if (row < BM) {
                    float* d = as + row * KC_LD + ch * 4;
                    d[0] = ra[i].x; d[1] = ra[i].y; d[2] = ra[i].z; d[3] = ra[i].w;
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < NLA; ++i) {
                int idx = tid + i * 256;
                if (idx < BK * (BM / 4)) {
                    int kr = idx / (BM / 4), c4 = idx % (BM / 4);
                    *reinterpret_cast<float4*>(as + kr * BM + c4 * 4) = ra[i];
                }
            }
        }
        if (B_KC) {
#pragma unroll
            for (int i = 0; i < NLB; ++i) {
                int idx = tid + i * 256;
                int row = idx >> 2, ch = idx & 3;
                if (row < BN) {
                    float* d = bs + row * KC_LD + ch * 4;
                    d[0] = rb[i].x; d[1] = rb[i].y; d[2] = rb[i].z; d[3] = rb[i].w;
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < NLB; ++i) {
                int idx = tid + i * 256;
                if (idx < BK * (BN / 4)) {
                    int kr = idx / (BN / 4), c4 = idx % (BN / 4);
                    *reinterpret_cast<float4*>(bs + kr * BN + c4 * 4) = rb[i];
                }
            }
        }
    };

    auto compute = [&](int buf) {
        const float* as = lds + buf * STAGE;
        const float* bs = as + A_ELEMS;
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk) {
            float a[TM], b[TN];
            const int k = kk * 2 + half;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                int m = wm * WTM + i * 32 + l31;
                a[i] = A_KC ? as[m * KC_LD + k] : as[k * BM + m];
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                int n = wn * WTN + j * 32 + l31;
                b[j] = B_KC ? bs[n * KC_LD + k] : bs[k * BN + n];
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    };

    if (kt_begin < kt_end) {
        load_tiles(kt_begin);
        store_tiles(0);
        __syncthreads();
        int buf = 0;
        for (int kt = kt_begin; kt < kt_end; ++kt) {
            const bool more = (kt + 1) < kt_end;
            if (more) load_tiles(kt + 1);
            compute(buf);
            if (more) store_tiles(buf ^ 1);
            __syncthreads();
            buf ^= 1;
        }
    }

    if constexpr (!A_KC && !B_KC) {
        // bias-gradient partials: sum over this split's rows of dy for the BM output channels of the tile
        if (g.colsum != nullptr && blockIdx.x == 0 && ztap == 0) {
            __syncthreads();
#pragma unroll
            for (int i = 0; i < NLA; ++i) {
                int idx = tid + i * 256;
                if (idx < BK * (BM / 4)) {
                    int kr = idx / (BM / 4), c4 = idx % (BM / 4);
                    *reinterpret_cast<float4*>(lds + kr * BM + c4 * 4) = csum[i];
                }
            }
            __syncthreads();
            if (tid < BM && m0 + tid < g.M) {
                float sacc = 0.f;
#pragma unroll
                for (int kr = 0; kr < BK; ++kr) sacc += lds[kr * BM + tid];
                g.colsum[(long)zsplit * g.M + m0 + tid] = sacc;
            }
        }
    }

    // ---------------- epilogue
    float* C = g.C + (long)z * g.c_zstride;
    const bool do_drop = g.drop_thr != 0u;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int col = n0 + wn * WTN + j * 32 + l31;
            const bool col_ok = col < g.N;
            const float bv = (g.bias != nullptr && col_ok) ? g.bias[col] : 0.f;
            const int row0 = m0 + wm * WTM + i * 32;
            float res[16];
            // all residual loads of the sub-tile are issued before the first store (one wait, not sixteen)
            if (g.residual != nullptr) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = row0 + acc_row(r, half);
                    res[r] = (row < g.M && col_ok) ? g.residual[(long)row * g.ldr + col] : 0.f;
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) res[r] = 0.f;
            }
            float gate[16];
            if (g.relu_out != nullptr) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = row0 + acc_row(r, half);
                    gate[r] = (row < g.M && col_ok && g.relu_out[(long)row * g.ldc + col] > 0.f) ? g.relu_scale : 0.f;
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) gate[r] = 1.f;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = row0 + acc_row(r, half);
                float v = acc[i][j][r] + bv;
                if (g.act == 1) v = fmaxf(v, 0.f);
                if (do_drop) {
                    uint64_t idx = (uint64_t)row * (uint64_t)g.N + (uint64_t)col;
                    v = keep_elem(seed_eff, idx, g.drop_thr) ? v * g.drop_scale : 0.f;
                }
                v = v * gate[r] + res[r];
                if (row < g.M && col_ok) C[(long)row * g.ldc + col] = v;
            }
        }
    }
}

// w[co][ci][tap] -> wp[co][tap][ci]  (forward: K-contiguous rows per output channel)
//                -> wt[ci][tap][co]  (data gradient: K-contiguous rows per input channel)
__global__ void conv_pack_weight_kernel(const float* __restrict__ w, float* __restrict__ wp, float* __restrict__ wt,
                                        int cout, int cin, int taps) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long n = (long)cout * cin * taps;
    if (i >= n) return;
    int tap = (int)(i % taps);
    long r = i / taps;
    int ci = (int)(r % cin);
    int co = (int)(r / cin);
    float v = w[i];
    if (wp) wp[((long)co * taps + tap) * cin + ci] = v;
    if (wt) wt[((long)ci * taps + tap) * cout + co] = v;
}

template <int BM, int BN, int WM, int WN, bool A_KC, bool B_KC>
static int launch_gemm(const GemmArgs& g, int zdim, hipStream_t stream) {
    dim3 grid(cdiv(g.N, BN), cdiv(g.M, BM), zdim);
    hipLaunchKernelGGL((gemm_f32_kernel<BM, BN, WM, WN, A_KC, B_KC>), grid, dim3(256), 0, stream, g);
    TTTS_LAUNCH_CHECK("gemm_f32_kernel");
    return TTTS_OK;
}


// Pick the tile that minimises the busiest CU's work: ceil(tiles / 256 CUs) workgroups in sequence, each costing
// its area divided by how efficiently that tile shape runs.  E.g. M = 55 680, N = 256 in fp32: 870 tiles of 128x128
// are 4 deep on some CUs (65 536), 1 740 tiles of 64x128 are 7 deep at 0.93 efficiency (61 660) -> 64x128.
// The split-precision kernel is latency / traffic bound, so small tiles cost it more (second efficiency table).
static int choose_tile(long M, long N, long zdim, bool x6 = false) {
    struct Cand { int tile, bm, bn; float eff_f32, eff_x6; };
    const Cand cands[] = {{TILE_128, 128, 128, 1.00f, 1.00f}, {TILE_64x128, 64, 128, 0.93f, 0.75f}, {TILE_64, 64, 64, 0.80f, 0.60f}};
    int best = TILE_128;
    float best_cost = 1e30f;
    for (const Cand& c : cands) {
        long tiles = (long)cdiv(M, c.bm) * cdiv(N, c.bn) * zdim;
        float cost = (float)((tiles + 255) / 256) * (float)(c.bm * c.bn) / (x6 ? c.eff_x6 : c.eff_f32);
        if (cost < best_cost) { best_cost = cost; best = c.tile; }
    }
    return best;
}

template <bool A_KC, bool B_KC>
static int dispatch_gemm(const GemmArgs& g, int zdim, int tile, hipStream_t stream) {
    if (tile == TILE_AUTO) {
        if (g.N <= 96 && (long)cdiv(g.M, 128) * zdim >= 384) tile = TILE_128x96;   // 80-wide mel GEMMs
        else tile = choose_tile(g.M, g.N, zdim);
    }
    switch (tile) {
        case TILE_64: return launch_gemm<64, 64, 2, 2, A_KC, B_KC>(g, zdim, stream);
        case TILE_64x128: return launch_gemm<64, 128, 2, 2, A_KC, B_KC>(g, zdim, stream);
        case TILE_128x96: return launch_gemm<128, 96, 4, 1, A_KC, B_KC>(g, zdim, stream);
        default: return launch_gemm<128, 128, 2, 2, A_KC, B_KC>(g, zdim, stream);
    }
}

// ===============================================================================================================
// Split-precision variant ("bf16x6"): fp32-accurate products on the 16x faster bf16 MFMA.
// Every fp32 operand value is written as hi + mid + lo, three bf16 numbers (8 mantissa bits each, so 24 bits: the
// split is exact up to 2^-25 relative), and the six leading cross products
//     a1*b1 + (a1*b2 + a2*b1) + (a1*b3 + a2*b2 + a3*b1)
// are accumulated in fp32 by v_mfma_f32_32x32x16_bf16 (each bf16 x bf16 product is exact in fp32).  The dropped
// terms are O(2^-24) relative: measured error of a K = 256..1024 GEMM against fp64 is 1.1e-7, BELOW the 2.9e-7 of
// a plain fp32 fma chain, at 6/16 of the fp32-MFMA cycle count.
// Activations (A) are split on the fly while they are staged into LDS; weights (B) are split once per call by
// weight_split_kernel into bf16 planes laid k-tile-major ([K/16][plane][N][16]), so the B loader moves whole lines.
// LDS image per operand plane: [row][16 k] bf16 = 32-byte rows; the two 16-byte chunks of a row are swapped on rows
// with bit 3 set (chunk ^= (row >> 3) & 1), which makes the ds_read_b128 of the MFMA fragments conflict-free.

// B[r][c] (R rows of C bf16 per plane p = hi, mid, lo; stored as [c/16][p][r][c%16]) from a weight tensor:
//   mode 0: linear forward      B[r][c] = w[r*C + c]                      (w is (R, C))
//   mode 1: linear data-grad    B[r][c] = w[c*R + r]                      (w is (C, R); B = w^T)
//   mode 2: conv forward        B[co][tap*cin + ci] = w[(co*cin + ci)*taps + tap]       (R = cout, C = taps*cin)
//   mode 3: conv data-grad      B[ci][tap*cout + co] = w[(co*cin + ci)*taps + tap]      (R = cin,  C = taps*cout)
__device__ __forceinline__ void weight_split_one(const float* __restrict__ w, unsigned short* __restrict__ planes, int R,
                                                 int C, int mode, int c2, int taps, long i) {
    const long n = (long)R * C;
    if (i >= n) return;
    const int r = (int)(i / C), c = (int)(i % C);
    float v;
    if (mode == 0) v = w[i];
    else if (mode == 1) v = w[(long)c * R + r];
    else {
        const int tap = c / c2, ch = c % c2;          // c2 = channels per tap
        if (mode == 2) v = w[((long)r * c2 + ch) * taps + tap];          // r = co, ch = ci, c2 = cin
        else v = w[((long)ch * R + r) * taps + tap];                     // r = ci, ch = co, R = cin
    }
    __bf16 b1 = (__bf16)v;
    float r1 = v - (float)b1;
    __bf16 b2 = (__bf16)r1;
    float r2 = r1 - (float)b2;
    __bf16 b3 = (__bf16)r2;
    // k-tile-major image: [c / 16][plane][r][c % 16], so the BN x 16 block a workgroup stages per k-step and plane is
    // one contiguous run (whole 128-byte lines; a [r][c] image gave 32-byte row pieces and 4x the L2->L1 traffic)
    const long o = ((long)(c >> 4) * 3 * R + r) * 16 + (c & 15);
    const long ps = (long)R * 16;
    planes[o] = __builtin_bit_cast(unsigned short, b1);
    planes[o + ps] = __builtin_bit_cast(unsigned short, b2);
    planes[o + 2 * ps] = __builtin_bit_cast(unsigned short, b3);
}
__global__ __launch_bounds__(256) void weight_split_kernel(const float* __restrict__ w, unsigned short* __restrict__ planes,
                                                           int R, int C, int mode, int c2, int taps) {
    weight_split_one(w, planes, R, C, mode, c2, taps, (long)blockIdx.x * blockDim.x + threadIdx.x);
}
// every weight of the model in one launch (after an optimizer step): descriptor i = 8 int64
// {w, planes, R, C, mode, c2, taps, first block}; a workgroup finds its descriptor by bisection on the block starts
// descriptor of the weight that block `blk` of a batched launch works on (first_block ascending)
__device__ __forceinline__ const long* batched_desc(const long* __restrict__ descs, int n, long blk) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (descs[mid * 8 + 7] <= blk) lo = mid; else hi = mid - 1;
    }
    return descs + lo * 8;
}

// fp16x3 images (modes 4-7) carry max|w| in their tail: zero the tails, then one atomic max per wave
// A LINEAR entry (modes 4, 5, 8, 9) may describe a WINDOW of a stacked image (weight_split_h3_tile): d[5] = (image rows << 32) |
// image columns, d[6] = (first image row << 32) | first image column of the window; d[5] = 0: the entry is its own image.
struct DescGeom { long Rimg, Cimg; int r_off, c_off; bool stacked; };
__device__ __forceinline__ DescGeom desc_geom(const long* d) {
    DescGeom g;
    const bool conv = h3_mode_base(d[4]) >= 2;
    g.stacked = !conv && d[5] != 0;
    g.Rimg = g.stacked ? (d[5] >> 32) : d[2];
    g.Cimg = g.stacked ? (d[5] & 0xffffffffL) : d[3];
    g.r_off = g.stacked ? (int)(d[6] >> 32) : 0;
    g.c_off = g.stacked ? (int)(d[6] & 0xffffffffL) : 0;
    return g;
}
__device__ __forceinline__ float* batched_tail(const long* d) {
    const bool conv = h3_mode_base(d[4]) >= 2;
    const DescGeom g = desc_geom(d);
    return reinterpret_cast<float*>(reinterpret_cast<char*>(d[1]) +
                                    h3_plane_bytes(g.Rimg, h3_image_cols(g.Cimg, conv ? (int)d[5] : 0, conv ? (int)d[6] : 0)));
}
__global__ __launch_bounds__(256) void weight_tail_zero_batched_kernel(const long* __restrict__ descs, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const long* d = descs + i * 8;
        if (d[4] >= 4) *batched_tail(d) = 0.f;
    }
}
// The images of ONE weight (forward / data-gradient, row-major / K16-major: up to four table entries, adjacent because the table
// is built parameter by parameter) share max|w|: the first of them -- the leader -- measures it, the others copy it while they
// are split (weight_split_batched_kernel).  Same source address and element count = same tensor.  Windows of stacked images
// share only among themselves: the tail they publish into holds the maximum over EVERY weight of the stack (each window's
// leader adds its own), which a plain image of one of those weights must not take for its own scale.
__device__ __forceinline__ const long* batched_leader(const long* __restrict__ descs, const long* d) {
    const long* l = d;
    const bool stacked = desc_geom(d).stacked;
    while (l > descs && (l - 8)[0] == d[0] && (l - 8)[2] * (l - 8)[3] == d[2] * d[3] && (l - 8)[4] >= 4 &&
           desc_geom(l - 8).stacked == stacked)
        l -= 8;
    return l;
}

__global__ __launch_bounds__(256) void weight_amax_batched_kernel(const long* __restrict__ descs, int n) {
    const long blk = blockIdx.x;
    const long* d = batched_desc(descs, n, blk);
    if (d[4] >= 4 && batched_leader(descs, d) == d) {
        const bool conv = h3_mode_base(d[4]) >= 2;
        weight_amax_h3_unit(reinterpret_cast<const float*>(d[0]), reinterpret_cast<unsigned short*>(d[1]), (int)d[2], (int)d[3],
                            h3_image_cols(d[3], conv ? (int)d[5] : 0, conv ? (int)d[6] : 0), blk - d[7],
                            h3_split_units(d[2], d[3], h3_mode_base(d[4]), conv ? (int)d[5] : 0), batched_tail(d));
    }
}

__global__ __launch_bounds__(256) void weight_split_batched_kernel(const long* __restrict__ descs, int n) {
    __shared__ float t[H3_SPLIT_TAPS][32][33];
    const long blk = blockIdx.x;
    const long* d = batched_desc(descs, n, blk);
    if (d[4] >= 4) {    // modes 4-7: the fp16x3 image of modes 0-3 (block-uniform branch), a 32 x 32 tile per workgroup
        const long* lead = batched_leader(descs, d);
        const float* amax = batched_tail(lead);
        // the GEMMs read the image's own tail (for the windows of a stacked image: every window writes the same value)
        if (lead != d && blk == d[7] && threadIdx.x == 0) *batched_tail(d) = *amax;
        const DescGeom g = desc_geom(d);
        const bool conv = h3_mode_base(d[4]) >= 2;
        weight_split_h3_tile(reinterpret_cast<const float*>(d[0]), reinterpret_cast<unsigned short*>(d[1]), (int)d[2],
                             (int)d[3], h3_mode_base(d[4]), conv ? (int)d[5] : 0, conv ? (int)d[6] : 0, blk - d[7], t, h3_mode_k16(d[4]), amax,
                             g.stacked ? (int)g.Rimg : 0, g.r_off, g.c_off);
    } else
        weight_split_one(reinterpret_cast<const float*>(d[0]), reinterpret_cast<unsigned short*>(d[1]), (int)d[2], (int)d[3],
                         (int)d[4], (int)d[5], (int)d[6], (blk - d[7]) * 256 + threadIdx.x);
}

template <int BM, int BN, int WM, int WN, bool CLIP>
__global__ __launch_bounds__(256, TTTS_GEMM_MINWAVES) void gemm_bf16x6_kernel(GemmArgs g) {
    const uint64_t seed_eff = site_seed(g.seed, g.step_seed);
    constexpr int WTM = BM / WM, WTN = BN / WN;
    constexpr int TM = WTM / 32, TN = WTN / 32;
    static_assert(WM * WN == 4 && BK == 16, "4 waves per workgroup, one MFMA k-step per k-tile");
    static_assert((BM * 4) % 256 == 0, "every thread stages whole float4s of the A tile");
    constexpr int A_PLANE = BM * 8, B_PLANE = BN * 8;          // dwords per plane (32-byte rows)
    constexpr int STAGE = 3 * (A_PLANE + B_PLANE);
    constexpr int NLA = (BM * 4 + 255) / 256;                  // float4 loads per thread for the A tile
    constexpr bool B_ALL = (BN * 2 >= 256);                    // B tile: BN rows x 2 half-chunks of 16 B per plane

    __shared__ __attribute__((aligned(16))) uint32_t lds[2 * STAGE];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const int wm = wave / WN, wn = wave % WN;
#if TTTS_X6_XCD
    // Workgroups are dispatched x-fastest and dealt round-robin to the 8 XCDs, each with its own L2.  Renumber so
    // that XCD e works on one contiguous run of tiles (column blocks of a row panel first): the nx workgroups that
    // read the same A rows then share an L2 (1 miss + nx-1 hits instead of nx fetches from the Infinity Cache / HBM,
    // whose per-CU rate -- 10-14 B/clk -- is what bounds this kernel otherwise).
    const int nx = gridDim.x;
    const int ntiles = nx * gridDim.y;
    const int bid = blockIdx.y * nx + blockIdx.x;
    const int xcd = bid & 7, slot = bid >> 3;
    const int per = ntiles >> 3, rem = ntiles & 7;
    const int t = xcd * per + min(xcd, rem) + slot;
    const int ty = t / nx, tx = t - ty * nx;
    const int m0 = ty * BM, n0 = tx * BN;
#else
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
#endif
    const int nkt = g.K / BK;

    const __amdgpu_buffer_rsrc_t rsrcA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.A), 0, g.a_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrcB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.B), 0, g.b_bytes, 0x00020000);
    const uint32_t b_plane_bytes = (uint32_t)g.N * 32u;           // one plane of one k-tile: N rows of 16 bf16

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    float4 ra[NLA];
    u32x4 rb[3];

    // Loader state.  No per-load validity arithmetic except the utterance clipping of shifted rows (CLIP): rows past the
    // end of an operand fall outside its buffer descriptor (hardware returns 0), weight rows past N only feed accumulator
    // columns that are never stored.  The k position (tap, channel offset, row shift) advances incrementally: loads are
    // requested in k order, each k-tile exactly once.
    int a_t[NLA];
    uint32_t a_off[NLA];
#pragma unroll
    for (int i = 0; i < NLA; ++i) {
        const int idx = tid + i * 256;
        const int row = idx >> 2, ch = idx & 3;
        const int m = m0 + row;
        a_off[i] = (uint32_t)(((long)m * g.lda + ch * 4) * 4);
        a_t[i] = CLIP ? (m % g.T) : 0;
    }
    // B: thread -> (row = tid>>1, half-chunk = tid&1): 8 bf16 = 16 bytes per plane
    const int b_row = tid >> 1, b_hc = tid & 1;
    uint32_t b_cur = (uint32_t)((n0 + b_row) * 32 + b_hc * 16);
    int k_c0 = 0, k_shift = g.shift0;
    uint32_t k_off = (uint32_t)((long)g.shift0 * g.lda * 4);
    const uint32_t tap_step = (uint32_t)(((long)g.shift_step * g.lda - g.cin) * 4);

    auto load_a = [&](int) {
#pragma unroll
        for (int i = 0; i < NLA; ++i) {
            uint32_t off = a_off[i] + k_off;
            if (CLIP) off = ((unsigned)(a_t[i] + k_shift) < (unsigned)g.T) ? off : OOB;
            ra[i] = buf_load4(rsrcA, off);
        }
        k_c0 += BK;
        k_off += BK * 4;
        if (k_c0 == g.cin) { k_c0 = 0; k_shift += g.shift_step; k_off += tap_step; }
    };
    auto load_b = [&](int) {
#pragma unroll
        for (int p = 0; p < 3; ++p)
            rb[p] = __builtin_amdgcn_raw_buffer_load_b128(rsrcB, (int)(b_cur + p * b_plane_bytes), 0, 0);
        b_cur += 3u * b_plane_bytes;
    };

    auto store_a = [&](int buf, int i) {
        uint32_t* as = lds + buf * STAGE;
        int idx = tid + i * 256;
        int row = idx >> 2, ch = idx & 3;
        if ((BM * 4) % 256 == 0 || row < BM) {
            uint2 hi, mid, lo;
            split3_pack4(ra[i], hi, mid, lo);
            const int d = row * 8 + (((ch >> 1) ^ ((row >> 3) & 1)) * 4) + (ch & 1) * 2;
            *reinterpret_cast<uint2*>(as + d) = hi;
            *reinterpret_cast<uint2*>(as + A_PLANE + d) = mid;
            *reinterpret_cast<uint2*>(as + 2 * A_PLANE + d) = lo;
        }
    };
    auto store_b = [&](int buf) {
        uint32_t* bs = lds + buf * STAGE + 3 * A_PLANE;
        if (B_ALL || b_row < BN) {
            const int d = b_row * 8 + ((b_hc ^ ((b_row >> 3) & 1)) * 4);
#pragma unroll
            for (int p = 0; p < 3; ++p) *reinterpret_cast<u32x4*>(bs + p * B_PLANE + d) = rb[p];
        }
    };

    // One k-step.  LDS[buf] holds tile kt, the staging registers hold tile kt+1 (requested in the middle of the previous
    // step).  After the first accumulator tile's MFMAs the registers are split / written to LDS[buf^1] and immediately
    // re-used to request tile kt+2: every load has a whole k-step to land and the staging VALU / LDS work sits in the
    // shadow of the remaining MFMAs, on ONE register set.
    auto step = [&](int buf, int kt_next2, bool stage, bool fetch) {
        const uint32_t* as = lds + buf * STAGE;
        const uint32_t* bs = as + 3 * A_PLANE;
        const int cw = ((half ^ ((l31 >> 3) & 1)) * 4);       // swizzled 16-byte chunk of this lane's 8 k values
        bf16x8 a[3][TM], b[3][TN];
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
                a[p][i] = *reinterpret_cast<const bf16x8*>(as + p * A_PLANE + (wm * WTM + i * 32 + l31) * 8 + cw);
#pragma unroll
            for (int j = 0; j < TN; ++j)
                b[p][j] = *reinterpret_cast<const bf16x8*>(bs + p * B_PLANE + (wn * WTN + j * 32 + l31) * 8 + cw);
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                f32x16 c = acc[i][j];
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2][i], b[0][j], c, 0, 0, 0);   // smallest terms first
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1][i], b[1][j], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][i], b[2][j], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1][i], b[0][j], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][i], b[1][j], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][i], b[0][j], c, 0, 0, 0);
                acc[i][j] = c;
                if (i == 0 && j == 0) {
                    if (stage) {
#pragma unroll
                        for (int q = 0; q < NLA; ++q) store_a(buf ^ 1, q);
                        store_b(buf ^ 1);
                    }
                    if (fetch) { load_a(kt_next2); load_b(kt_next2); }
                }
            }
    };

    if (nkt > 0) {
        load_a(0);
        load_b(0);
#pragma unroll
        for (int q = 0; q < NLA; ++q) store_a(0, q);
        store_b(0);
        if (nkt > 1) { load_a(1); load_b(1); }
        __syncthreads();
        int buf = 0;
        for (int kt = 0; kt < nkt; ++kt) {
            step(buf, kt + 2, kt + 1 < nkt, kt + 2 < nkt);
            __syncthreads();
            buf ^= 1;
        }
    }

    // ---------------- epilogue.  The auxiliary operands (residual; the forward activation whose relu / dropout mask gates a
    // data gradient) are read through buffer descriptors: rows past M fall outside the descriptor and columns past N get
    // an out-of-range offset, so no load sits behind a branch -- a predicated global load compiles to "branch, load,
    // s_waitcnt vmcnt(0)" and serialises every one of the 16 loads of a tile.
    float* C = g.C;
    const bool do_drop = g.drop_thr != 0u;
    const bool has_gate = g.relu_out != nullptr, has_res = g.residual != nullptr;
    const __amdgpu_buffer_rsrc_t rsrcG = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(has_gate ? g.relu_out : g.A), 0, has_gate ? (uint32_t)((long)g.M * g.ldc * 4) : 0u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrcR = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(has_res ? g.residual : g.A), 0, has_res ? (uint32_t)((long)g.M * g.ldr * 4) : 0u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrcBias = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(g.bias != nullptr ? g.bias : g.A), 0, g.bias != nullptr ? (uint32_t)g.N * 4u : 0u, 0x00020000);
    float bias_v[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j)      // columns past N (and a null bias) fall outside the descriptor: 0
        bias_v[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrcBias, (n0 + wn * WTN + j * 32 + l31) * 4, 0, 0));
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int col = n0 + wn * WTN + j * 32 + l31;
            const bool col_ok = col < g.N;
            const float bv = bias_v[j];
            const int row0 = m0 + wm * WTM + i * 32;
            float res[16], gsrc[16];
            if (has_res) {                 // block-uniform: one scalar branch around the whole group of loads
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const long row = row0 + acc_row(r, half);
                    res[r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                        rsrcR, (int)(col_ok ? (uint32_t)((row * g.ldr + col) * 4) : OOB), 0, 0));
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) res[r] = 0.f;
            }
            if (has_gate) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const long row = row0 + acc_row(r, half);
                    gsrc[r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                        rsrcG, (int)(col_ok ? (uint32_t)((row * g.ldc + col) * 4) : OOB), 0, 0));
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = row0 + acc_row(r, half);
                float v = acc[i][j][r] + bv;
                if (g.act == 1) v = fmaxf(v, 0.f);
                if (do_drop) {
                    uint64_t idx = (uint64_t)row * (uint64_t)g.N + (uint64_t)col;
                    v = keep_elem(seed_eff, idx, g.drop_thr) ? v * g.drop_scale : 0.f;
                }
                if (has_gate) v = gsrc[r] > 0.f ? v * g.relu_scale : 0.f;
                v += res[r];
                if (row < g.M && col_ok) C[(long)row * g.ldc + col] = v;
            }
        }
    }
}

template <int BM, int BN, int WM, int WN>
static int launch_split(const GemmArgs& g, hipStream_t stream) {
    dim3 grid(cdiv(g.N, BN), cdiv(g.M, BM), 1);
    if (g.T > 0)
        hipLaunchKernelGGL((gemm_bf16x6_kernel<BM, BN, WM, WN, true>), grid, dim3(256), 0, stream, g);
    else
        hipLaunchKernelGGL((gemm_bf16x6_kernel<BM, BN, WM, WN, false>), grid, dim3(256), 0, stream, g);
    TTTS_LAUNCH_CHECK("gemm_bf16x6_kernel");
    return TTTS_OK;
}

static int dispatch_split(const GemmArgs& g, hipStream_t stream) {
    int tile = (g.N <= 96 && (long)cdiv(g.M, 128) >= 384) ? TILE_128x96 : choose_tile(g.M, g.N, 1, true);
    switch (tile) {
        case TILE_64: return launch_split<64, 64, 2, 2>(g, stream);
        case TILE_64x128: return launch_split<64, 128, 2, 2>(g, stream);
        case TILE_128x96: return launch_split<128, 96, 4, 1>(g, stream);
        default: return launch_split<128, 128, 2, 2>(g, stream);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Weight gradients in the split-precision form: C[n][k] (per tap, per row split) = sum_m dy[m][n] * x[m + shift][k].
// Both operands are activations whose REDUCTION index (the row m) is the slow one in memory, so the MFMA fragments
// (8 consecutive reduction indices per lane) are columns of the stored matrices.  The loader turns them: a thread
// fetches 8 consecutive rows of ONE column with 8 dword loads (a wave covers 64 adjacent columns: 256-byte runs),
// splits the 8 values into hi / mid / lo and writes three 16-byte pieces -- exactly the [row = column][16 k] LDS
// image of the kernel above, so fragments, MFMA order and bank behaviour are shared with it.
// Same GemmArgs meaning as gemm_f32_kernel<.., false, false>: A = dy (K x M), B = x (K x N), K = rows, z = split * ztaps
// + tap, colsum = per-split column sums of dy (bias gradient).
template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(256, TTTS_GEMM_MINWAVES) void wgrad_bf16x6_kernel(GemmArgs g) {
    constexpr int WTM = BM / WM, WTN = BN / WN;
    constexpr int TM = WTM / 32, TN = WTN / 32;
    static_assert(WM * WN == 4 && BK == 16 && BM <= 128 && BN <= 128, "4 waves, 16 rows per step, <= 128 columns per operand");
    constexpr int A_PLANE = BM * 8, B_PLANE = BN * 8;          // dwords per plane (32-byte rows)
    constexpr int STAGE = 3 * (A_PLANE + B_PLANE);

    __shared__ __attribute__((aligned(16))) uint32_t lds[2 * STAGE];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const int wm = wave / WN, wn = wave % WN;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    const int z = blockIdx.z;
    const int ztap = (g.ztaps > 1) ? (z % g.ztaps) : 0;
    const int zsplit = (g.ztaps > 1) ? (z / g.ztaps) : z;
    const int nkt = (g.K + BK - 1) / BK;
    const int kt_begin = zsplit * g.kt_per_split;
    int kt_end = kt_begin + g.kt_per_split;
    if (kt_end > nkt) kt_end = nkt;
    const int shift = g.shift0 + ztap * g.shift_step;

    const __amdgpu_buffer_rsrc_t rsrcA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.A), 0, g.a_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrcB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.B), 0, g.b_bytes, 0x00020000);

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // loader roles: thread -> (column, which 8 of the 16 rows).  2*BM (2*BN) threads take part.
    //               When both operands fit side by side (64x64 tile) A and B slots go to different waves.
    // No per-load validity arithmetic: rows past the end of the operand fall outside the buffer descriptor (hardware
    // returns 0), columns past the matrix edge only feed accumulator rows / columns that are never stored, and the
    // utterance clipping of shifted rows is applied to the loaded VALUES from one 8-bit mask per k-step.
    constexpr int B_T0 = (2 * BM + 2 * BN <= 256) ? 2 * BM : 0;
    const int tb = tid - B_T0;
    const bool a_slot = tid < 2 * BM, b_slot = tb >= 0 && tb < 2 * BN;
    const int a_col = tid % BM, a_rh = (tid / BM) & 1;
    const int b_col = (tb & 0xffff) % BN, b_rh = ((tb & 0xffff) / BN) & 1;
    const uint32_t a_row = (uint32_t)(g.lda * 4), b_row = (uint32_t)(g.ldb * 4);
    // byte offsets of this thread's first row at k-step kt_begin; advanced by 16 rows per step (wrap-around of the
    // shifted B offset below zero lands beyond the descriptor, i.e. reads 0)
    uint32_t a_cur = (uint32_t)(((long)kt_begin * BK + a_rh * 8) * g.lda + m0 + a_col) * 4u;
    uint32_t b_cur = (uint32_t)((((long)kt_begin * BK + b_rh * 8 + shift) * g.ldb + n0 + b_col) * 4);
    // position of this thread's first B row inside its utterance (clipping of shifted rows), kept incrementally
    int b_t = (g.T > 0) ? (int)(((long)kt_begin * BK + b_rh * 8) % g.T) : 0;
    const bool clip = g.T > 0 && shift != 0;

    float av[8], bv[8];
    float csum = 0.f;   // bias gradient: running sum of this thread's dy values

    auto load_tiles = [&](int) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            av[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrcA, (int)(a_cur + j * a_row), 0, 0));
#pragma unroll
        for (int j = 0; j < 8; ++j)
            bv[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrcB, (int)(b_cur + j * b_row), 0, 0));
        a_cur += BK * a_row;
        b_cur += BK * b_row;
    };
    // bit j set = row j of this thread's 8 is clipped: its position t_j = (b_t + j) mod T has t_j + shift outside [0, T)
    auto clip_mask = [&]() -> uint32_t {
        uint32_t m = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            int t = b_t + j;
            if (g.T >= BK) { if (t >= g.T) t -= g.T; } else t %= g.T;
            m |= ((unsigned)(t + shift) >= (unsigned)g.T) ? (1u << j) : 0u;
        }
        b_t += BK;
        if (g.T >= BK) { if (b_t >= g.T) b_t -= g.T; } else b_t %= g.T;
        return m;
    };

    auto store_tiles = [&](int buf) {
        uint32_t* as = lds + buf * STAGE;
        uint32_t* bs = as + 3 * A_PLANE;
        if (a_slot) {
            u32x4 hi, mid, lo;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                uint32_t h, m, l;
                split3_pair(f32x2{av[2 * q], av[2 * q + 1]}, h, m, l);
                hi[q] = h; mid[q] = m; lo[q] = l;
            }
            csum += ((av[0] + av[1]) + (av[2] + av[3])) + ((av[4] + av[5]) + (av[6] + av[7]));
            const int d = a_col * 8 + ((a_rh ^ ((a_col >> 3) & 1)) * 4);
            *reinterpret_cast<u32x4*>(as + d) = hi;
            *reinterpret_cast<u32x4*>(as + A_PLANE + d) = mid;
            *reinterpret_cast<u32x4*>(as + 2 * A_PLANE + d) = lo;
        }
        if (b_slot) {
            if (clip) {                      // block-uniform: only shifted taps pay for the clipping
                const uint32_t cm = clip_mask();
                if (cm != 0u) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) bv[j] = ((cm >> j) & 1u) ? 0.f : bv[j];
                }
            }
            u32x4 hi, mid, lo;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                uint32_t h, m, l;
                split3_pair(f32x2{bv[2 * q], bv[2 * q + 1]}, h, m, l);
                hi[q] = h; mid[q] = m; lo[q] = l;
            }
            const int d = b_col * 8 + ((b_rh ^ ((b_col >> 3) & 1)) * 4);
            *reinterpret_cast<u32x4*>(bs + d) = hi;
            *reinterpret_cast<u32x4*>(bs + B_PLANE + d) = mid;
            *reinterpret_cast<u32x4*>(bs + 2 * B_PLANE + d) = lo;
        }
    };

    auto compute = [&](int buf) {
        const uint32_t* as = lds + buf * STAGE;
        const uint32_t* bs = as + 3 * A_PLANE;
        const int cw = ((half ^ ((l31 >> 3) & 1)) * 4);
        bf16x8 a[3][TM], b[3][TN];
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
                a[p][i] = *reinterpret_cast<const bf16x8*>(as + p * A_PLANE + (wm * WTM + i * 32 + l31) * 8 + cw);
#pragma unroll
            for (int j = 0; j < TN; ++j)
                b[p][j] = *reinterpret_cast<const bf16x8*>(bs + p * B_PLANE + (wn * WTN + j * 32 + l31) * 8 + cw);
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                f32x16 c = acc[i][j];
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2][i], b[0][j], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1][i], b[1][j], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][i], b[2][j], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1][i], b[0][j], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][i], b[1][j], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][i], b[0][j], c, 0, 0, 0);
                acc[i][j] = c;
            }
    };

    if (kt_begin < kt_end) {
        load_tiles(kt_begin);
        store_tiles(0);
        __syncthreads();
        int buf = 0;
        for (int kt = kt_begin; kt < kt_end; ++kt) {
            const bool more = (kt + 1) < kt_end;
            if (more) load_tiles(kt + 1);
            compute(buf);
            if (more) store_tiles(buf ^ 1);
            __syncthreads();
            buf ^= 1;
        }
    }

    if (g.colsum != nullptr && blockIdx.x == 0 && ztap == 0) {
        float* fs = reinterpret_cast<float*>(lds);
        __syncthreads();
        if (a_slot) fs[a_rh * BM + a_col] = csum;
        __syncthreads();
        if (tid < BM && m0 + tid < g.M) g.colsum[(long)zsplit * g.M + m0 + tid] = fs[tid] + fs[BM + tid];
    }

    float* C = g.C + (long)z * g.c_zstride;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int col = n0 + wn * WTN + j * 32 + l31;
            const int row0 = m0 + wm * WTM + i * 32;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = row0 + acc_row(r, half);
                if (row < g.M && col < g.N) C[(long)row * g.ldc + col] = acc[i][j][r];
            }
        }
}

template <int BM, int BN, int WM, int WN>
static int launch_wgrad_split(const GemmArgs& g, int zdim, hipStream_t stream) {
    dim3 grid(cdiv(g.N, BN), cdiv(g.M, BM), zdim);
    hipLaunchKernelGGL((wgrad_bf16x6_kernel<BM, BN, WM, WN>), grid, dim3(256), 0, stream, g);
    TTTS_LAUNCH_CHECK("wgrad_bf16x6_kernel");
    return TTTS_OK;
}

static int dispatch_wgrad_split(const GemmArgs& g, int zdim, int tile, hipStream_t stream) {
    switch (tile) {
        case TILE_64: return launch_wgrad_split<64, 64, 2, 2>(g, zdim, stream);
        case TILE_128x96: return launch_wgrad_split<128, 96, 4, 1>(g, zdim, stream);
        case TILE_96x128: return launch_wgrad_split<96, 128, 1, 4>(g, zdim, stream);
        default: return launch_wgrad_split<128, 128, 2, 2>(g, zdim, stream);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Weight gradients: the problem C[N][K] (per tap) = dy^T[N][M] . x_shifted[M][K] with the row (reduction) dimension split over the
// grid's z, and a second stage that sums the partial products.  One planner, one description of the problem, one workspace layout,
// one set of checks and one body per stage serve all ten entry points.
enum WgradForm { WG_F32, WG_X6, WG_H3 };        // fp32 MFMA, bf16x6 (16-row k-steps), fp16x3 (32-row k-steps, dynamic pre-scales)
struct WgradPlan { int tile; int nsplit; int kt_per_split; long tiles; };
// a grouped launch as its members' plans see it: the class (ttts_wgrad_group_ok), the tile total, the longest row range in k-tiles
struct WgradGroup { int cls; long tiles_total; long nkt_max; };

// The workgroups a launch OF ITS OWN aims at.  The fp32-MFMA / bf16x6 kernels aim at about 768
// workgroups (3 per CU).  The fp16x3 kernel holds two workgroups per CU, so 768 is one full round plus a half-empty one;
// it gets ONE round -- 512 workgroups for outputs of more than 12 tiles over long row ranges, else 256: every split costs
// a partial tile written and read again, which for the small outputs weighs more than a second workgroup per CU brings
// (measured on the step's shapes, tools/wgrad_bench.py: 256x256 118 -> 134, 768x256 157 -> 188, 256x1024 189 -> 214 TF).
static long wgrad_target_single(WgradForm f, int tile, long tiles, long nkt) {
    if (f != WG_H3) return 768;
    if (tile == H3_TILE_256) return 256;                           // (the 8-wave tile holds one workgroup per CU)
    return (tiles > 12 && nkt >= 800) ? 512 : 256;
}

// The workgroups a GROUPED launch aims at -- the rule above applied to the group as a whole: the 8-wave tile (class 2) holds one
// workgroup per CU, the 4-wave tile two (a second round only for many tiles over long row ranges)
// (the 96-wide tiles' workgroups are long -- 10 + 2 tiles of the mel side over 55 680 rows were 140 us on 252 workgroups -- and
// their partial tiles small: both workgroup slots of every CU from 8 tiles on)
// (row ranges from 200 k-tiles on -- 6 400 rows: at 13 920 rows a group on ONE workgroup slot per CU ran its 109 k-tiles per
// workgroup at a fifth of the MFMA rate, nothing covering its operand latencies: batch 16 -0.08 ms, `profiles/r06_ab_wgrad_target.txt`)
constexpr long WG_GROUP_NKT512 = 200;
static long wgrad_group_many(int cls) { return (cls == 3 || cls == 4) ? 8 : 13; }
static long wgrad_target_group(const WgradGroup& grp) {
    if (grp.cls == 2) return 256;
    return (grp.tiles_total >= wgrad_group_many(grp.cls) && grp.nkt_max >= WG_GROUP_NKT512) ? 512 : 256;
}

// THE planner: the tile of dw[N][K] x taps over M rows in form `f`, and how the rows are split -- for a launch of its own, or
// (grp) as a member of a grouped launch, whose workgroup target is shared by the tiles of all members.  M, N, K, taps > 0.
static WgradPlan plan_wgrad(int64_t M, int N, int K, int taps, WgradForm f, const WgradGroup* grp = nullptr) {
    WgradPlan p; const long bk = f == WG_H3 ? HBK : BK, nkt = (M + bk - 1) / bk;
    p.tile = (K <= 96) ? TILE_128x96 : TILE_128;
    p.tiles = (long)cdiv(N, 128) * cdiv(K, 128) * taps;
    if (f != WG_F32) {
        // the split-precision kernel wants the large tile (its per-thread staging work is fixed per k-step); small
        // outputs get more row splits instead, capped so that the partial sums stay a few tens of MB
        if (N <= 64 && K <= 64) { p.tile = TILE_64; p.tiles = (long)cdiv(N, 64) * cdiv(K, 64) * taps; }
        else if (N <= 96 && K > 96) p.tile = TILE_96x128;          // 80-wide mel outputs
    } else if (p.tiles < 16) { p.tile = TILE_64; p.tiles = (long)cdiv(N, 64) * cdiv(K, 64) * taps; }
    if (f == WG_H3) {
        // The kernel's speed is set by the operand bytes its workgroups request (tiles x rows x (BM + BN) x 4 B at about
        // 7.7 TB/s over the chip: 1024x256 with 128-wide tiles asks for 913 MB = 119 us, measured 119), so outputs of three
        // or more 256 x 256 tiles take the 8-wave 256-wide tile (half the bytes per product) on one workgroup per CU.  Smaller
        // outputs stay on the 128-wide tile: at 256 row splits their partial sums (256 KB each, written and read back)
        // would cost what the operands save.
        const long tiles256 = (long)cdiv(N, 256) * cdiv(K, 256) * taps;
        if (p.tile == TILE_128 && N >= 256 && K >= 256 && tiles256 >= 3 && nkt >= 800) { p.tile = H3_TILE_256; p.tiles = tiles256; }
    }
    // the row splits: `want` per tile, at most one per k-tile, at least 8 k-tiles each
    long want = grp ? wgrad_target_group(*grp) / grp->tiles_total : wgrad_target_single(f, p.tile, p.tiles, nkt) / p.tiles;
    if (want < 1) want = 1;
    if (!grp && f != WG_F32 && want > 128) want = 128;             // (the cap on a small output's partial sums, above)
    if (want > nkt) want = nkt;
    long per = (nkt + want - 1) / want;
    if (per < 8 && nkt >= 8) per = 8;
    p.kt_per_split = (int)per;
    p.nsplit = (int)((nkt + per - 1) / per);
    return p;
}

// the split-precision weight-gradient kernel pays off when its 128-wide (or 96-wide, for the 80-channel mel side) tiles
// are reasonably full
static bool wgrad_use_x6(int N, int K) { return (N >= 128 || N == 80 || N == 96) && (K >= 128 || K == 80 || K == 96) && (N >= 128 || K >= 128); }

// can dw[N,K(,tap)] = dy[M,N]^T x[M(+tap shift),K] be a member of a grouped launch, and of which CLASS (members of one launch
// share it)?  1: the fp16x3 form on the 4-wave 128 x 128 tile (small outputs); 2: whole 256 x 256 tiles on the 8-wave LDS-DMA
// kernel (long row ranges); 3 / 4: the 96-wide tiles of the 80-channel mel side; 0: none (the fp32-MFMA shapes, ragged
// 256-tiles keep launches of their own).  taps = 1: a linear weight; taps > 1: a convolution's (cout = N, cin = K).  The class's
// tile is the one of the problem's own fp16x3 plan; *tiles: how many of them the output is
static int wgrad_class(int64_t M, int N, int K, int taps, long* tiles = nullptr) {
    if (!(M > 0 && N > 0 && K > 0 && taps >= 1 && taps <= 64 && N % 4 == 0 && K % 4 == 0 && wgrad_use_x6(N, K))) return 0;
    const WgradPlan p = plan_wgrad(M, N, K, taps, WG_H3);
    if (tiles) *tiles = p.tiles;
    if (p.tile == TILE_128) return 1;
    if (p.tile == H3_TILE_256 && N % 256 == 0 && K % 256 == 0) return 2;
    if (p.tile == TILE_128x96) return 3;            // 80 input channels: the decoder pre-net's first linear, the post-net's first convolution
    if (p.tile == TILE_96x128) return 4;            // 80 output channels: the mel head, the post-net's last convolution
    return 0;
}

// The workspace of a weight gradient in `nsplit` row splits, in floats: nsplit x taps partial products of N x K from 0 on, then
// (from `colsum` on) nsplit rows of N column sums of dy -- the bias gradient's partial sums
struct WgradLayout { size_t colsum; size_t floats; };
static WgradLayout wgrad_layout(int nsplit, int N, int K, int taps) {
    const size_t prod = (size_t)nsplit * taps * N * K;
    return {prod, prod + (size_t)nsplit * N};
}

// One weight gradient dw[N][K] (x taps) (+)= dy[M][N]^T . x[M (row-shifted)][K] as its entry point states it
struct WgradProblem {
    const float *dy, *x; float* ws; size_t ws_bytes;
    int64_t M; int N, K, taps;          // (a convolution entry gives B and T: M = B T, N = cout, K = cin)
    int B, T, row_shift;                // utterances of T rows; a linear weight's x is read row_shift rows further inside them
    const float *dy_amax, *x_amax;      // partial maxima of |dy| and |x| (fp16x3)
    bool conv = false;                  // a same-padded convolution; else a linear weight
    bool bias = false;                  // the column sums of dy are wanted
};

// the GemmArgs of a planned problem: C[N][K] (per tap) = dy^T[N][M] . xshift[M][K], partial products and column sums into pb.ws
static GemmArgs wgrad_args(const WgradProblem& pb, WgradForm f, const WgradPlan& p) {
    GemmArgs g = base_args();
    g.A = pb.dy; g.B = pb.x; g.C = pb.ws; g.M = pb.N; g.N = pb.K; g.K = (int)pb.M;
    g.lda = pb.N; g.ldb = pb.K; g.ldc = pb.K;
    g.a_bytes = (uint32_t)((uint64_t)pb.M * pb.N * 4); g.b_bytes = (uint32_t)((uint64_t)pb.M * pb.K * 4);
    // the shift of x's rows: a convolution's taps walk from -(taps - 1) / 2 on, one row per tap; a linear weight has the one shift
    // its caller names, and utterances only then
    g.T = (pb.conv || pb.row_shift != 0) ? pb.T : 0;
    g.shift0 = pb.conv ? -((pb.taps - 1) / 2) : pb.row_shift; g.shift_step = pb.conv ? 1 : 0;
    g.ztaps = pb.taps; g.kt_per_split = p.kt_per_split; g.c_zstride = (long)pb.N * pb.K;
    g.colsum = pb.bias ? pb.ws + wgrad_layout(p.nsplit, pb.N, pb.K, pb.taps).colsum : nullptr;
    if (f == WG_H3) {
        g.a_amax = pb.dy_amax; g.a_amax_n = H3_AMAX_PARTIALS;
        g.b_amax = pb.x_amax; g.b_amax_n = H3_AMAX_PARTIALS;
    }
    return g;
}

// the second stage: the partial products of pb.ws summed into dw, the column sums into dbias.  A linear weight's N rows may belong
// to `nparts` destinations (equal row blocks; one pair of reductions per block), a convolution's are transposed to [co][ci][tap]
static int wgrad_reduce(const WgradProblem& pb, const WgradPlan& p, const float* colsum, float* const* dw, float* const* dbias, int nparts,
                        bool accumulate, hipStream_t stream, ttts_reduce_queue* queue) {
    if (pb.conv) {
        int rc = launch_conv_wgrad_reduce(pb.ws, dw[0], pb.N, pb.K, pb.taps, p.nsplit, accumulate, stream, queue);
        if (rc == TTTS_OK && colsum) rc = launch_reduce_rows(colsum, pb.N, p.nsplit, pb.N, dbias[0], pb.N, nullptr, accumulate, stream, queue);
        return rc;
    }
    const int Np = pb.N / nparts;
    const long nk = (long)pb.N * pb.K, np = (long)Np * pb.K;
    for (int i = 0; i < nparts; ++i) {
        int rc = launch_reduce_rows_pair(pb.ws + (size_t)i * np, nk, p.nsplit, np, dw[i], colsum ? colsum + (size_t)i * Np : nullptr, pb.N, Np,
                                         colsum ? dbias[i] : nullptr, accumulate, stream, queue);
        if (rc) return rc;
    }
    return TTTS_OK;
}

#define ENTRY_REQUIRE(cond, fmt, ...) TTTS_REQUIRE(cond, "%s: " fmt, name, ##__VA_ARGS__)
static int wgrad_check_operands(const char* name, const WgradProblem& pb) {
    ENTRY_REQUIRE(aligned16(pb.dy) && aligned16(pb.x) && aligned16(pb.ws), "pointers must be 16-byte aligned");
    ENTRY_REQUIRE((uint64_t)pb.M * pb.N * 4 < (1ull << 32) && (uint64_t)pb.M * pb.K * 4 < (1ull << 32), "operand larger than 4 GiB");
    return TTTS_OK;
}

// A launch of its own: the three Linear entries, `parts` and the three convolution entries -- the form their name asks for (shapes the
// split kernels do not take: the fp32-MFMA form, no maxima), then the second stage of one (dw, dbias), of a convolution, or per row block
enum WgradStage2 { WG_PAIR, WG_CONV, WG_PARTS };
static int wgrad_single(const char* name, WgradForm f, WgradStage2 stage, WgradProblem pb, float* const* dw, float* const* dbias,
                        int nparts, int accumulate, ttts_reduce_queue* queue, void* stream) {
    pb.conv = stage == WG_CONV;
    ENTRY_REQUIRE(pb.dy && pb.x && pb.ws && dw && (stage == WG_PARTS || dw[0]), "null pointer");
    ENTRY_REQUIRE(f != WG_H3 || (pb.dy_amax && pb.x_amax), "null pointer: dy_amax and x_amax (partial maxima of dy and x) are required");
    if (pb.conv) {
        ENTRY_REQUIRE(pb.B > 0 && pb.T > 0 && pb.K > 0 && pb.N > 0 && pb.taps > 0 && (pb.taps & 1), "bad dims B=%d T=%d cin=%d cout=%d taps=%d",
                      pb.B, pb.T, pb.K, pb.N, pb.taps);
        ENTRY_REQUIRE((long)pb.B * pb.T < (1L << 31), "B*T too large");
        pb.M = (int64_t)pb.B * pb.T;
    }
    ENTRY_REQUIRE(pb.M > 0 && pb.N > 0 && pb.K > 0 && pb.M < (1LL << 31), "bad dims M=%lld N=%d K=%d", (long long)pb.M, pb.N, pb.K);
    ENTRY_REQUIRE(pb.N % 4 == 0 && pb.K % 4 == 0, "%s=%d and %s=%d must be multiples of 4", pb.conv ? "cout" : "N", pb.N,
                  pb.conv ? "cin" : "K", pb.K);
    if (stage == WG_PARTS)
        ENTRY_REQUIRE(nparts > 0 && nparts <= 64 && pb.N % nparts == 0 && (pb.N / nparts) % 4 == 0,
                      "N=%d does not split in %d blocks of whole float4s", pb.N, nparts);
    if (int rc = wgrad_check_operands(name, pb)) return rc;
    ENTRY_REQUIRE(pb.ws_bytes >= ttts_wgrad_workspace_bytes(pb.M, pb.N, pb.K, pb.taps), "workspace too small");
    ENTRY_REQUIRE(pb.conv || pb.row_shift == 0 || (pb.T > 0 && pb.M % pb.T == 0), "row_shift needs T>0 and M %% T == 0");
    for (int i = 0; i < nparts; ++i) ENTRY_REQUIRE(dw[i] != nullptr, "null destination");
    if (!wgrad_use_x6(pb.N, pb.K)) f = WG_F32;
    pb.bias = dbias != nullptr && dbias[0] != nullptr;
    const WgradPlan p = plan_wgrad(pb.M, pb.N, pb.K, pb.taps, f);
    const GemmArgs g = wgrad_args(pb, f, p);
    const int zdim = p.nsplit * pb.taps;
    const int rc = f == WG_H3 ? dispatch_wgrad_h3(g, zdim, p.tile, (hipStream_t)stream)
           : f == WG_X6 ? dispatch_wgrad_split(g, zdim, p.tile, (hipStream_t)stream)
                        : dispatch_gemm<false, false>(g, zdim, p.tile, (hipStream_t)stream);
    return rc ? rc : wgrad_reduce(pb, p, g.colsum, dw, dbias, nparts, accumulate != 0, (hipStream_t)stream, queue);
}

}  // namespace ttts

using namespace ttts;

extern "C" {

size_t ttts_wgrad_workspace_bytes(int64_t M, int N, int K, int taps) {
    // The largest split count any launch can plan for this problem: the three forms of a launch of its own (their counts differ) and
    // the grouped launches it may be a member of.  A member's count grows with the splits wanted per tile, target / tile total
    // (plan_wgrad: fewer k-tiles per split, never fewer splits), and a group's tile total is at least the member's own: the worst
    // group is the member ALONE -- or, for an output of fewer tiles than the 512-workgroup target asks for, the smallest group that
    // reaches that target (wgrad_group_many tiles, a row range as long as another member may bring).  0 for a dimension that is none.
    if (!(M > 0 && N > 0 && K > 0 && taps > 0)) return 0;
    int ns = 0;
    auto cover = [&](WgradForm f, const WgradGroup* grp) { const int n = plan_wgrad(M, N, K, taps, f, grp).nsplit; ns = n > ns ? n : ns; };
    cover(WG_F32, nullptr); cover(WG_X6, nullptr); cover(WG_H3, nullptr);
    long tiles = 0;
    if (const int cls = wgrad_class(M, N, K, taps, &tiles)) {
        const long many = wgrad_group_many(cls);
        const WgradGroup alone = {cls, tiles, (long)((M + HBK - 1) / HBK)}, full = {cls, tiles < many ? many : tiles, WG_GROUP_NKT512};
        cover(WG_H3, &alone); cover(WG_H3, &full);
    }
    return wgrad_layout(ns, N, K, taps).floats * sizeof(float);
}

// dw[N,K] (+)= dy[M,N]^T . x[M,K] ; dbias[N] (+)= column sums of dy     ({...}: a WgradProblem up to its maxima)
int ttts_linear_bwd_weight(const float* dy, const float* x, float* dw, float* dbias, float* ws, size_t ws_bytes,
                           int64_t M, int N, int K, int row_shift, int T, int accumulate, ttts_reduce_queue* queue, void* stream) {
    return wgrad_single("linear_bwd_weight", WG_F32, WG_PAIR, {dy, x, ws, ws_bytes, M, N, K, 1, 0, T, row_shift, nullptr, nullptr}, &dw, &dbias, 1,
                        accumulate, queue, stream);
}
int ttts_linear_bwd_weight_x6(const float* dy, const float* x, float* dw, float* dbias, float* ws, size_t ws_bytes,
                              int64_t M, int N, int K, int row_shift, int T, int accumulate, ttts_reduce_queue* queue, void* stream) {
    return wgrad_single("linear_bwd_weight_x6", WG_X6, WG_PAIR, {dy, x, ws, ws_bytes, M, N, K, 1, 0, T, row_shift, nullptr, nullptr}, &dw, &dbias, 1,
                        accumulate, queue, stream);
}
int ttts_linear_bwd_weight_h3(const float* dy, const float* x, float* dw, float* dbias, float* ws, size_t ws_bytes,
                              int64_t M, int N, int K, int row_shift, int T, int accumulate, const float* dy_amax,
                              const float* x_amax, ttts_reduce_queue* queue, void* stream) {
    return wgrad_single("linear_bwd_weight_h3", WG_H3, WG_PAIR, {dy, x, ws, ws_bytes, M, N, K, 1, 0, T, row_shift, dy_amax, x_amax}, &dw, &dbias, 1,
                        accumulate, queue, stream);
}

// ONE weight-gradient GEMM dy^T x (N x K) whose N rows belong to `nparts` different weights (equal row blocks): block i is reduced into
// dw_parts[i] ((N / nparts) x K, contiguous), its column sums into dbias_parts[i] -- the fused K/V projection of all decoder layers'
// cross-attention (model/layers.py:54-74 runs it once per layer on the same memory)
int ttts_linear_bwd_weight_h3_parts(const float* dy, const float* x, float* const* dw_parts, float* const* dbias_parts, int nparts,
                                    float* ws, size_t ws_bytes, int64_t M, int N, int K, int accumulate, const float* dy_amax,
                                    const float* x_amax, ttts_reduce_queue* queue, void* stream) {
    return wgrad_single("linear_bwd_weight_h3_parts", WG_H3, WG_PARTS, {dy, x, ws, ws_bytes, M, N, K, 1, 0, 0, 0, dy_amax, x_amax}, dw_parts,
                        dbias_parts, nparts, accumulate, queue, stream);
}

// dw[co,ci,tap] (+)= sum_{b,t} dy[b,t,co] * x[b,t+tap-pad,ci] ; dbias[co] (+)= sum dy
int ttts_conv1d_bwd_weight(const float* dy, const float* x, float* dw, float* dbias, float* ws, size_t ws_bytes, int B,
                           int T, int cin, int cout, int taps, int accumulate, ttts_reduce_queue* queue, void* stream) {
    return wgrad_single("conv1d_bwd_weight", WG_F32, WG_CONV, {dy, x, ws, ws_bytes, 0, cout, cin, taps, B, T, 0, nullptr, nullptr}, &dw, &dbias, 1,
                        accumulate, queue, stream);
}
int ttts_conv1d_bwd_weight_x6(const float* dy, const float* x, float* dw, float* dbias, float* ws, size_t ws_bytes, int B,
                              int T, int cin, int cout, int taps, int accumulate, ttts_reduce_queue* queue, void* stream) {
    return wgrad_single("conv1d_bwd_weight_x6", WG_X6, WG_CONV, {dy, x, ws, ws_bytes, 0, cout, cin, taps, B, T, 0, nullptr, nullptr}, &dw, &dbias, 1,
                        accumulate, queue, stream);
}
int ttts_conv1d_bwd_weight_h3(const float* dy, const float* x, float* dw, float* dbias, float* ws, size_t ws_bytes, int B,
                              int T, int cin, int cout, int taps, int accumulate, const float* dy_amax, const float* x_amax,
                              ttts_reduce_queue* queue, void* stream) {
    return wgrad_single("conv1d_bwd_weight_h3", WG_H3, WG_CONV, {dy, x, ws, ws_bytes, 0, cout, cin, taps, B, T, 0, dy_amax, x_amax}, &dw, &dbias, 1,
                        accumulate, queue, stream);
}

int ttts_wgrad_group_ok(int64_t M, int N, int K, int taps) { return wgrad_class(M, N, K, taps); }

// n <= 4 independent weight gradients as ONE grid (all members of one class, ttts_wgrad_group_ok).  Member i is the problem of
// ttts_linear_bwd_weight_h3 (taps_i = 1; row_shift_i / T_i as its row_shift / T -- the decoder pre-net's go-frame shift) or of
// ttts_conv1d_bwd_weight_h3 (taps_i > 1, M_i = B T_i).  The row splits are planned for the group (same chip-filling target as a
// single launch, shared by the members), so every member writes 1/n of the partial sums a launch of its own would and its
// workgroups walk n times the rows.  Each member's partial sums go to its own workspace and are reduced (queued) as a single one's.
int ttts_wgrad_group(int n, const float* const* dy, const float* const* x, float* const* dw, float* const* dbias,
                     float* const* ws, const size_t* ws_bytes, const int64_t* M, const int* N, const int* K, const int* taps,
                     const int* T, const int* row_shift, int accumulate, const float* const* dy_amax, const float* const* x_amax,
                     ttts_reduce_queue* queue, void* stream_) {
    const char* name = "wgrad_group";
    hipStream_t stream = (hipStream_t)stream_;
    ENTRY_REQUIRE(n >= 1 && n <= WG_GROUP_MAX && dy && x && dw && ws && ws_bytes && M && N && K && taps && T && row_shift && dy_amax && x_amax,
                  "bad arguments");
    WgradProblem pb[WG_GROUP_MAX]; WgradPlan plan[WG_GROUP_MAX]; GemmArgs gs[WG_GROUP_MAX]; int zd[WG_GROUP_MAX];      // (zd: row splits x taps)
    WgradGroup grp = {wgrad_class(M[0], N[0], K[0], taps[0]), 0, 0};
    for (int i = 0; i < n; ++i) {
        pb[i] = {dy[i], x[i], ws[i], ws_bytes[i], M[i], N[i], K[i], taps[i], 0, T[i], row_shift[i], dy_amax[i], x_amax[i], taps[i] > 1,
                 dbias != nullptr && dbias[i] != nullptr};
        ENTRY_REQUIRE(dy[i] && x[i] && dw[i] && ws[i] && dy_amax[i] && x_amax[i], "null pointer (member %d)", i);
        // (the class query answers for any tap count; "same" padding is symmetric for odd ones only, as in the single entries)
        ENTRY_REQUIRE(taps[i] <= 1 || (taps[i] & 1), "member %d: bad dims M=%lld N=%d K=%d taps=%d (a convolution's tap count must be odd)", i,
                      (long long)M[i], N[i], K[i], taps[i]);
        long tiles = 0;
        ENTRY_REQUIRE(grp.cls != 0 && wgrad_class(M[i], N[i], K[i], taps[i], &tiles) == grp.cls && M[i] < (1LL << 31),
                      "member %d (M=%lld N=%d K=%d taps=%d) is not of the group's class %d", i, (long long)M[i], N[i], K[i], taps[i], grp.cls);
        if (int rc = wgrad_check_operands(name, pb[i])) return rc;
        grp.tiles_total += tiles;
        if ((M[i] + HBK - 1) / HBK > grp.nkt_max) grp.nkt_max = (M[i] + HBK - 1) / HBK;
    }
    for (int i = 0; i < n; ++i) {
        plan[i] = plan_wgrad(M[i], N[i], K[i], taps[i], WG_H3, &grp);
        ENTRY_REQUIRE(ws_bytes[i] >= wgrad_layout(plan[i].nsplit, N[i], K[i], taps[i]).floats * sizeof(float), "workspace %d too small", i);
        ENTRY_REQUIRE((taps[i] == 1 && row_shift[i] == 0) || (T[i] > 0 && M[i] % T[i] == 0 && (grp.cls != 2 || T[i] >= 16)),
                      "member %d: a convolution / a shifted linear needs its utterance length", i);
        ENTRY_REQUIRE(taps[i] == 1 || row_shift[i] == 0, "member %d: a convolution takes no row shift of its own", i);
        gs[i] = wgrad_args(pb[i], WG_H3, plan[i]);
        zd[i] = plan[i].nsplit * taps[i];
    }
    int rc = grp.cls == 2 ? launch_wgrad_dma_group(gs, zd, n, stream) : launch_wgrad_h3_group(gs, zd, n, plan[0].tile, stream);
    for (int i = 0; i < n && rc == TTTS_OK; ++i)
        rc = wgrad_reduce(pb[i], plan[i], gs[i].colsum, dw + i, dbias ? dbias + i : nullptr, 1, accumulate != 0, stream, queue);
    return rc;
}
#undef ENTRY_REQUIRE

size_t ttts_conv1d_pack_bytes(int cout, int cin, int taps) { return (size_t)cout * cin * taps * sizeof(float); }

int ttts_conv1d_pack_weight(const float* w, float* w_fwd, float* w_bwd, int cout, int cin, int taps, void* stream) {
    TTTS_REQUIRE(w && (w_fwd || w_bwd), "conv1d_pack_weight: null pointer");
    long n = (long)cout * cin * taps;
    hipLaunchKernelGGL(conv_pack_weight_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, w, w_fwd, w_bwd,
                       cout, cin, taps);
    TTTS_LAUNCH_CHECK("conv_pack_weight_kernel");
    return TTTS_OK;
}

int ttts_gemm_tile_choice(int64_t M, int N, int K, int x6) {
    // which tile the forward / data-gradient dispatch picks for an M x N output: 1 = 64x64, 2 = 128x128, 3 = 64x128,
    // 4 = 128x96 (profiling aid: lets a host-side probe attribute a launch to its kernel instantiation);
    // x6 = 0: fp32 MFMA kernel, 1: bf16x6, 2: fp16x3
    if (x6 == 2) return h3_tile_choice(M, N, K);
    if (N <= 96 && (long)cdiv(M, 128) >= 384) return TILE_128x96;
    return choose_tile(M, N, 1, x6 != 0);
}

size_t ttts_split_bytes(int64_t rows, int64_t cols) { return (size_t)3 * (size_t)rows * (size_t)cols * 2; }

size_t ttts_split_image_bytes(int64_t rows, int64_t cols, int mode, int channels_per_tap, int taps) {
    // bytes of the image ttts_weight_split writes in `mode`: three bf16 planes (modes 0-3), or two f16 planes of the
    // channel-padded image plus the 16-byte tail (modes 4-7)
    if (mode < 4) return ttts_split_bytes(rows, cols);
    const bool conv = h3_mode_base(mode) >= 2;
    return h3_plane_bytes(rows, h3_image_cols(cols, conv ? channels_per_tap : 0, conv ? taps : 0)) + 16;
}

int ttts_weight_split(const float* w, void* planes, int rows, int cols, int mode, int channels_per_tap, int taps,
                      void* stream) {
    // planes[3][rows][cols] bf16 (hi, mid, lo) of a weight re-laid as the K-contiguous B operand; modes in gemm.hip
    TTTS_REQUIRE(w && planes && rows > 0 && cols > 0, "weight_split: bad arguments");
    TTTS_REQUIRE(mode >= 0 && mode <= 11, "weight_split: mode must be 0..11");
    TTTS_REQUIRE(cols % (mode >= 4 ? 4 : BK) == 0, "weight_split: cols=%d must be a multiple of %d", cols, mode >= 4 ? 4 : BK);
    TTTS_REQUIRE((mode < 4 ? mode : h3_mode_base(mode)) < 2 || (channels_per_tap > 0 && taps > 0 && cols == channels_per_tap * taps),
                 "weight_split: conv modes need cols == channels_per_tap * taps");
    if (mode >= 4) {
        // (the fp16x3 image pads the channels of a tap -- all columns of a linear weight -- to a multiple of 32 with zeros:
        // size it with ttts_split_image_bytes)
        TTTS_REQUIRE(h3_mode_base(mode) < 2 || channels_per_tap % 4 == 0, "weight_split: fp16x3 conv image needs channels %% 4 == 0");
        launch_weight_split_h3(w, planes, rows, cols, h3_mode_base(mode), channels_per_tap, taps, (hipStream_t)stream, h3_mode_k16(mode));
        TTTS_LAUNCH_CHECK("weight_split_h3_kernel");
        return TTTS_OK;
    }
    long n = (long)rows * cols;
    hipLaunchKernelGGL(weight_split_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, w,
                       (unsigned short*)planes, rows, cols, mode, channels_per_tap, taps);
    TTTS_LAUNCH_CHECK("weight_split_kernel");
    return TTTS_OK;
}

int64_t ttts_weight_split_units(int64_t rows, int64_t cols, int mode, int channels_per_tap) {
    // workgroups an entry of ttts_weight_split_batched takes: 256 elements each (bf16x6 images), a 32-row x 32-channel
    // tile over all taps each (fp16x3 images)
    // (linear entries may carry the geometry of a stacked image in channels_per_tap / taps: no part of their unit count)
    return mode >= 4 ? h3_split_units(rows, cols, h3_mode_base(mode), h3_mode_base(mode) >= 2 ? channels_per_tap : 0) : (rows * cols + 255) / 256;
}

int ttts_weight_split_batched(const int64_t* descs, int n, int64_t total_blocks, void* stream) {
    // descs (device): n x 8 int64 {w, planes, rows, cols, mode, channels_per_tap, taps, first_block}; first_block are the
    // prefix sums of ttts_weight_split_units(); the caller guarantees the per-entry constraints of ttts_weight_split
    TTTS_REQUIRE(descs && n > 0 && total_blocks > 0 && total_blocks < (1LL << 31), "weight_split_batched: bad arguments");
    hipLaunchKernelGGL(weight_tail_zero_batched_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const long*>(descs), n);
    hipLaunchKernelGGL(weight_amax_batched_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const long*>(descs), n);
    hipLaunchKernelGGL(weight_split_batched_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const long*>(descs), n);
    TTTS_LAUNCH_CHECK("weight_split_batched_kernel");
    return TTTS_OK;
}

int ttts_conv1d_fwd_h3_bn_blocks(int B, int T, int cin, int cout, int taps) {
    return h3_bn_blocks((long)B * T, cout, (long)taps * h3_pad32(cin));
}

int ttts_conv1d_fwd_h3_bn_chunk_rows(int B, int T, int cin, int cout, int taps) {
    // rows of (b, t) one partial covers (0: no partials for this shape): partial i holds rows i * chunk .. of the B T rows, so a
    // caller may finish the statistics of a row range that is a whole number of chunks on its own (the two forwards of a
    // training step run as one batch: ops.ConvBNFn, twin batches)
    return h3_bn_blocks((long)B * T, cout, (long)taps * h3_pad32(cin)) > 0 ? h3_bn_chunk_rows((long)B * T, cout, (long)taps * h3_pad32(cin)) : 0;
}

// ---------------------------------------------------------------------------------------------------------------
// The 17 forward-type entry points: Linear and Conv1d, forward and data gradient, in six FORMS.  All of them are the problem
// C[rows][width] = A[rows][depth (x taps, row-shifted)] . B[width][taps x depth]: three bodies below state the argument checks
// and the GemmArgs once, the entries name their form and pass empty operands for what they lack.
enum GemmForm {
    FORM_F32,       // fp32 MFMA (gemm.hip): fp32 weight as it is
    FORM_X6,        // bf16x6 (gemm.hip): three bf16 weight planes, 6 bytes per element
    FORM_H3,        // fp16x3 (gemm_h3.hip): two f16 planes whose depth is padded to 32, the activation's partial maxima
    FORM_H3I,       // fp16x3 on the LDS-DMA kernel (gemm_h3i.hip), activation IMAGE + per-row inverse scales; K16-major weight image
    FORM_H3D,       // ... with a plain fp32 activation and its partial maxima
    FORM_H3D_IMG    // ... and a HEAD-IMAGE output
};
static int form_depth_mult(GemmForm f) { return f <= FORM_X6 ? BK : f == FORM_H3 ? 4 : 32; }
static int form_width_mult(GemmForm f) { return f <= FORM_X6 ? 1 : f == FORM_H3D_IMG ? 64 : 4; }
static bool form_takes_amax(GemmForm f) { return f == FORM_H3 || f >= FORM_H3D; }

#define ENTRY_REQUIRE(cond, fmt, ...) TTTS_REQUIRE(cond, "%s: " fmt, name, ##__VA_ARGS__)

// the checks every body makes once it knows its rows, reduction depth and output width (dn / wn: what the entry calls them)
static int entry_check_shape(const char* name, GemmForm f, const void* a, const void* b, const void* c, int64_t rows, int depth,
                             const char* dn, int width, const char* wn, int wmult, int taps) {
    const int dmult = form_depth_mult(f);
    if (wmult == 1) ENTRY_REQUIRE(depth % dmult == 0, "%s=%d must be a multiple of %d", dn, depth, dmult);
    ENTRY_REQUIRE(depth % dmult == 0 && width % wmult == 0, "%s=%d must be a multiple of %d and %s=%d of %d", dn, depth, dmult, wn,
                  width, wmult);
    // (the LDS-DMA kernels store whole 16-byte pieces through a descriptor on the output as well)
    ENTRY_REQUIRE(aligned16(a) && aligned16(b) && (f < FORM_H3I || aligned16(c)), "pointers must be 16-byte aligned");
    const uint64_t w_bytes = (uint64_t)width * depth * (f == FORM_X6 ? 6 : 4);      // (the unpadded extent, per tap)
    ENTRY_REQUIRE((uint64_t)rows * depth * 4 < (1ull << 32) && w_bytes < (1ull << 32) && w_bytes * taps < (1ull << 32),
                  "operand larger than 4 GiB");
    return TTTS_OK;
}

// A: rows x depth, B: width rows of taps x depth (fp16x3: x the depth padded to the image's 32-deep k-tiles -- the loader reads
// up to 28 floats past a row's end, the next row or zeros past the buffer, against zero weight columns), C: rows x width
static GemmArgs entry_args(GemmForm f, const void* a, const void* b, void* c, int64_t rows, int depth, int width, int taps,
                           const float* a_amax, const float* a_row_inv, float* c_amax) {
    GemmArgs g = base_args();
    const int dp = f == FORM_H3 ? h3_pad32(depth) : depth;
    g.A = (const float*)a; g.B = (const float*)b; g.C = (float*)c;
    g.M = (int)rows; g.N = width; g.K = taps * dp;
    g.lda = depth; g.ldb = (long)taps * dp; g.ldc = width; g.cin = dp;
    g.a_bytes = (uint32_t)((uint64_t)rows * depth * 4);
    g.b_bytes = (uint32_t)((uint64_t)width * taps * dp * (f == FORM_X6 ? 6 : 4));
    if (form_takes_amax(f)) { g.a_amax = a_amax; g.a_amax_n = H3_AMAX_PARTIALS; }
    if (f >= FORM_H3) { g.b_amax = h3_plane_tail(b, width, (long)taps * dp); g.b_amax_n = 1; }
    g.a_row_inv = a_row_inv;
    g.c_amax = c_amax;
    return g;
}

static int entry_dispatch(GemmForm f, const GemmArgs& g, void* stream, bool b_kc = true) {
    switch (f) {
        case FORM_F32: return b_kc ? dispatch_gemm<true, true>(g, 1, TILE_AUTO, (hipStream_t)stream)
                                   : dispatch_gemm<true, false>(g, 1, TILE_AUTO, (hipStream_t)stream);
        case FORM_X6: return dispatch_split(g, (hipStream_t)stream);
        case FORM_H3: return dispatch_h3(g, (hipStream_t)stream);
        default: return dispatch_h3i(g, (hipStream_t)stream);
    }
}

// y[M,N] = drop(act(x[M,K] . w[N,K]^T + bias)) + residual; row_shift: x read that many rows further inside utterances of T rows
static int linear_fwd_impl(const char* name, GemmForm f, const void* x, const float* x_row_inv, const void* w, const float* bias,
                           const float* residual, void* y, float* y_row_inv, int64_t M, int N, int K, int act, float drop_p,
                           uint64_t seed, const uint64_t* step_seed, int row_shift, int T, const float* x_amax, float* y_amax_out,
                           int amax_section_cols, void* stream) {
    ENTRY_REQUIRE(x && w && y && (!form_takes_amax(f) || x_amax) && (f != FORM_H3I || x_row_inv) && (f != FORM_H3D_IMG || y_row_inv),
                  "null pointer");
    ENTRY_REQUIRE(M > 0 && N > 0 && K > 0 && M < (1LL << 31), "bad dims M=%lld N=%d K=%d", (long long)M, N, K);
    if (int rc = entry_check_shape(name, f, x, w, y, M, K, "K", N, "N", form_width_mult(f), 1)) return rc;
    ENTRY_REQUIRE(act == 0 || act == 1, "act must be 0 (none) or 1 (relu)");
    ENTRY_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "dropout p=%f out of [0,1)", drop_p);
    ENTRY_REQUIRE(row_shift == 0 || (T > 0 && M % T == 0), "row_shift needs T>0 and M %% T == 0");
    ENTRY_REQUIRE(amax_section_cols >= 0 && (amax_section_cols == 0 || (amax_section_cols % 64 == 0 && N % amax_section_cols == 0)),
                  "amax sections must be whole heads that divide N");
    GemmArgs g = entry_args(f, x, w, y, M, K, N, 1, x_amax, x_row_inv, y_amax_out);
    g.shift0 = row_shift; g.T = (row_shift != 0) ? T : 0;
    g.bias = bias; g.act = act;
    if (drop_p > 0.f) { g.drop_thr = drop_threshold(drop_p); g.drop_scale = 1.f / (1.f - drop_p); g.seed = seed; g.step_seed = step_seed; }
    g.residual = residual; g.ldr = N;
    g.c_row_inv = y_row_inv; g.c_amax_sec = amax_section_cols;
    return entry_dispatch(f, g, stream);
}

// dx[M,K] = dy[M,N] . w[N,K] (+ residual), times the relu mask of relu_out and relu_scale (reduction over N).  The fp32 form
// takes w in its natural [N][K] layout; the others its transposed image (ttts_weight_split modes 1 / 5 / 9: [K][N] rows)
static int linear_bwd_data_impl(const char* name, GemmForm f, const void* dy, const float* dy_row_inv, const void* w,
                                const float* residual, float* dx, int64_t M, int N, int K, const float* relu_out, float relu_scale,
                                const float* dy_amax, float* dx_amax_out, void* stream) {
    ENTRY_REQUIRE(dy && w && dx && (!form_takes_amax(f) || dy_amax) && (f != FORM_H3I || dy_row_inv), "null pointer");
    ENTRY_REQUIRE(M > 0 && N > 0 && K > 0 && M < (1LL << 31), "bad dims M=%lld N=%d K=%d", (long long)M, N, K);
    // (fp32: the natural-layout weight is read four neighbouring columns at a time)
    if (int rc = entry_check_shape(name, f, dy, w, dx, M, N, "N", K, "K", f == FORM_F32 ? 4 : form_width_mult(f), 1)) return rc;
    GemmArgs g = entry_args(f, dy, w, dx, M, N, K, 1, dy_amax, dy_row_inv, dx_amax_out);
    if (f == FORM_F32) g.ldb = K;
    g.residual = residual; g.ldr = K;
    g.relu_out = relu_out; g.relu_scale = relu_scale;
    return entry_dispatch(f, g, stream, f != FORM_F32);
}

// same-padded Conv1d over (b, t) rows, zero outside [0, T), pad = (taps - 1) / 2:
//   forward        y[b,t,co]  = bias[co] + sum_{tap,ci} x[b,t+tap-pad,ci] * w[co,ci,tap]     (planes: [co][tap * cin + ci])
//   data gradient  dx[b,t,ci] = sum_{tap,co} dy[b,t-tap+pad,co] * w[co,ci,tap]               (planes: [ci][tap * cout + co])
// -- one problem with the sign of the tap shift and the roles of cin and cout exchanged
static int conv1d_impl(const char* name, GemmForm f, bool fwd, const void* a, const void* planes, const float* bias, float* c, int B,
                       int T, int cin, int cout, int taps, const float* a_amax, float* bn_partials, void* stream) {
    ENTRY_REQUIRE(a && planes && c && (!form_takes_amax(f) || a_amax), "null pointer");
    ENTRY_REQUIRE(B > 0 && T > 0 && cin > 0 && cout > 0 && taps > 0 && (taps & 1), "bad dims B=%d T=%d cin=%d cout=%d taps=%d", B, T,
                  cin, cout, taps);
    ENTRY_REQUIRE((long)B * T < (1L << 31), "B*T too large");
    const int depth = fwd ? cin : cout, width = fwd ? cout : cin, pad = (taps - 1) / 2;
    if (int rc = entry_check_shape(name, f, a, planes, c, (int64_t)B * T, depth, fwd ? "cin" : "cout", width, fwd ? "cout" : "cin",
                                   form_width_mult(f), taps))
        return rc;
    ENTRY_REQUIRE(aligned16(bn_partials), "bn_partials must be 16-byte aligned");
    GemmArgs g = entry_args(f, a, planes, c, (int64_t)B * T, depth, width, taps, a_amax, nullptr, nullptr);
    g.T = T; g.shift0 = fwd ? -pad : pad; g.shift_step = fwd ? 1 : -1;
    g.bias = bias;
    g.bn_ws = bn_partials;          // NULL, or the workspace of ttts_bn_train_stats (fp16x3 forward only)
    return entry_dispatch(f, g, stream);
}
#undef ENTRY_REQUIRE

int ttts_linear_fwd(const float* x, const float* w, const float* bias, const float* residual, float* y, int64_t M, int N, int K,
                    int act, float drop_p, uint64_t seed, const uint64_t* step_seed, int row_shift, int T, void* stream) {
    return linear_fwd_impl("linear_fwd", FORM_F32, x, nullptr, w, bias, residual, y, nullptr, M, N, K, act, drop_p, seed, step_seed,
                           row_shift, T, nullptr, nullptr, 0, stream);
}
int ttts_linear_fwd_x6(const float* x, const void* w_planes, const float* bias, const float* residual, float* y, int64_t M, int N,
                       int K, int act, float drop_p, uint64_t seed, const uint64_t* step_seed, int row_shift, int T, void* stream) {
    return linear_fwd_impl("linear_fwd_x6", FORM_X6, x, nullptr, w_planes, bias, residual, y, nullptr, M, N, K, act, drop_p, seed,
                           step_seed, row_shift, T, nullptr, nullptr, 0, stream);
}
// x_amax: the partial maxima of |x| (ttts_amax_partials or a producer's `*_amax_out`); y_amax_out: NULL, or where max|y| goes
int ttts_linear_fwd_h3(const float* x, const void* w_planes, const float* bias, const float* residual, float* y, int64_t M, int N,
                       int K, int act, float drop_p, uint64_t seed, const uint64_t* step_seed, int row_shift, int T,
                       const float* x_amax, float* y_amax_out, void* stream) {
    return linear_fwd_impl("linear_fwd_h3", FORM_H3, x, nullptr, w_planes, bias, residual, y, nullptr, M, N, K, act, drop_p, seed,
                           step_seed, row_shift, T, x_amax, y_amax_out, 0, stream);
}
int ttts_linear_fwd_h3i(const void* x_image, const float* x_row_inv, const void* w_planes, const float* bias, const float* residual,
                        float* y, int64_t M, int N, int K, int act, float drop_p, uint64_t seed, const uint64_t* step_seed,
                        float* y_amax_out, void* stream) {
    return linear_fwd_impl("linear_fwd_h3i", FORM_H3I, x_image, x_row_inv, w_planes, bias, residual, y, nullptr, M, N, K, act, drop_p,
                           seed, step_seed, 0, 0, nullptr, y_amax_out, 0, stream);
}
/* fp32 activation (per-tensor scale from its partial maxima) on the LDS-DMA kernel: the weight image is the K16-major one
 * (ttts_weight_split modes 8 / 9); arguments otherwise as ttts_linear_fwd_h3 / ttts_linear_bwd_data_h3 without a row shift */
int ttts_linear_fwd_h3d(const float* x, const void* w_planes, const float* bias, const float* residual, float* y, int64_t M, int N,
                        int K, int act, float drop_p, uint64_t seed, const uint64_t* step_seed, const float* x_amax,
                        float* y_amax_out, void* stream) {
    return linear_fwd_impl("linear_fwd_h3d", FORM_H3D, x, nullptr, w_planes, bias, residual, y, nullptr, M, N, K, act, drop_p, seed,
                           step_seed, 0, 0, x_amax, y_amax_out, 0, stream);
}
/* The in-projections of nn.MultiheadAttention (packed q/k/v, or its q and k/v row slices: torch/nn/functional.py:6206+ reached
 * from model/layers.py:54-74 and torch _sa_block) with a HEAD-IMAGE output: y_image has the geometry of the fp32 output (M rows of
 * N 4-byte cells) but holds, per row and 64-column head, {64 f16 hi, 64 f16 lo} of (x W^T + b) * 2^e(row, head);
 * y_row_inv[head * M + row] = 2^-e.  y_amax_out: NULL, or N / amax_section_cols caller-zeroed TTTS_AMAX_SLOTS-float arrays (one per
 * section: q / k / v), each receiving max|y| of its section. */
int ttts_linear_fwd_h3d_img(const float* x, const void* w_planes, const float* bias, void* y_image, float* y_row_inv, int64_t M,
                            int N, int K, const float* x_amax, float* y_amax_out, int amax_section_cols, void* stream) {
    return linear_fwd_impl("linear_fwd_h3d_img", FORM_H3D_IMG, x, nullptr, w_planes, bias, nullptr, y_image, y_row_inv, M, N, K, 0, 0.f,
                           0, nullptr, 0, 0, x_amax, y_amax_out, amax_section_cols, stream);
}

int ttts_linear_bwd_data(const float* dy, const float* w, const float* residual, float* dx, int64_t M, int N, int K,
                         const float* relu_out, float relu_scale, void* stream) {
    return linear_bwd_data_impl("linear_bwd_data", FORM_F32, dy, nullptr, w, residual, dx, M, N, K, relu_out, relu_scale, nullptr,
                                nullptr, stream);
}
int ttts_linear_bwd_data_x6(const float* dy, const void* wt_planes, const float* residual, float* dx, int64_t M, int N, int K,
                            const float* relu_out, float relu_scale, void* stream) {
    return linear_bwd_data_impl("linear_bwd_data_x6", FORM_X6, dy, nullptr, wt_planes, residual, dx, M, N, K, relu_out, relu_scale,
                                nullptr, nullptr, stream);
}
// dy_amax: the partial maxima of |dy| (the dynamic pre-scale of the gradient operand); dx_amax_out: NULL, or where max|dx| goes
int ttts_linear_bwd_data_h3(const float* dy, const void* wt_planes, const float* residual, float* dx, int64_t M, int N, int K,
                            const float* relu_out, float relu_scale, const float* dy_amax, float* dx_amax_out, void* stream) {
    return linear_bwd_data_impl("linear_bwd_data_h3", FORM_H3, dy, nullptr, wt_planes, residual, dx, M, N, K, relu_out, relu_scale,
                                dy_amax, dx_amax_out, stream);
}
int ttts_linear_bwd_data_h3i(const void* dy_image, const float* dy_row_inv, const void* wt_planes, const float* residual, float* dx,
                             int64_t M, int N, int K, const float* relu_out, float relu_scale, float* dx_amax_out, void* stream) {
    return linear_bwd_data_impl("linear_bwd_data_h3i", FORM_H3I, dy_image, dy_row_inv, wt_planes, residual, dx, M, N, K, relu_out,
                                relu_scale, nullptr, dx_amax_out, stream);
}
int ttts_linear_bwd_data_h3d(const float* dy, const void* wt_planes, const float* residual, float* dx, int64_t M, int N, int K,
                             const float* relu_out, float relu_scale, const float* dy_amax, float* dx_amax_out, void* stream) {
    return linear_bwd_data_impl("linear_bwd_data_h3d", FORM_H3D, dy, nullptr, wt_planes, residual, dx, M, N, K, relu_out, relu_scale,
                                dy_amax, dx_amax_out, stream);
}

int ttts_conv1d_fwd(const float* x, const float* w_fwd, const float* bias, float* y, int B, int T, int cin, int cout, int taps,
                    void* stream) {
    return conv1d_impl("conv1d_fwd", FORM_F32, true, x, w_fwd, bias, y, B, T, cin, cout, taps, nullptr, nullptr, stream);
}
int ttts_conv1d_fwd_x6(const float* x, const void* planes_fwd, const float* bias, float* y, int B, int T, int cin, int cout, int taps,
                       void* stream) {
    return conv1d_impl("conv1d_fwd_x6", FORM_X6, true, x, planes_fwd, bias, y, B, T, cin, cout, taps, nullptr, nullptr, stream);
}
int ttts_conv1d_fwd_h3(const float* x, const void* planes_fwd, const float* bias, float* y, int B, int T, int cin, int cout, int taps,
                       const float* x_amax, float* bn_partials, void* stream) {
    return conv1d_impl("conv1d_fwd_h3", FORM_H3, true, x, planes_fwd, bias, y, B, T, cin, cout, taps, x_amax, bn_partials, stream);
}
int ttts_conv1d_bwd_data(const float* dy, const float* w_bwd, float* dx, int B, int T, int cin, int cout, int taps, void* stream) {
    return conv1d_impl("conv1d_bwd_data", FORM_F32, false, dy, w_bwd, nullptr, dx, B, T, cin, cout, taps, nullptr, nullptr, stream);
}
int ttts_conv1d_bwd_data_x6(const float* dy, const void* planes_bwd, float* dx, int B, int T, int cin, int cout, int taps,
                            void* stream) {
    return conv1d_impl("conv1d_bwd_data_x6", FORM_X6, false, dy, planes_bwd, nullptr, dx, B, T, cin, cout, taps, nullptr, nullptr,
                       stream);
}
int ttts_conv1d_bwd_data_h3(const float* dy, const void* planes_bwd, float* dx, int B, int T, int cin, int cout, int taps,
                            const float* dy_amax, void* stream) {
    return conv1d_impl("conv1d_bwd_data_h3", FORM_H3, false, dy, planes_bwd, nullptr, dx, B, T, cin, cout, taps, dy_amax, nullptr,
                       stream);
}

}  // extern "C"
