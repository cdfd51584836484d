// Scaled dot-product attention for heads of 128 columns (head_dim 65..128, narrower ones zero-padded) forward + backward on
// fp32 MFMA, gfx950.  The same three call sites as attention.hip -- encoder self-attention, decoder masked self-attention,
// encoder-decoder cross-attention with the per-head post-dropout weights -- and the same conventions: masks from `key_lens`
// in-kernel, a query row without a live key gives zeros, dropout from the counter-based (site seed, row, key) hash.
//
// Orientation as in attention.hip ("key on the accumulator rows, query on the lane"): S^T[key][query] = K . (Q*scale)^T on
// v_mfma_f32_32x32x2_f32 with K from LDS as the A operand and the lane's own query row in registers as the B operand, so
// row max / row sum are lane-local plus one lane^32 exchange and P is already the B operand of O^T += V^T . P^T.  What a
// 128-column head changes:
//  * 64 two-deep steps per score tile.  The contraction order is free, so step j pairs column j (lanes 0-31) with column
//    64 + j (lanes 32-63): a lane's B operand is 64 CONTIGUOUS floats of its row, loaded straight from global memory
//    (16 x 16 bytes per lane, rows past the end read as zeros through the buffer descriptor) -- no LDS round trip.
//  * four 32x32 accumulators for O^T / dQ^T / dK^T / dV^T, stored as two 64-column halves through the per-wave transpose.
//  * 32-row stages: two staged operands at 129 floats per row are 33 KB, inside the static LDS limit.
//  * the backward kernels hold 128 (dQ) resp. 256 (dK/dV) floats of operand rows and accumulators per lane next to the
//    score tiles: they are built for one wave per SIMD (the 512-register file); the compiler's report is in DESIGN.md.
//
// Row statistics: the forward writes the final row maximum m (0 for a row without a live key) and the row sum l of
// exp(s - m) as two (B, H, Tq) planes; the backward forms p = exp(s - m) / l from bit-identical score accumulators, i.e.
// the forward's own probabilities whatever the scores' magnitude (from lse alone they are only good to ulp(lse)).  A row
// whose l is exactly 1.0f is one-hot in fp32: torch's softmax backward of such a row is exactly zero, so its score
// gradient is taken as zero instead of the rounding of delta against dP.
#include <type_traits>
#include "attention_common.h"

namespace ttts {

// lane-resident B operand: reg[j] = X[row][64 * half + j] * scale (zeros for a row past the end)
__device__ __forceinline__ void wide_load_lane_row(const RowSrc& src, long row, int half, float scale, float (&reg)[64]) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float4 v = row_load4(src, row, 16 * half + i);
        reg[4 * i] = v.x * scale; reg[4 * i + 1] = v.y * scale; reg[4 * i + 2] = v.z * scale; reg[4 * i + 3] = v.w * scale;
    }
}
// one 32x32 tile of A . B^T over the 128 columns: A rows from LDS (stride WLD), B the lane's row
__device__ __forceinline__ void wide_dot(const float* tile, int l31, int half, const float (&reg)[64], f32x16& s) {
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int j = 0; j < 64; ++j)
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(tile[l31 * WLD + 64 * half + j], reg[j], s, 0, 0, 0);
}
// =====================================================================================  forward
// MASKED (every kernel of this file): the masks are tensors (AttnMaskArgs) on top of the ones derived from `key_lens` -- see
// attn_alive_masked.  The mask loads are issued with the stage's operand loads; a row that no key is left for gives zeros like
// an utterance without keys.
template <bool MASKED> using WideArgs = std::conditional_t<MASKED, AttnMaskArgs, AttnArgs>;
// DATTN (backward kernels, non-causal MASKED forms only): the weights the forward wrote have a gradient dA of their own
// (AttnDattnArgs).  With A = D o P / (1 - p) as written: dA_tot = dO . V + dA, dS = P o (D / (1 - p) dA_tot - delta),
// delta = dO . O + sum_n A dA.  The second term of delta is in `a.delta` when the dQ kernel starts (attn_dattn_rowdot_kernel).
template <bool MASKED, bool DATTN> using WideBwdArgs = std::conditional_t<DATTN, AttnDattnArgs, WideArgs<MASKED>>;

template <bool CAUSAL, bool WRITE_A, bool MASKED = false>
__global__ __launch_bounds__(256, 2) void attn_wide_fwd_kernel(WideArgs<MASKED> a) {
    const uint64_t seed_eff = site_seed(a.seed, a.step_seed);
    const uint32_t thr16 = a.thr << 16;
    __shared__ __attribute__((aligned(16))) float smem[WSMEM_FLOATS];
    __shared__ float ptile_all[WRITE_A ? 4 * 32 * 33 : 1];
    float* Ks = smem;                   // [WKB][129]
    float* Vs = smem + WKB * WLD;       // [WKB][128]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    float* ptile = ptile_all + (WRITE_A ? wave * 32 * 33 : 0);
    // grid = (B*H, query blocks), heaviest block first for the causal form (last query block = longest key range)
    const int qblk = CAUSAL ? (gridDim.y - 1 - blockIdx.y) : blockIdx.y;
    const int h = blockIdx.x % a.H, b = blockIdx.x / a.H;
    const int q0 = qblk * QB, qw0 = q0 + wave * 32;
    const int qg = qw0 + l31;
    float* scratch = smem + wave * 32 * KT_LD;

    const int klen = attn_klen(a.key_lens, b, a.Tk);
    const KeyRange kr = key_range<CAUSAL, WRITE_A, WKB>(klen, a.Tk, q0, qw0);

    const float* qb_ = a.q + (long)b * a.Tq * a.ldq + h * WHD;
    const float* kb_ = a.k + (long)b * a.Tk * a.ldk + h * WHD;
    const float* vb_ = a.v + (long)b * a.Tk * a.ldv + h * WHD;

    float qreg[64];
    wide_load_lane_row(row_src(qb_, a.Tq, a.ldq), qg, half, a.qscale, qreg);

    float m = NEG_INF, l = 0.f;
    f32x16 o[4];
#pragma unroll
    for (int blk = 0; blk < 4; ++blk)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[blk][r] = 0.f;

    const long arow = ((long)(b * a.H + h) * a.Tq);   // row base of the (B,H,Tq,*) outputs
    const uint32_t rowid = (uint32_t)(arow + qg);

    // MASKED: the lane's 16 mask values and the tile's dead-key bits of the stage in flight (unused otherwise)
    float mk[MASKED ? 16 : 1];
    uint32_t dbits = 0;
    RowSrc msrc;
    __amdgpu_buffer_rsrc_t dsrc;
    if constexpr (MASKED) { msrc = mask_src(a, b, h); dsrc = dead_src(a, b); }

    auto drop16 = [&](float (&p)[16], int key0) { attn_drop16<true>(p, seed_eff, rowid, key0, half, thr16, a.drop_scale); };
    // online row max / row sum over one masked score tile; -> the factor the running sums shrink by
    auto online = [&](f32x16& s, int key0, float (&p)[16]) -> float {
        float mx = NEG_INF;
        if constexpr (MASKED) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s[r] = attn_alive_masked<CAUSAL>(key0 + acc_row(r, half), klen, qg, (dbits >> acc_row(r, 0)) & 1u, mk[r]) ? s[r] + mk[r] : NEG_INF;
                mx = fmaxf(mx, s[r]);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s[r] = attn_alive<CAUSAL>(key0 + acc_row(r, half), klen, qg) ? s[r] : NEG_INF;
                mx = fmaxf(mx, s[r]);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m, mx);
        const float m_use = (m_new == NEG_INF) ? 0.f : m_new;
        const float alpha = __expf(m - m_use);
        float ps = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) { p[r] = __expf(s[r] - m_use); ps += p[r]; }
        l = l * alpha + ps;
        m = m_new;
        return alpha;
    };

    if (WRITE_A) {
        // ---------------- pass 1: row max / row sum only
        for (int t = 0; t < kr.nst_live; ++t) {
            __syncthreads();
            if constexpr (MASKED) {
                mask_load_row16(msrc, qg, t * WKB, half, mk);
                dbits = dead_tile_bits(dsrc, t * WKB, l31, half);
            }
            stage_rows<WHD, true>(kb_, (long)t * WKB, a.Tk, a.ldk, tid, Ks, 1.f);
            __syncthreads();
            f32x16 s;
            float p[16];
            wide_dot(Ks, l31, half, qreg, s);
            online(s, t * WKB, p);
        }
        l = l + __shfl_xor(l, 32, 64);
    }

    const float m_fin = (m == NEG_INF) ? 0.f : m;
    const float inv_l = (l > 0.f) ? 1.f / l : 0.f;

    // ---------------- main pass
    for (int t = 0; t < kr.nst; ++t) {
        __syncthreads();
        if constexpr (MASKED) {
            mask_load_row16(msrc, qg, t * WKB, half, mk);
            dbits = dead_tile_bits(dsrc, t * WKB, l31, half);
        }
        stage_rows<WHD, true>(kb_, (long)t * WKB, a.Tk, a.ldk, tid, Ks, 1.f);
        stage_rows<WHD, false>(vb_, (long)t * WKB, a.Tk, a.ldv, tid, Vs, 1.f);
        __syncthreads();
        const int key0 = t * WKB;
        if (key0 < kr.wave_kend) {      // else: tile entirely above this wave's causal frontier / past the keys
            f32x16 s;
            wide_dot(Ks, l31, half, qreg, s);
            float p[16];
            if (WRITE_A && MASKED) {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    p[r] = attn_alive_masked<CAUSAL>(key0 + acc_row(r, half), klen, qg, (dbits >> acc_row(r, 0)) & 1u, mk[r])
                               ? __expf((s[r] + mk[r]) - m_fin) * inv_l : 0.f;
            } else if (WRITE_A) {
#pragma unroll
                for (int r = 0; r < 16; ++r) p[r] = attn_alive<CAUSAL>(key0 + acc_row(r, half), klen, qg) ? __expf(s[r] - m_fin) * inv_l : 0.f;
            } else {
                const float alpha = online(s, key0, p);
#pragma unroll
                for (int blk = 0; blk < 4; ++blk)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[blk][r] *= alpha;
            }
            if (a.thr != 0u) drop16(p, key0);
            if (WRITE_A) {
                // transpose the 32(key) x 32(query) tile through a small per-wave LDS buffer so every weight row leaves
                // as a 128-B segment
#pragma unroll
                for (int r = 0; r < 16; ++r) ptile[l31 * 33 + acc_row(r, half)] = p[r];
                wave_lds_sync();
#pragma unroll 4
                for (int i = 0; i < 16; ++i) {
                    const int qrow = 2 * i + half;
                    const float v = ptile[qrow * 33 + l31];
                    const int q_g = qw0 + qrow, key_g = key0 + l31;
                    if (q_g < a.Tq && key_g < a.Tk) a.attn[(arow + q_g) * a.Tk + key_g] = v;
                }
                wave_lds_sync();
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int krow = acc_row(r, half);
#pragma unroll
                for (int blk = 0; blk < 4; ++blk)
                    o[blk] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[krow * WHD + 32 * blk + l31], p[r], o[blk], 0, 0, 0);
            }
        }
    }

    float out_scale = 1.f, l_fin = l;
    if (!WRITE_A) {
        l_fin = l + __shfl_xor(l, 32, 64);
        out_scale = (l_fin > 0.f) ? 1.f / l_fin : 0.f;
    }
    if (half == 0 && qg < a.Tq) {
        a.rowstat[arow + qg] = (m == NEG_INF) ? 0.f : m;      // (single-pass form: m reached its final value in the main pass)
        a.rowstat[(long)a.B * a.H * a.Tq + arow + qg] = l_fin;
    }
#pragma unroll
    for (int blk = 0; blk < 4; ++blk)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[blk][r] *= out_scale;
    __syncthreads();
    wave_store_rows(o, scratch, a.o + (long)b * a.Tq * a.ldo + h * WHD, qw0, a.Tq, a.ldo, lane, 1.f);
}

// =====================================================================================  backward: dQ (+ delta)
// delta[row] = sum_n A[row][n] dA[row][n] over the Tk keys of one (b, h, q) row: one wave per row, lane j takes keys j, j + 64,
// ... in ascending order and the 64 partial sums meet in a fixed xor tree -- the same bits whatever the grid or arrival order
__global__ __launch_bounds__(256) void attn_dattn_rowdot_kernel(const float* attn, const float* d_attn, long stride_b, long stride_h,
                                                                int ld, float* delta, int H, int Tq, int Tk, long rows) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const long t = row % Tq, bh = row / Tq;
    const float* ar = attn + row * Tk;
    const float* gr = d_attn + (bh / H) * stride_b + (bh % H) * stride_h + t * ld;
    float acc = 0.f;
    for (int n = lane; n < Tk; n += 64) acc = fmaf(ar[n], gr[n], acc);
    acc = wave_sum(acc);
    if (lane == 0) delta[row] = acc;
}

template <bool CAUSAL, bool MASKED = false, bool DATTN = false>
__global__ __launch_bounds__(256, 1) void attn_wide_bwd_dq_kernel(WideBwdArgs<MASKED, DATTN> a) {
    static_assert(!DATTN || (MASKED && !CAUSAL), "the weights are written by the non-causal form only; DATTN rides on MASKED");
    const uint64_t seed_eff = site_seed(a.seed, a.step_seed);
    const uint32_t thr16 = a.thr << 16;
    __shared__ __attribute__((aligned(16))) float smem[WSMEM_FLOATS];
    float* Ks = smem;                   // [WKB][129]
    float* Vs = smem + WKB * WLD;       // [WKB][129]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const int qblk = CAUSAL ? (gridDim.y - 1 - blockIdx.y) : blockIdx.y;
    const int h = blockIdx.x % a.H, b = blockIdx.x / a.H;
    const int q0 = qblk * QB, qw0 = q0 + wave * 32;
    const int qg = qw0 + l31;
    float* scratch = smem + wave * 32 * KT_LD;

    const int klen = attn_klen(a.key_lens, b, a.Tk);
    const KeyRange kr = key_range<CAUSAL, false, WKB>(klen, a.Tk, q0, qw0);

    const float* qb_ = a.q + (long)b * a.Tq * a.ldq + h * WHD;
    const float* kb_ = a.k + (long)b * a.Tk * a.ldk + h * WHD;
    const float* vb_ = a.v + (long)b * a.Tk * a.ldv + h * WHD;
    const float* ob_ = a.o + (long)b * a.Tq * a.ldo + h * WHD;
    const float* gb_ = a.dout + (long)b * a.Tq * a.ldo + h * WHD;
    const long arow = ((long)(b * a.H + h) * a.Tq);
    const uint32_t rowid = (uint32_t)(arow + qg);

    float qreg[64], greg[64];
    wide_load_lane_row(row_src(qb_, a.Tq, a.ldq), qg, half, a.qscale, qreg);
    wide_load_lane_row(row_src(gb_, a.Tq, a.ldo), qg, half, 1.f, greg);
    float delta = 0.f;
    {
        const RowSrc osrc = row_src(ob_, a.Tq, a.ldo);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float4 v = row_load4(osrc, qg, 16 * half + i);
            delta += greg[4 * i] * v.x + greg[4 * i + 1] * v.y + greg[4 * i + 2] * v.z + greg[4 * i + 3] * v.w;
        }
    }
    delta += __shfl_xor(delta, 32, 64);
    if constexpr (DATTN) delta += (qg < a.Tq) ? a.delta[arow + qg] : 0.f;      // sum_n A dA of the row (attn_dattn_rowdot_kernel)
    if (half == 0 && qg < a.Tq) a.delta[arow + qg] = delta;
    const float m_q = (qg < a.Tq) ? a.rowstat[arow + qg] : 0.f;
    const float l_q = (qg < a.Tq) ? a.rowstat[(long)a.B * a.H * a.Tq + arow + qg] : 0.f;
    const float inv_l = (l_q > 0.f) ? 1.f / l_q : 0.f;
    const bool one_hot = l_q == 1.0f;

    f32x16 dq[4];
#pragma unroll
    for (int blk = 0; blk < 4; ++blk)
#pragma unroll
        for (int r = 0; r < 16; ++r) dq[blk][r] = 0.f;

    float mk[MASKED ? 16 : 1];
    uint32_t dbits = 0;
    RowSrc msrc;
    __amdgpu_buffer_rsrc_t dsrc;
    if constexpr (MASKED) { msrc = mask_src(a, b, h); dsrc = dead_src(a, b); }
    // DATTN: the lane's 16 values of its dA row of the stage in flight, loaded like the mask row
    float da[DATTN ? 16 : 1];
    RowSrc gsrc;
    if constexpr (DATTN) gsrc = dattn_src(a, b, h);

    for (int t = 0; t < kr.nst; ++t) {
        __syncthreads();
        if constexpr (MASKED) {
            mask_load_row16(msrc, qg, t * WKB, half, mk);
            dbits = dead_tile_bits(dsrc, t * WKB, l31, half);
        }
        if constexpr (DATTN) mask_load_row16(gsrc, qg, t * WKB, half, da);
        stage_rows<WHD, true>(kb_, (long)t * WKB, a.Tk, a.ldk, tid, Ks, 1.f);
        stage_rows<WHD, true>(vb_, (long)t * WKB, a.Tk, a.ldv, tid, Vs, 1.f);
        __syncthreads();
        const int key0 = t * WKB;
        if (key0 < kr.wave_kend) {
            f32x16 s, dp;
            wide_dot(Ks, l31, half, qreg, s);
            wide_dot(Vs, l31, half, greg, dp);
            float ds[16];
#pragma unroll
            for (int r = 0; r < 16; r += 4) {
                const int key_g = key0 + acc_row(r, half);
                // MASKED: the hash is taken and applied whether dropout is on or not (thr16 = 0 keeps everything, at scale 1): a
                // branch on `a.thr` right behind the dP MFMAs would leave its shorter side too few wait states before the first
                // read of their accumulator ("A read that came too early")
                uint32_t qh = 0;
                if (MASKED || a.thr != 0u) qh = attn_quad_hash(seed_eff, rowid, (uint32_t)key_g >> 2);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int kg = key_g + e;
                    float p;
                    if constexpr (MASKED)
                        p = attn_alive_masked<CAUSAL>(kg, klen, qg, (dbits >> acc_row(r + e, 0)) & 1u, mk[r + e])
                                ? __expf((s[r + e] + mk[r + e]) - m_q) * inv_l : 0.f;
                    else
                        p = attn_alive<CAUSAL>(kg, klen, qg) ? __expf(s[r + e] - m_q) * inv_l : 0.f;
                    float g = dp[r + e];
                    // DATTN: dA of a key that is not alive is whatever lies there; selected, not branched on (straight-line code
                    // from the dP MFMAs to the first read of their accumulator)
                    if constexpr (DATTN)
                        g += attn_alive_masked<CAUSAL>(kg, klen, qg, (dbits >> acc_row(r + e, 0)) & 1u, mk[r + e]) ? da[r + e] : 0.f;
                    if (MASKED || a.thr != 0u) g = attn_drop1<true>(g, qh, e, thr16, a.drop_scale);
                    ds[r + e] = one_hot ? 0.f : p * (g - delta);
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int krow = acc_row(r, half);
#pragma unroll
                for (int blk = 0; blk < 4; ++blk)
                    dq[blk] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[krow * WLD + 32 * blk + l31], ds[r], dq[blk], 0, 0, 0);
            }
        }
    }
    __syncthreads();
    wave_store_rows(dq, scratch, a.dq + (long)b * a.Tq * a.lddq + h * WHD, qw0, a.Tq, a.lddq, lane, a.qscale);
}

// =====================================================================================  backward: dK, dV
template <bool CAUSAL, bool MASKED = false, bool DATTN = false>
__global__ __launch_bounds__(256, 1) void attn_wide_bwd_dkv_kernel(WideBwdArgs<MASKED, DATTN> a) {
    static_assert(!DATTN || (MASKED && !CAUSAL), "the weights are written by the non-causal form only; DATTN rides on MASKED");
    const uint64_t seed_eff = site_seed(a.seed, a.step_seed);
    const uint32_t thr16 = a.thr << 16;
    __shared__ __attribute__((aligned(16))) float smem[WSMEM_FLOATS];
    __shared__ float m_s[WKB], il_s[WKB], delta_s[WKB], hot_s[WKB];
    float* Qs = smem;                   // [WKB][129]
    float* Gs = smem + WKB * WLD;       // [WKB][129]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const int kblk = blockIdx.y;          // ascending = heaviest first for the causal form (key block 0 meets every query)
    const int h = blockIdx.x % a.H, b = blockIdx.x / a.H;
    const int k0 = kblk * QB, kw0 = k0 + wave * 32;
    const int kg = kw0 + l31;
    float* scratch = smem + wave * 32 * KT_LD;

    const int klen = attn_klen(a.key_lens, b, a.Tk);

    const float* qb_ = a.q + (long)b * a.Tq * a.ldq + h * WHD;
    const float* kb_ = a.k + (long)b * a.Tk * a.ldk + h * WHD;
    const float* vb_ = a.v + (long)b * a.Tk * a.ldv + h * WHD;
    const float* gb_ = a.dout + (long)b * a.Tq * a.ldo + h * WHD;
    const long arow = ((long)(b * a.H + h) * a.Tq);
    const long plane = (long)a.B * a.H * a.Tq;

    float kreg[64], vreg[64];
    wide_load_lane_row(row_src(kb_, a.Tk, a.ldk), kg, half, 1.f, kreg);
    wide_load_lane_row(row_src(vb_, a.Tk, a.ldv), kg, half, 1.f, vreg);

    f32x16 dk[4], dv[4];
#pragma unroll
    for (int blk = 0; blk < 4; ++blk)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dk[blk][r] = 0.f; dv[blk][r] = 0.f; }

    const int nqs = (a.Tq + WKB - 1) / WKB;
    const int qs_begin = attn_qs_begin<CAUSAL, WKB>(k0, klen, nqs);

    // MASKED: the lane's key is dead or not once and for all; its mask column arrives 16 queries per stage and waits in a
    // lane-private LDS column like the staged operands (held in registers across the stage it costs the causal form a spill)
    __shared__ float mask_s[MASKED ? 4 * 16 * 64 : 1];
    float* mcol = mask_s + (MASKED ? wave * 16 * 64 + lane : 0);
    bool kdead = false;
    RowSrc msrc;
    if constexpr (MASKED) { msrc = mask_src(a, b, h); kdead = dead_load(dead_src(a, b), kg); }
    // DATTN: the lane's dA column arrives and waits the same way, in a further lane-private column of WIDE_DATTN_LDS bytes of
    // dynamic LDS (with it the kernel holds more than 64 KB: the launch opts in, attn_launch_bwd_pair)
    float* dacol = nullptr;
    RowSrc gsrc;
    if constexpr (DATTN) {
        extern __shared__ float dattn_s[];
        dacol = dattn_s + wave * 16 * 64 + lane;
        gsrc = dattn_src(a, b, h);
    }

    for (int qs = qs_begin; qs < nqs; ++qs) {
        __syncthreads();
        stage_rows<WHD, true>(qb_, (long)qs * WKB, a.Tq, a.ldq, tid, Qs, a.qscale);
        stage_rows<WHD, true>(gb_, (long)qs * WKB, a.Tq, a.ldo, tid, Gs, 1.f);
        if constexpr (MASKED) {
            float mk[16];
            mask_load_col16(msrc, qs * WKB, kg, half, mk);
#pragma unroll
            for (int r = 0; r < 16; ++r) mcol[r * 64] = mk[r];
        }
        if constexpr (DATTN) {
            float dav[16];
            mask_load_col16(gsrc, qs * WKB, kg, half, dav);
#pragma unroll
            for (int r = 0; r < 16; ++r) dacol[r * 64] = dav[r];
        }
        if (tid < WKB) {
            const int q = qs * WKB + tid;
            const float lq = (q < a.Tq) ? a.rowstat[plane + arow + q] : 0.f;
            m_s[tid] = (q < a.Tq) ? a.rowstat[arow + q] : 0.f;
            il_s[tid] = (lq > 0.f) ? 1.f / lq : 0.f;
            hot_s[tid] = (lq == 1.0f) ? 1.f : 0.f;
            delta_s[tid] = (q < a.Tq) ? a.delta[arow + q] : 0.f;
        }
        __syncthreads();
        const int qt0 = qs * WKB;
        if (!CAUSAL || qt0 + 31 >= kw0) {         // else: every query of the tile precedes this wave's keys
            f32x16 s, dp;
            wide_dot(Qs, l31, half, kreg, s);
            uint32_t okbits = 0;      // MASKED: bit r = the key is alive for the query of register r, a query there is (the mask values end here)
            if constexpr (MASKED) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float mk = mcol[r * 64];
                    const int q_g = qt0 + acc_row(r, half);
                    okbits |= (uint32_t)(attn_alive_masked<CAUSAL>(kg, klen, q_g, kdead, mk) & (q_g < a.Tq)) << r;
                    s[r] += mk;
                }
            }
            wide_dot(Gs, l31, half, vreg, dp);
            float pd[16], ds[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qrow = acc_row(r, half);
                const int q_g = qt0 + qrow;
                float p;
                if constexpr (MASKED) {
                    // the row's statistics are read and the exponent is taken whether the key is alive or not, and the result
                    // is selected: no lane-dependent branch may stand between the dP MFMAs and the first read of their
                    // accumulator (the compiler counts the wait that read needs through a block which a wave whose lanes are
                    // all dead skips)
                    const float e = __expf(s[r] - m_s[qrow]) * il_s[qrow];
                    p = ((okbits >> r) & 1u) ? e : 0.f;
                } else {
                    const bool live = attn_alive<CAUSAL>(kg, klen, q_g) && q_g < a.Tq;
                    p = live ? __expf(s[r] - m_s[qrow]) * il_s[qrow] : 0.f;
                }
                float g = dp[r];
                if constexpr (DATTN) g += ((okbits >> r) & 1u) ? dacol[r * 64] : 0.f;
                float pk = p;
                if (a.thr != 0u) {
                    const bool keep = attn_keep(seed_eff, (uint32_t)(arow + q_g), (uint32_t)kg, thr16);
                    g = keep ? g * a.drop_scale : 0.f;
                    pk = keep ? p * a.drop_scale : 0.f;
                }
                pd[r] = pk;
                ds[r] = (hot_s[qrow] != 0.f) ? 0.f : p * (g - delta_s[qrow]);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qrow = acc_row(r, half);
#pragma unroll
                for (int blk = 0; blk < 4; ++blk) {
                    dv[blk] = __builtin_amdgcn_mfma_f32_32x32x2f32(Gs[qrow * WLD + 32 * blk + l31], pd[r], dv[blk], 0, 0, 0);
                    dk[blk] = __builtin_amdgcn_mfma_f32_32x32x2f32(Qs[qrow * WLD + 32 * blk + l31], ds[r], dk[blk], 0, 0, 0);
                }
            }
        }
    }
    __syncthreads();
    wave_store_rows(dk, scratch, a.dk + (long)b * a.Tk * a.lddk + h * WHD, kw0, a.Tk, a.lddk, lane, 1.f);
    wave_store_rows(dv, scratch, a.dv + (long)b * a.Tk * a.lddv + h * WHD, kw0, a.Tk, a.lddv, lane, 1.f);
}

}  // namespace ttts

using namespace ttts;

constexpr int WIDE_DATTN_LDS = 4 * 16 * 64 * 4;      // the dA columns of the DATTN dK/dV kernel: 16 floats per lane, dynamic LDS

// ---- host side: the five entry points are names for two bodies, wide_fwd and wide_bwd.  An entry passes its own name (every
// refusal starts with it), empty operands for what its signature lacks, and its form: WIDE_PLAIN takes no mask operands (the
// kernels of AttnArgs), WIDE_MASKED requires at least one mask (the MASKED kernels), WIDE_DATTN (backward only) requires attn and
// d_attn and takes masks or none (the DATTN kernels: non-causal, MASKED).  Order of the checks: null pointers, attn_check,
// attn_check_grad_strides (backward), wide_dattn_check (WIDE_DATTN), wide_mask_check (a mask given or required), causal with
// weights (forward), 16-byte alignment of the operands.
enum WideForm { WIDE_PLAIN, WIDE_MASKED, WIDE_DATTN };
// a (B | 1, H | 1, Tq, Tk) fp32 operand whose rows the kernels read where they lie: the additive mask, the gradient of the weights
struct WideSlices { const float* p; long ld, stride_b, stride_h; };
struct WideMask { WideSlices add; const uint8_t* key_dead; long ldd; };      // the mask operands of the _masked / _dattn entry points
struct WideDattn { const float* attn; WideSlices d; };                       // ttts_attention_bwd_wide_dattn: the weights, their gradient

// refused before any launch, each refusal naming its value; `what` / `ptr` / `ld` / `stride`: the operand's names in the refusals
static int wide_slices_check(const char* name, const char* what, const char* ptr, const char* ld, const char* stride, const WideSlices& s,
                             int Tq, int Tk) {
    TTTS_REQUIRE(s.ld >= Tk && s.ld % 4 == 0, "%s: the %s row stride must be a multiple of 4 floats and >= Tk (%s %ld, Tk %d)",
                 name, what, ld, s.ld, Tk);
    TTTS_REQUIRE(s.stride_b >= 0 && s.stride_h >= 0, "%s: %s strides must not be negative (%s_stride_b %ld, %s_stride_h %ld)",
                 name, what, stride, s.stride_b, stride, s.stride_h);
    TTTS_REQUIRE(((uintptr_t)s.p & 15) == 0 && s.stride_b % 4 == 0 && s.stride_h % 4 == 0,
                 "%s: %s must be 16-byte aligned in every (batch, head) slice (address %p, %s_stride_b %ld, %s_stride_h %ld)",
                 name, ptr, (const void*)s.p, stride, s.stride_b, stride, s.stride_h);
    TTTS_REQUIRE((long)Tq * s.ld < (1L << 30), "%s: one %s slice exceeds 4 GiB (Tq %d, %s %ld)", name, what, Tq, ld, s.ld);
    return TTTS_OK;
}
static int wide_mask_check(const char* name, const WideMask& m, int Tq, int Tk) {
    TTTS_REQUIRE(m.add.p || m.key_dead, "%s: add_mask and key_dead are both NULL (use the unmasked entry point)", name);
    if (m.add.p) {
        int rc = wide_slices_check(name, "mask", "add_mask", "ldm", "mask", m.add, Tq, Tk);
        if (rc) return rc;
    }
    TTTS_REQUIRE(!m.key_dead || m.ldd >= Tk, "%s: the dead-key row stride must be >= Tk (ldd %ld, Tk %d)", name, m.ldd, Tk);
    return TTTS_OK;
}
static void wide_mask_fill(AttnMaskArgs& a, const WideMask& m) {
    a.add_mask = m.add.p; a.key_dead = m.key_dead;
    a.mask_stride_b = m.add.stride_b; a.mask_stride_h = m.add.stride_h;
    a.ldm = m.add.p ? (int)m.add.ld : 4; a.ldd = (int)m.ldd;
}
static int wide_dattn_check(const char* name, const WideDattn& g, int causal, int Tq, int Tk) {
    TTTS_REQUIRE(g.attn, "%s: attn is NULL (the forward's weights are required)", name);
    TTTS_REQUIRE(g.d.p, "%s: d_attn is NULL (use ttts_attention_bwd_wide / _masked without a gradient of the weights)", name);
    TTTS_REQUIRE(!causal, "%s: the weights are only written by the non-causal (cross) form (causal %d)", name, causal);
    return wide_slices_check(name, "d_attn", "d_attn", "ld_dattn", "dattn", g.d, Tq, Tk);
}

// One AttnDattnArgs is filled whatever the form; each launcher gets the base its kernels take (AttnArgs, AttnMaskArgs), i.e. the
// leading bytes of it.  Without a mask the descriptors are empty (s + 0.f == s), which is what WIDE_DATTN runs on then.
static int wide_fwd(const char* entry, WideForm form, const float* q, const float* k, const float* v, float* o, float* rowstat,
                    float* attn, const int64_t* key_lens, int B, int H, int Tq, int Tk, int ldq, int ldk, int ldv, int ldo, int causal,
                    float q_scale, float drop_p, uint64_t seed, const uint64_t* step_seed, const WideMask& m, hipStream_t stream) {
    TTTS_REQUIRE(q && k && v && o && rowstat && key_lens, "%s: null pointer", entry);
    int rc = attn_check(entry, WHD, B, H, Tq, Tk, ldq, ldk, ldv, ldo, causal, drop_p);
    if (!rc && form == WIDE_MASKED) rc = wide_mask_check(entry, m, Tq, Tk);
    if (rc) return rc;
    TTTS_REQUIRE(!(causal && attn), "%s: the weights are only written by the non-causal (cross) form", entry);
    TTTS_REQUIRE((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) & 15) == 0, "%s: q/k/v must be 16-byte aligned", entry);
    AttnDattnArgs a = {};
    attn_fill(a, key_lens, B, H, Tq, Tk, ldq, ldk, ldv, ldo, q_scale, drop_p, seed, step_seed);
    wide_mask_fill(a, m);
    a.q = q; a.k = k; a.v = v; a.o = o; a.rowstat = rowstat; a.attn = attn;
    if (form == WIDE_MASKED)
        return attn_launch_fwd("attn_wide_fwd_kernel<masked>", attn_wide_fwd_kernel<true, false, true>, attn_wide_fwd_kernel<false, true, true>,
                               attn_wide_fwd_kernel<false, false, true>, causal, attn != nullptr, static_cast<const AttnMaskArgs&>(a), stream);
    return attn_launch_fwd("attn_wide_fwd_kernel", ATTN_FWD_FORMS(attn_wide_fwd_kernel), causal, attn != nullptr,
                           static_cast<const AttnArgs&>(a), stream);
}

static int wide_bwd(const char* entry, WideForm form, const float* q, const float* k, const float* v, const float* o, const float* d_o,
                    const float* rowstat, float* delta, float* dq, float* dk, float* dv, const int64_t* key_lens, int B, int H, int Tq,
                    int Tk, int ldq, int ldk, int ldv, int ldo, int lddq, int lddk, int lddv, int causal, float q_scale, float drop_p,
                    uint64_t seed, const uint64_t* step_seed, const WideMask& m, const WideDattn& g, hipStream_t stream) {
    TTTS_REQUIRE(q && k && v && o && d_o && rowstat && delta && dq && dk && dv && key_lens, "%s: null pointer", entry);
    int rc = attn_check(entry, WHD, B, H, Tq, Tk, ldq, ldk, ldv, ldo, causal, drop_p);
    if (!rc) rc = attn_check_grad_strides(entry, WHD, H, lddq, lddk, lddv);
    if (!rc && form == WIDE_DATTN) rc = wide_dattn_check(entry, g, causal, Tq, Tk);
    if (!rc && (form == WIDE_MASKED || (form == WIDE_DATTN && (m.add.p || m.key_dead)))) rc = wide_mask_check(entry, m, Tq, Tk);
    if (rc) return rc;
    TTTS_REQUIRE((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o | (uintptr_t)d_o) & 15) == 0,
                 "%s: q/k/v/o/d_o must be 16-byte aligned", entry);
    AttnDattnArgs a = {};
    attn_fill(a, key_lens, B, H, Tq, Tk, ldq, ldk, ldv, ldo, q_scale, drop_p, seed, step_seed);
    wide_mask_fill(a, m);
    a.q = q; a.k = k; a.v = v; a.o = const_cast<float*>(o); a.dout = d_o; a.rowstat = const_cast<float*>(rowstat);
    a.delta = delta; a.dq = dq; a.dk = dk; a.dv = dv;
    a.lddq = lddq; a.lddk = lddk; a.lddv = lddv;
    if (form == WIDE_DATTN) {
        a.attn_w = g.attn; a.d_attn = g.d.p; a.ld_dattn = (int)g.d.ld;
        a.dattn_stride_b = g.d.stride_b; a.dattn_stride_h = g.d.stride_h;
        const long rows = (long)B * H * Tq;
        TTTS_REQUIRE(rows < (1L << 32), "%s: grid too large (B*H*Tq %ld)", entry, rows);
        hipLaunchKernelGGL(attn_dattn_rowdot_kernel, dim3((unsigned)cdiv(rows, 4L)), dim3(256), 0, stream, g.attn, g.d.p, g.d.stride_b,
                           g.d.stride_h, (int)g.d.ld, delta, H, Tq, Tk, rows);
        TTTS_LAUNCH_CHECK("attn_dattn_rowdot_kernel");
        return attn_launch_bwd_pair<&attn_wide_bwd_dq_kernel<false, true, true>, 0, &attn_wide_bwd_dkv_kernel<false, true, true>, WIDE_DATTN_LDS>(
            entry, "attn_wide_bwd_dq_kernel<dattn>", "attn_wide_bwd_dkv_kernel<dattn>", a, 1, stream);
    }
    if (form == WIDE_MASKED) {
        const AttnMaskArgs& am = a;
        const char* names[2] = {"attn_wide_bwd_dq_kernel<masked>", "attn_wide_bwd_dkv_kernel<masked>"};
        return causal ? attn_launch_bwd_pair<&attn_wide_bwd_dq_kernel<true, true>, 0, &attn_wide_bwd_dkv_kernel<true, true>, 0>(
                            entry, names[0], names[1], am, 1, stream)
                      : attn_launch_bwd_pair<&attn_wide_bwd_dq_kernel<false, true>, 0, &attn_wide_bwd_dkv_kernel<false, true>, 0>(
                            entry, names[0], names[1], am, 1, stream);
    }
    return ATTN_LAUNCH_BWD(attn_wide_bwd_dq_kernel, 0, attn_wide_bwd_dkv_kernel, 0, causal, entry, "attn_wide_bwd_dq_kernel",
                           "attn_wide_bwd_dkv_kernel", static_cast<const AttnArgs&>(a), 1, stream);
}

extern "C" {

int ttts_attention_fwd_wide(const float* q, const float* k, const float* v, float* o, float* rowstat, float* attn,
                            const int64_t* key_lens, int B, int H, int Tq, int Tk, int ldq, int ldk, int ldv, int ldo,
                            int causal, float q_scale, float drop_p, uint64_t seed, const uint64_t* step_seed, void* stream) {
    return wide_fwd("attention_fwd_wide", WIDE_PLAIN, q, k, v, o, rowstat, attn, key_lens, B, H, Tq, Tk, ldq, ldk, ldv, ldo, causal,
                    q_scale, drop_p, seed, step_seed, WideMask{}, (hipStream_t)stream);
}

int ttts_attention_fwd_wide_masked(const float* q, const float* k, const float* v, float* o, float* rowstat, float* attn,
                                   const int64_t* key_lens, int B, int H, int Tq, int Tk, int ldq, int ldk, int ldv, int ldo,
                                   int causal, float q_scale, float drop_p, uint64_t seed, const uint64_t* step_seed,
                                   const float* add_mask, int64_t ldm, int64_t mask_stride_b, int64_t mask_stride_h,
                                   const uint8_t* key_dead, int64_t ldd, void* stream) {
    return wide_fwd("attention_fwd_wide_masked", WIDE_MASKED, q, k, v, o, rowstat, attn, key_lens, B, H, Tq, Tk, ldq, ldk, ldv, ldo,
                    causal, q_scale, drop_p, seed, step_seed, WideMask{{add_mask, ldm, mask_stride_b, mask_stride_h}, key_dead, ldd},
                    (hipStream_t)stream);
}

int ttts_attention_bwd_wide(const float* q, const float* k, const float* v, const float* o, const float* d_o,
                            const float* rowstat, float* delta, float* dq, float* dk, float* dv, const int64_t* key_lens,
                            int B, int H, int Tq, int Tk, int ldq, int ldk, int ldv, int ldo, int lddq, int lddk, int lddv,
                            int causal, float q_scale, float drop_p, uint64_t seed, const uint64_t* step_seed, void* stream) {
    return wide_bwd("attention_bwd_wide", WIDE_PLAIN, q, k, v, o, d_o, rowstat, delta, dq, dk, dv, key_lens, B, H, Tq, Tk, ldq, ldk, ldv,
                    ldo, lddq, lddk, lddv, causal, q_scale, drop_p, seed, step_seed, WideMask{}, WideDattn{}, (hipStream_t)stream);
}

int ttts_attention_bwd_wide_masked(const float* q, const float* k, const float* v, const float* o, const float* d_o,
                                   const float* rowstat, float* delta, float* dq, float* dk, float* dv, const int64_t* key_lens,
                                   int B, int H, int Tq, int Tk, int ldq, int ldk, int ldv, int ldo, int lddq, int lddk, int lddv,
                                   int causal, float q_scale, float drop_p, uint64_t seed, const uint64_t* step_seed,
                                   const float* add_mask, int64_t ldm, int64_t mask_stride_b, int64_t mask_stride_h,
                                   const uint8_t* key_dead, int64_t ldd, void* stream) {
    return wide_bwd("attention_bwd_wide_masked", WIDE_MASKED, q, k, v, o, d_o, rowstat, delta, dq, dk, dv, key_lens, B, H, Tq, Tk, ldq,
                    ldk, ldv, ldo, lddq, lddk, lddv, causal, q_scale, drop_p, seed, step_seed,
                    WideMask{{add_mask, ldm, mask_stride_b, mask_stride_h}, key_dead, ldd}, WideDattn{}, (hipStream_t)stream);
}

int ttts_attention_bwd_wide_dattn(const float* q, const float* k, const float* v, const float* o, const float* d_o,
                                  const float* rowstat, float* delta, float* dq, float* dk, float* dv, const int64_t* key_lens,
                                  int B, int H, int Tq, int Tk, int ldq, int ldk, int ldv, int ldo, int lddq, int lddk, int lddv,
                                  int causal, float q_scale, float drop_p, uint64_t seed, const uint64_t* step_seed,
                                  const float* add_mask, int64_t ldm, int64_t mask_stride_b, int64_t mask_stride_h,
                                  const uint8_t* key_dead, int64_t ldd, const float* attn, const float* d_attn, int64_t ld_dattn,
                                  int64_t dattn_stride_b, int64_t dattn_stride_h, void* stream) {
    return wide_bwd("attention_bwd_wide_dattn", WIDE_DATTN, q, k, v, o, d_o, rowstat, delta, dq, dk, dv, key_lens, B, H, Tq, Tk, ldq,
                    ldk, ldv, ldo, lddq, lddk, lddv, causal, q_scale, drop_p, seed, step_seed,
                    WideMask{{add_mask, ldm, mask_stride_b, mask_stride_h}, key_dead, ldd},
                    WideDattn{attn, {d_attn, ld_dattn, dattn_stride_b, dattn_stride_h}}, (hipStream_t)stream);
}

}  // extern "C"
