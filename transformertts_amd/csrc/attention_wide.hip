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
#include "attention_common.h"

namespace ttts {

constexpr int WHD = 128;          // columns per (padded) head
constexpr int WLD = WHD + 1;      // LDS row stride (odd: conflict-free "row per lane" reads)
constexpr int WKB = 32;           // rows staged per barrier pair (one 32-row MFMA sub-tile)
// two staged 32-row tiles, re-used as per-wave 32x65 scratch in the epilogue (4 waves x 8320 B = 33280 B)
constexpr int WSMEM_FLOATS = 4 * 32 * KT_LD;
static_assert(2 * WKB * WLD <= WSMEM_FLOATS, "staging buffers must fit the shared scratch");

// cooperative staging (256 threads): WKB rows x 128 floats from global into LDS; rows beyond `nrows_total` are zero
template <bool PADDED>
__device__ __forceinline__ void wide_stage_rows(const float* base, long row0, long nrows_total, int ld, int tid, float* dst,
                                                float scale) {
    constexpr int LDD = PADDED ? WLD : WHD;
    const RowSrc src = row_src(base, nrows_total, ld);
    float4 v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = row_load4(src, row0 + (tid >> 5) + 8 * i, tid & 31);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float* d = dst + ((tid >> 5) + 8 * i) * LDD + (tid & 31) * 4;
        if (PADDED) {
            d[0] = v[i].x * scale; d[1] = v[i].y * scale; d[2] = v[i].z * scale; d[3] = v[i].w * scale;
        } else {
            *reinterpret_cast<float4*>(d) = make_float4(v[i].x * scale, v[i].y * scale, v[i].z * scale, v[i].w * scale);
        }
    }
}
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
// write four 32x32 accumulators holding X^T[d][row] (row on the lane) as rows of 128 floats, one 64-column half at a time
__device__ __forceinline__ void wide_store_rows(const f32x16 (&acc)[4], float* scratch, float* gbase, long row0,
                                                long nrows_total, int ld, int lane, float scale) {
    const int l31 = lane & 31, half = lane >> 5;
#pragma unroll
    for (int hb = 0; hb < 2; ++hb) {
#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int r = 0; r < 16; ++r) scratch[l31 * KT_LD + blk * 32 + acc_row(r, half)] = acc[2 * hb + blk][r] * scale;
        wave_lds_sync();
#pragma unroll 4
        for (int i = 0; i < 32; ++i) {
            float v = scratch[i * KT_LD + lane];
            if (row0 + i < nrows_total) gbase[(row0 + i) * ld + hb * 64 + lane] = v;
        }
        wave_lds_sync();
    }
}
__device__ __forceinline__ int wide_klen(const AttnArgs& a, int b) {
    int klen = (int)a.key_lens[b];
    if (klen > a.Tk) klen = a.Tk;
    if (klen < 0) klen = 0;
    return klen;
}

// =====================================================================================  forward
template <bool CAUSAL, bool WRITE_A>
__global__ __launch_bounds__(256, 2) void attn_wide_fwd_kernel(AttnArgs a) {
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

    const int klen = wide_klen(a, b);
    int kend = klen;
    if (CAUSAL && kend > q0 + QB) kend = q0 + QB;
    const int nst_live = (kend + WKB - 1) / WKB;
    const int nst = WRITE_A ? (a.Tk + WKB - 1) / WKB : nst_live;
    int wave_kend = WRITE_A ? a.Tk : kend;
    if (CAUSAL && wave_kend > qw0 + 32) wave_kend = qw0 + 32;

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

    auto alive = [&](int key_g) -> bool { return key_g < klen && (!CAUSAL || key_g <= qg); };
    // registers r .. r+3 of a lane are four neighbouring keys: one hash
    auto drop16 = [&](float (&p)[16], int key0) {
#pragma unroll
        for (int r = 0; r < 16; r += 4) {
            const uint32_t qh = attn_quad_hash(seed_eff, rowid, (uint32_t)(key0 + acc_row(r, half)) >> 2);
#pragma unroll
            for (int e = 0; e < 4; ++e) p[r + e] = attn_keep_word(qh, attn_drop_mult(e), thr16) ? p[r + e] * a.drop_scale : 0.f;
        }
    };
    // online row max / row sum over one masked score tile; -> the factor the running sums shrink by
    auto online = [&](f32x16& s, int key0, float (&p)[16]) -> float {
        float mx = NEG_INF;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[r] = alive(key0 + acc_row(r, half)) ? s[r] : NEG_INF;
            mx = fmaxf(mx, s[r]);
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
        for (int t = 0; t < nst_live; ++t) {
            __syncthreads();
            wide_stage_rows<true>(kb_, (long)t * WKB, a.Tk, a.ldk, tid, Ks, 1.f);
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
    for (int t = 0; t < nst; ++t) {
        __syncthreads();
        wide_stage_rows<true>(kb_, (long)t * WKB, a.Tk, a.ldk, tid, Ks, 1.f);
        wide_stage_rows<false>(vb_, (long)t * WKB, a.Tk, a.ldv, tid, Vs, 1.f);
        __syncthreads();
        const int key0 = t * WKB;
        if (key0 < wave_kend) {      // else: tile entirely above this wave's causal frontier / past the keys
            f32x16 s;
            wide_dot(Ks, l31, half, qreg, s);
            float p[16];
            if (WRITE_A) {
#pragma unroll
                for (int r = 0; r < 16; ++r) p[r] = alive(key0 + acc_row(r, half)) ? __expf(s[r] - m_fin) * inv_l : 0.f;
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
    wide_store_rows(o, scratch, a.o + (long)b * a.Tq * a.ldo + h * WHD, qw0, a.Tq, a.ldo, lane, 1.f);
}

// =====================================================================================  backward: dQ (+ delta)
template <bool CAUSAL>
__global__ __launch_bounds__(256, 1) void attn_wide_bwd_dq_kernel(AttnArgs a) {
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

    const int klen = wide_klen(a, b);
    int kend = klen;
    if (CAUSAL && kend > q0 + QB) kend = q0 + QB;
    const int nst = (kend + WKB - 1) / WKB;
    int wave_kend = kend;
    if (CAUSAL && wave_kend > qw0 + 32) wave_kend = qw0 + 32;

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

    for (int t = 0; t < nst; ++t) {
        __syncthreads();
        wide_stage_rows<true>(kb_, (long)t * WKB, a.Tk, a.ldk, tid, Ks, 1.f);
        wide_stage_rows<true>(vb_, (long)t * WKB, a.Tk, a.ldv, tid, Vs, 1.f);
        __syncthreads();
        const int key0 = t * WKB;
        if (key0 < wave_kend) {
            f32x16 s, dp;
            wide_dot(Ks, l31, half, qreg, s);
            wide_dot(Vs, l31, half, greg, dp);
            float ds[16];
#pragma unroll
            for (int r = 0; r < 16; r += 4) {
                const int key_g = key0 + acc_row(r, half);
                uint32_t qh = 0;
                if (a.thr != 0u) qh = attn_quad_hash(seed_eff, rowid, (uint32_t)key_g >> 2);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int kg = key_g + e;
                    const bool live = kg < klen && (!CAUSAL || kg <= qg);
                    const float p = live ? __expf(s[r + e] - m_q) * inv_l : 0.f;
                    float g = dp[r + e];
                    if (a.thr != 0u) g = attn_keep_word(qh, attn_drop_mult(e), thr16) ? g * a.drop_scale : 0.f;
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
    wide_store_rows(dq, scratch, a.dq + (long)b * a.Tq * a.lddq + h * WHD, qw0, a.Tq, a.lddq, lane, a.qscale);
}

// =====================================================================================  backward: dK, dV
template <bool CAUSAL>
__global__ __launch_bounds__(256, 1) void attn_wide_bwd_dkv_kernel(AttnArgs a) {
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

    const int klen = wide_klen(a, b);

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
    int qs_begin = CAUSAL ? (k0 / WKB) : 0;       // queries below the block's first key never see it
    if (k0 >= klen) qs_begin = nqs;               // whole key block is padding: gradients are zero

    for (int qs = qs_begin; qs < nqs; ++qs) {
        __syncthreads();
        wide_stage_rows<true>(qb_, (long)qs * WKB, a.Tq, a.ldq, tid, Qs, a.qscale);
        wide_stage_rows<true>(gb_, (long)qs * WKB, a.Tq, a.ldo, tid, Gs, 1.f);
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
            wide_dot(Gs, l31, half, vreg, dp);
            float pd[16], ds[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qrow = acc_row(r, half);
                const int q_g = qt0 + qrow;
                const bool live = kg < klen && (!CAUSAL || kg <= q_g) && q_g < a.Tq;
                const float p = live ? __expf(s[r] - m_s[qrow]) * il_s[qrow] : 0.f;
                float g = dp[r];
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
    wide_store_rows(dk, scratch, a.dk + (long)b * a.Tk * a.lddk + h * WHD, kw0, a.Tk, a.lddk, lane, 1.f);
    wide_store_rows(dv, scratch, a.dv + (long)b * a.Tk * a.lddv + h * WHD, kw0, a.Tk, a.lddv, lane, 1.f);
}

// arguments both entry points share; every refusal names the value it refuses
static int wide_check(const char* name, int B, int H, int Tq, int Tk, int ldq, int ldk, int ldv, int ldo, int causal,
                      float drop_p) {
    TTTS_REQUIRE(B > 0 && H > 0 && Tq > 0 && Tk > 0, "%s: sizes must be positive (B %d, H %d, Tq %d, Tk %d)", name, B, H, Tq, Tk);
    TTTS_REQUIRE((long)B * H < (1L << 31) && cdiv(Tq, QB) <= 65535 && cdiv(Tk, QB) <= 65535,
                 "%s: grid too large (B*H %ld, Tq %d, Tk %d)", name, (long)B * H, Tq, Tk);
    TTTS_REQUIRE(ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0 && ldo % 4 == 0,
                 "%s: row strides must be multiples of 4 floats (ldq %d, ldk %d, ldv %d, ldo %d)", name, ldq, ldk, ldv, ldo);
    TTTS_REQUIRE(ldq >= H * WHD && ldk >= H * WHD && ldv >= H * WHD && ldo >= H * WHD,
                 "%s: row strides must be >= H*128 = %d (ldq %d, ldk %d, ldv %d, ldo %d)", name, H * WHD, ldq, ldk, ldv, ldo);
    TTTS_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "%s: dropout p %g is outside [0, 1)", name, (double)drop_p);
    TTTS_REQUIRE(!causal || Tq == Tk, "%s: the causal form needs Tq == Tk (Tq %d, Tk %d)", name, Tq, Tk);
    return TTTS_OK;
}

}  // namespace ttts

using namespace ttts;

extern "C" {

int ttts_attention_fwd_wide(const float* q, const float* k, const float* v, float* o, float* rowstat, float* attn,
                            const int64_t* key_lens, int B, int H, int Tq, int Tk, int ldq, int ldk, int ldv, int ldo,
                            int causal, float q_scale, float drop_p, uint64_t seed, const uint64_t* step_seed, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    TTTS_REQUIRE(q && k && v && o && rowstat && key_lens, "attention_fwd_wide: null pointer");
    int rc = wide_check("attention_fwd_wide", B, H, Tq, Tk, ldq, ldk, ldv, ldo, causal, drop_p);
    if (rc) return rc;
    TTTS_REQUIRE(!(causal && attn), "attention_fwd_wide: the weights are only written by the non-causal (cross) form");
    TTTS_REQUIRE((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) & 15) == 0, "attention_fwd_wide: q/k/v must be 16-byte aligned");
    AttnArgs a = {};
    a.q = q; a.k = k; a.v = v; a.o = o; a.rowstat = rowstat; a.attn = attn; a.key_lens = key_lens;
    a.B = B; a.H = H; a.Tq = Tq; a.Tk = Tk; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo;
    a.thr = drop_p > 0.f ? drop_threshold(drop_p) : 0u;
    a.drop_scale = 1.f / (1.f - drop_p);
    a.qscale = q_scale;
    a.seed = seed; a.step_seed = step_seed;
    dim3 grid(B * H, cdiv(Tq, QB), 1);
    if (causal)
        hipLaunchKernelGGL((attn_wide_fwd_kernel<true, false>), grid, dim3(256), 0, stream, a);
    else if (attn)
        hipLaunchKernelGGL((attn_wide_fwd_kernel<false, true>), grid, dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL((attn_wide_fwd_kernel<false, false>), grid, dim3(256), 0, stream, a);
    TTTS_LAUNCH_CHECK("attn_wide_fwd_kernel");
    return TTTS_OK;
}

int ttts_attention_bwd_wide(const float* q, const float* k, const float* v, const float* o, const float* d_o,
                            const float* rowstat, float* delta, float* dq, float* dk, float* dv, const int64_t* key_lens,
                            int B, int H, int Tq, int Tk, int ldq, int ldk, int ldv, int ldo, int lddq, int lddk, int lddv,
                            int causal, float q_scale, float drop_p, uint64_t seed, const uint64_t* step_seed, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    TTTS_REQUIRE(q && k && v && o && d_o && rowstat && delta && dq && dk && dv && key_lens, "attention_bwd_wide: null pointer");
    int rc = wide_check("attention_bwd_wide", B, H, Tq, Tk, ldq, ldk, ldv, ldo, causal, drop_p);
    if (rc) return rc;
    TTTS_REQUIRE(lddq >= H * WHD && lddk >= H * WHD && lddv >= H * WHD,
                 "attention_bwd_wide: gradient strides must be >= H*128 = %d (lddq %d, lddk %d, lddv %d)", H * WHD, lddq, lddk, lddv);
    TTTS_REQUIRE((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o | (uintptr_t)d_o) & 15) == 0,
                 "attention_bwd_wide: q/k/v/o/d_o must be 16-byte aligned");
    AttnArgs a = {};
    a.q = q; a.k = k; a.v = v; a.o = const_cast<float*>(o); a.dout = d_o; a.rowstat = const_cast<float*>(rowstat);
    a.delta = delta; a.dq = dq; a.dk = dk; a.dv = dv; a.key_lens = key_lens;
    a.B = B; a.H = H; a.Tq = Tq; a.Tk = Tk; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo;
    a.lddq = lddq; a.lddk = lddk; a.lddv = lddv;
    a.thr = drop_p > 0.f ? drop_threshold(drop_p) : 0u;
    a.drop_scale = 1.f / (1.f - drop_p);
    a.qscale = q_scale;
    a.seed = seed; a.step_seed = step_seed;
    dim3 gq(B * H, cdiv(Tq, QB), 1), gk(B * H, cdiv(Tk, QB), 1);
    if (causal) {
        hipLaunchKernelGGL((attn_wide_bwd_dq_kernel<true>), gq, dim3(256), 0, stream, a);
        TTTS_LAUNCH_CHECK("attn_wide_bwd_dq_kernel");
        hipLaunchKernelGGL((attn_wide_bwd_dkv_kernel<true>), gk, dim3(256), 0, stream, a);
    } else {
        hipLaunchKernelGGL((attn_wide_bwd_dq_kernel<false>), gq, dim3(256), 0, stream, a);
        TTTS_LAUNCH_CHECK("attn_wide_bwd_dq_kernel");
        hipLaunchKernelGGL((attn_wide_bwd_dkv_kernel<false>), gk, dim3(256), 0, stream, a);
    }
    TTTS_LAUNCH_CHECK("attn_wide_bwd_dkv_kernel");
    return TTTS_OK;
}

}  // extern "C"
