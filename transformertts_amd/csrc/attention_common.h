// Pieces shared by the three attention translation units (attention.hip: fp32 operands, 64 columns; attention_img.hip: head-image
// operands; attention_wide.hip: fp32 operands, 128 columns).  Besides the row loads and the split / MFMA helpers this header holds
// the FRAME every kernel family states the same way -- the clamped key count, the key range of a query block, the masks, the
// dropout of a lane's 16 weights, the row staging and stores -- and the host side's argument check, argument fill and launch
// ladders.  What differs in arithmetic between families (score and gradient products, exponent forms, row statistics, operand
// staging of the split forms, launch bounds) stays in the family's file.
// How the kernels reach the helpers follows what hipcc makes of them (tools/isa_diff.py against the copies they replace,
// profiles/attn_frame_isa.txt: registers and every non-scalar opcode count unchanged).  A helper called directly is inlined
// before the kernel body is simplified, a lambda after, and the same arithmetic can then cost two to nine more registers:
//  * attn_drop16: through a one-line `drop16` lambda in every forward that has one (attn_fwd_img_maps_kernel keeps its loop);
//  * attn_alive: called directly in attention_wide.hip and in the backward kernels; through a one-line `alive` lambda in the
//    three forwards of attention.hip; NOT used by attn_fwd_img_kernel, the image dQ kernel and the bf16x6 / fp16x3 dK/dV
//    kernels, which keep the predicate written out;
//  * the online row-maximum / row-sum update and the weight write-out stay written out in each forward.
#pragma once
#include "ttts_common.h"

namespace ttts {

constexpr int HD = 64;            // head dim
constexpr int KT_LD = HD + 1;     // LDS row stride (odd: conflict-free "row per lane" reads)
constexpr int WHD = 128;          // columns per (padded) head of the 128-column kernels
constexpr int WLD = WHD + 1;      // ... and their LDS row stride
constexpr int QB = 128;           // rows per workgroup (4 waves x 32)
constexpr float NEG_INF = -__builtin_inff();
// v_exp_f32 as it is: exp2f() wraps it in a range reduction for results below 2^-126 (compare, select, add, ldexp: four more
// instructions per element in kernels whose speed is set by their VALU count); such weights are zero at fp32 anyway
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
typedef unsigned int u32x4v __attribute__((ext_vector_type(4)));

// Row loads go through a raw buffer descriptor spanning `nrows` rows of the (batch, head) slice: a row index past the
// end gives an offset outside the descriptor and the hardware returns zeros.  A predicated global load ("if (row <
// nrows) v = *p") instead compiles to branch + load + s_waitcnt vmcnt(0) and serialises the loads of a stage.
struct RowSrc {
    __amdgpu_buffer_rsrc_t rsrc;
    int ld;
};
__device__ __forceinline__ RowSrc row_src(const float* base, long nrows, int ld) {
    RowSrc r;
    r.rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, (uint32_t)(nrows * ld * 4), 0x00020000);
    r.ld = ld;
    return r;
}
__device__ __forceinline__ float4 row_load4(const RowSrc& s, long row, int c4) {
    const u32x4v v = __builtin_amdgcn_raw_buffer_load_b128(s.rsrc, (int)(uint32_t)((row * s.ld + c4 * 4) * 4), 0, 0);
    return make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
}

struct AttnArgs {
    const float* q; const float* k; const float* v;
    float* o; float* lse; float* attn;
    const float* dout; float* delta; float* dq; float* dk; float* dv;
    const int64_t* key_lens;
    int B, H, Tq, Tk;
    int ldq, ldk, ldv, ldo, lddq, lddk, lddv;
    float qscale;                             // q is multiplied by this before q.k^T: sqrt(1 / head_dim) (torch/nn/functional.py:6578)
    float drop_scale; uint32_t thr; uint64_t seed; const uint64_t* step_seed;
    const float* do_amax; int do_amax_n;      // fp16x3 backward: partial maxima of |dout| (ttts_amax_partials)
    float* amax_dq; float* amax_dkv;          // fp16x3 backward: NULL, or caller-zeroed TTTS_AMAX_SLOTS-slot arrays receiving max|dq| / max|dk, dv|
    // fp16x3 forms: TTTS_AMAX_SLOTS partial maxima of |q|, |k|, |v| each (the same array three times for a packed projection output):
    // the operands' dynamic pre-scales.  o_amax (forward): NULL, or a caller-zeroed TTTS_AMAX_SLOTS-slot array receiving max|o|.
    const float* q_amax; const float* k_amax; const float* v_amax;
    float* o_amax;
    // fp16x3 forms: per-row softmax statistics in the forward's own units, (2, B, H, Tq): plane 0 = the subtrahend mcs of the
    // weights' exponents fma(s, c2, -mcs) exactly as the forward used it with the final row maximum (one rounded product
    // per row), plane 1 = log2 of the row sum of those weights.  The backward re-forms bit-identical score accumulators s and
    // the same exponents, so its probabilities ARE the forward's whatever the scores' magnitude; from lse (one float,
    // natural units) they are only good to ulp(lse): 6 % at scores of 1e6.
    float* rowstat;
};


constexpr int KB = 64;   // rows staged per barrier pair (two 32-row MFMA sub-tiles)

// one wave stages its own 32 x 64 tile (rows beyond nrows_total -> 0) into `dst` (stride KT_LD)
__device__ __forceinline__ void wave_stage_tile(const float* base, long row0, long nrows_total, int ld, int lane,
                                                float* dst, float scale) {
    const RowSrc src = row_src(base, nrows_total, ld);
    float4 v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int row = (lane >> 4) + 4 * i, c4 = lane & 15;
        v[i] = row_load4(src, row0 + row, c4);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int row = (lane >> 4) + 4 * i, c4 = lane & 15;
        float* d = dst + row * KT_LD + c4 * 4;
        d[0] = v[i].x * scale; d[1] = v[i].y * scale; d[2] = v[i].z * scale; d[3] = v[i].w * scale;
    }
}
__device__ __forceinline__ void wave_lds_sync() {
    // LDS traffic of one wave: make the writes above visible to the reads below (same wave)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// write NB (32x32) accumulators holding X^T[d][row] (row on the lane) as rows of 32 NB floats, one 64-column half at a time
template <int NB>
__device__ __forceinline__ void wave_store_rows(const f32x16 (&acc)[NB], float* scratch, float* gbase, long row0,
                                                long nrows_total, int ld, int lane, float scale) {
    const int l31 = lane & 31, half = lane >> 5;
#pragma unroll
    for (int hb = 0; hb < NB / 2; ++hb) {
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

// LDS budget shared by the three kernels: two staged 64-row tiles, re-used as per-wave 32x65 scratch in the
// prologue / epilogue (4 waves x 8320 B = 33280 B)
constexpr int SMEM_FLOATS = 4 * 32 * KT_LD;
static_assert(2 * KB * KT_LD <= SMEM_FLOATS, "staging buffers must fit the shared scratch");
constexpr int WKB = 32;  // 128-column kernels: rows staged per barrier pair (one 32-row MFMA sub-tile); same budget
constexpr int WSMEM_FLOATS = SMEM_FLOATS;
static_assert(2 * WKB * WLD <= WSMEM_FLOATS, "staging buffers must fit the shared scratch");

// ---- cooperative staging (256 threads): rows of W floats (W / 4 threads per row, four passes: 64 rows of 64 columns, 32 rows of
// 128) from global straight into LDS; rows beyond `nrows_total` are zero.  No register prefetch across the compute phase: with
// 3-4 workgroups per CU the other workgroups cover the load latency, and the registers are worth more as occupancy.
template <int W, bool PADDED>
__device__ __forceinline__ void stage_rows(const float* base, long row0, long nrows_total, int ld, int tid, float* dst,
                                           float scale) {
    constexpr int TPR = W / 4, RPP = 256 / TPR, LDD = PADDED ? W + 1 : W;     // threads per row, rows per pass
    const RowSrc src = row_src(base, nrows_total, ld);
    float4 v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = row_load4(src, row0 + (tid / TPR + RPP * i), tid % TPR);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float* d = dst + (tid / TPR + RPP * i) * LDD + (tid % TPR) * 4;
        if (PADDED) {
            d[0] = v[i].x * scale; d[1] = v[i].y * scale; d[2] = v[i].z * scale; d[3] = v[i].w * scale;
        } else {
            *reinterpret_cast<float4*>(d) = make_float4(v[i].x * scale, v[i].y * scale, v[i].z * scale, v[i].w * scale);
        }
    }
}

// ---- the frame: key counts, key ranges, masks
__device__ __forceinline__ int attn_klen(const int64_t* key_lens, int b, int Tk) {
    int klen = (int)key_lens[b];
    if (klen > Tk) klen = Tk;
    if (klen < 0) klen = 0;
    return klen;
}
// the key stages (of ROWS keys) a block of QB queries starting at q0 walks, and where the wave whose queries start at qw0 stops:
// `kend` = end of the live keys (causal frontier of the block included), `nst_live` = stages that hold one, `nst` = stages of the
// main pass (every key when the weights are written: the padding's zeros are part of the map), `wave_kend` = first key no
// 32-key sub-tile of this wave needs.  The backward dQ kernels use the WRITE_A = false form.
struct KeyRange { int kend, nst_live, nst, wave_kend; };
template <bool CAUSAL, bool WRITE_A, int ROWS>
__device__ __forceinline__ KeyRange key_range(int klen, int Tk, int q0, int qw0) {
    KeyRange r;
    r.kend = klen;
    if (CAUSAL && r.kend > q0 + QB) r.kend = q0 + QB;
    r.nst_live = (r.kend + ROWS - 1) / ROWS;
    r.nst = WRITE_A ? (Tk + ROWS - 1) / ROWS : r.nst_live;
    r.wave_kend = WRITE_A ? Tk : r.kend;
    if (CAUSAL && r.wave_kend > qw0 + 32) r.wave_kend = qw0 + 32;
    return r;
}
// dK / dV kernels: the first of the `nqs` query stages (of ROWS queries) the key block starting at k0 meets
template <bool CAUSAL, int ROWS>
__device__ __forceinline__ int attn_qs_begin(int k0, int klen, int nqs) {
    int qs_begin = CAUSAL ? (k0 / ROWS) : 0;      // queries below the block's first key never see it
    if (k0 >= klen) qs_begin = nqs;               // whole key block is padding: gradients are zero
    return qs_begin;
}
template <bool CAUSAL>
__device__ __forceinline__ bool attn_alive(int key, int klen, int q) { return key < klen && (!CAUSAL || key <= q); }

// ---- masks that arrive as tensors (the MASKED forms of the 128-column kernels): an additive fp32 mask per (batch, head) slice
// (row stride ldm floats, a multiple of 4; batch / head strides in elements, 0 = broadcast) and a (B, ldd) byte mask of dead keys;
// either may be NULL.  A mask element at or below MASK_FORBID (half the lowest finite float: what -inf and torch's
// finfo.min fill both satisfy; a NaN fails the comparison and forbids too) forbids the key, any other value is added to the
// scaled score.
struct AttnMaskArgs : AttnArgs {
    const float* add_mask; const uint8_t* key_dead;
    long mask_stride_b, mask_stride_h;
    int ldm, ldd;
};
constexpr float MASK_FORBID = -1.7014117e38f;      // 0.5 * -FLT_MAX
template <bool CAUSAL>
__device__ __forceinline__ bool attn_alive_masked(int key, int klen, int q, bool dead, float add) {
    return attn_alive<CAUSAL>(key, klen, q) && !dead && add > MASK_FORBID;
}
// the (Tq, ldm) mask slice of (b, h) behind a buffer descriptor: rows past Tq and a NULL mask (an empty descriptor) read as
// zeros -- "add nothing, forbid nothing" --, so no mask load sits behind a branch
__device__ __forceinline__ RowSrc mask_src(const AttnMaskArgs& a, int b, int h) {
    const float* base = a.add_mask ? a.add_mask + b * a.mask_stride_b + h * a.mask_stride_h : nullptr;
    return row_src(base, a.add_mask ? a.Tq : 0, a.ldm);
}
// query on the lane (forward, dQ): the lane's four aligned key quads of the 32-key tile at key0 -- registers 4 i .. 4 i + 3 --
// as four 16-byte loads of its mask row
__device__ __forceinline__ void mask_load_row16(const RowSrc& src, long q, int key0, int half, float (&mk)[16]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float4 v = row_load4(src, q, (key0 >> 2) + 2 * i + half);
        mk[4 * i] = v.x; mk[4 * i + 1] = v.y; mk[4 * i + 2] = v.z; mk[4 * i + 3] = v.w;
    }
}
// key on the lane (dK / dV): the 16 queries of the lane's accumulator rows, one dword each, coalesced across the 32 key lanes
__device__ __forceinline__ void mask_load_col16(const RowSrc& src, int q0, int key, int half, float (&mk)[16]) {
#pragma unroll
    for (int r = 0; r < 16; ++r)
        mk[r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
            src.rsrc, (int)(uint32_t)(((long)(q0 + acc_row(r, half)) * src.ld + key) * 4), 0, 0));
}
// the dead-key bytes of utterance b behind a descriptor of Tk bytes (NULL: empty, nothing dead); one byte per lane
__device__ __forceinline__ __amdgpu_buffer_rsrc_t dead_src(const AttnMaskArgs& a, int b) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(a.key_dead ? a.key_dead + (long)b * a.ldd : nullptr), 0,
                                             a.key_dead ? (uint32_t)a.Tk : 0u, 0x00020000);
}
__device__ __forceinline__ bool dead_load(__amdgpu_buffer_rsrc_t rsrc, int key) {
    return __builtin_amdgcn_raw_buffer_load_b8(rsrc, key, 0, 0) != 0;
}
// ... and of a 32-key tile as one wave-uniform word (bit j = key0 + j is dead), shifted so that bit acc_row(r, 0) is the
// lane's register r
__device__ __forceinline__ uint32_t dead_tile_bits(__amdgpu_buffer_rsrc_t rsrc, int key0, int l31, int half) {
    return (uint32_t)__ballot(dead_load(rsrc, key0 + l31)) >> (4 * half);
}

// ---- a gradient of the written weights (the DATTN forms of the 128-column backward kernels): fp32, addressed like the additive
// mask -- element (b, h, q, key) at d_attn[b*dattn_stride_b + h*dattn_stride_h + q*ld_dattn + key], strides in elements, 0 =
// broadcast, ld_dattn a multiple of 4 floats, every slice 16-byte aligned -- and read with the mask's loads (mask_load_row16 /
// mask_load_col16) through a descriptor over the slice's Tq rows.  What is read for a key that is not alive (columns past Tk,
// the neighbouring row) is never used: the kernels select on the key's liveness.  `attn`: the forward's own (B,H,Tq,Tk) weights.
struct AttnDattnArgs : AttnMaskArgs {
    const float* attn_w; const float* d_attn;
    long dattn_stride_b, dattn_stride_h;
    int ld_dattn;
};
__device__ __forceinline__ RowSrc dattn_src(const AttnDattnArgs& a, int b, int h) {
    return row_src(a.d_attn + b * a.dattn_stride_b + h * a.dattn_stride_h, a.Tq, a.ld_dattn);
}

// ---- dropout of a lane's weights: registers r .. r+3 of a lane are four neighbouring keys and share one hash word `qh` (of
// the quad of `key`); SCALE: the kept ones are multiplied by 1/(1-p) here (else that factor rides in a later scale)
template <bool SCALE>
__device__ __forceinline__ float attn_drop1(float x, uint32_t qh, int e, uint32_t thr16, float drop_scale) {
    return attn_keep_word(qh, attn_drop_mult(e), thr16) ? (SCALE ? x * drop_scale : x) : 0.f;
}
template <bool SCALE>
__device__ __forceinline__ void attn_drop16(float (&p)[16], uint64_t seed_eff, uint32_t rowid, int key0, int half, uint32_t thr16,
                                            float drop_scale) {
#pragma unroll
    for (int r = 0; r < 16; r += 4) {
        const uint32_t qh = attn_quad_hash(seed_eff, rowid, (uint32_t)(key0 + acc_row(r, half)) >> 2);
#pragma unroll
        for (int e = 0; e < 4; ++e) p[r + e] = attn_drop1<SCALE>(p[r + e], qh, e, thr16, drop_scale);
    }
}


typedef _Float16 f16x8v __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2v __attribute__((ext_vector_type(2)));
constexpr float H3A_P = 1024.0f;

__device__ __forceinline__ void split2_pair_h(f32x2 x, uint32_t& hi, uint32_t& lo) {
    const f16x2v h = __builtin_convertvector(x, f16x2v);
    const f32x2 r = x - __builtin_convertvector(h, f32x2);          // exact
    hi = __builtin_bit_cast(uint32_t, h);
    lo = __builtin_bit_cast(uint32_t, __builtin_convertvector(r, f16x2v));
}

// 8 fp32 -> two f16x8 fragments of x * scale
__device__ __forceinline__ void split_frag8_h3(const float (&x)[8], float scale, f16x8v& hi, f16x8v& lo) {
    u32x4v h, l;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        uint32_t a, b;
        split2_pair_h(f32x2{x[2 * u], x[2 * u + 1]} * scale, a, b);
        h[u] = a; l[u] = b;
    }
    hi = __builtin_bit_cast(f16x8v, h);
    lo = __builtin_bit_cast(f16x8v, l);
}
// c += a (hi,lo) x b (hi,lo), three products, smallest terms first
__device__ __forceinline__ void mfma_h3(f32x16& c, const f16x8v (&a)[2], const f16x8v (&b)[2]) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[1], b[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0], b[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0], b[0], c, 0, 0, 0);
}


// ds: this lane's 16 dS values of the tile (true units); sds: the lane's current pre-scale (0 = unset); acc: the
// accumulator pair the products land in (lane-local column).  Both half-waves hold halves of the same column.
__device__ __forceinline__ void attn_h3_track_scale(const float (&ds)[16], float& sds, f32x16 (&acc)[2]) {
    float m = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) m = fmaxf(m, fabsf(ds[r]));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    const uint32_t e = (__float_as_uint(m) >> 23) & 0xffu;
    const bool change = e >= 24u && e < 255u && (sds == 0.f || m * sds > 8192.f);
    if (__any(change)) {
        const float snew = change ? __uint_as_float((265u - e) << 23) : sds;
        const float f = (change && sds != 0.f) ? snew / sds : 1.f;        // a power of two <= 2^-1 when it applies
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[0][r] *= f; acc[1][r] *= f; }
        sds = snew;
    }
}

// lane-resident B operand: the 64 values of this lane's row (query or key) x scale, split in two, for the four 16-deep steps
__device__ __forceinline__ void load_lane_frags_h3(const float* scratch, int l31, int half, float scale, f16x8v (&f)[4][2]) {
#pragma unroll
    for (int st = 0; st < 4; ++st) {
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = scratch[l31 * KT_LD + 16 * st + 8 * half + e];
        split_frag8_h3(x, scale, f[st][0], f[st][1]);
    }
}

// ---- host side: one argument check, one argument fill, one launch ladder per direction
// the arguments every entry point shares (`width` = columns per head); every refusal names the value it refuses
static inline int attn_check(const char* name, int width, int B, int H, int Tq, int Tk, int ldq, int ldk, int ldv, int ldo,
                             int causal, float drop_p) {
    TTTS_REQUIRE(B > 0 && H > 0 && Tq > 0 && Tk > 0, "%s: sizes must be positive (B %d, H %d, Tq %d, Tk %d)", name, B, H, Tq, Tk);
    TTTS_REQUIRE((long)B * H < (1L << 31) && cdiv(Tq, QB) <= 65535 && cdiv(Tk, QB) <= 65535,
                 "%s: grid too large (B*H %ld, Tq %d, Tk %d)", name, (long)B * H, Tq, Tk);
    TTTS_REQUIRE(ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0 && ldo % 4 == 0,
                 "%s: row strides must be multiples of 4 floats (ldq %d, ldk %d, ldv %d, ldo %d)", name, ldq, ldk, ldv, ldo);
    TTTS_REQUIRE(ldq >= H * width && ldk >= H * width && ldv >= H * width && ldo >= H * width,
                 "%s: row strides must be >= H*%d = %d (ldq %d, ldk %d, ldv %d, ldo %d)", name, width, H * width, ldq, ldk, ldv, ldo);
    TTTS_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "%s: dropout p %g is outside [0, 1)", name, (double)drop_p);
    TTTS_REQUIRE(!causal || Tq == Tk, "%s: the causal form needs Tq == Tk (Tq %d, Tk %d)", name, Tq, Tk);
    return TTTS_OK;
}
static inline int attn_check_grad_strides(const char* name, int width, int H, int lddq, int lddk, int lddv) {
    TTTS_REQUIRE(lddq >= H * width && lddk >= H * width && lddv >= H * width,
                 "%s: gradient strides must be >= H*%d = %d (lddq %d, lddk %d, lddv %d)", name, width, H * width, lddq, lddk, lddv);
    return TTTS_OK;
}
// the fields AttnArgs and AttnImgArgs have in common
template <class Args>
static inline void attn_fill(Args& a, const int64_t* key_lens, int B, int H, int Tq, int Tk, int ldq, int ldk, int ldv, int ldo,
                             float q_scale, float drop_p, uint64_t seed, const uint64_t* step_seed) {
    a.key_lens = key_lens;
    a.B = B; a.H = H; a.Tq = Tq; a.Tk = Tk; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo;
    a.thr = drop_p > 0.f ? drop_threshold(drop_p) : 0u;
    a.drop_scale = 1.f / (1.f - drop_p);
    a.qscale = q_scale;
    a.seed = seed; a.step_seed = step_seed;
}
// forward: K<CAUSAL, WRITE_A> as <true, false> (causal), <false, true> (weights written) or <false, false>
#define ATTN_FWD_FORMS(K) K<true, false>, K<false, true>, K<false, false>
template <class Args>
static inline int attn_launch_fwd(const char* name, void (*causal_k)(Args), void (*weights_k)(Args), void (*plain_k)(Args),
                                  int causal, bool weights, const Args& a, hipStream_t stream) {
    hipLaunchKernelGGL(causal ? causal_k : weights ? weights_k : plain_k, dim3(a.B * a.H, cdiv(a.Tq, QB), 1), dim3(256), 0, stream, a);
    TTTS_LAUNCH_CHECK(name);
    return TTTS_OK;
}
// backward: the dQ kernel, then the dK / dV kernel (key blocks x `gk_z`); a dynamic LDS size is registered once per kernel
template <auto DQ_K, int DQ_LDS, auto DKV_K, int DKV_LDS, class Args>
static inline int attn_launch_bwd_pair(const char* entry, const char* dq_name, const char* dkv_name, const Args& a, int gk_z,
                                       hipStream_t stream) {
    if constexpr (DQ_LDS > 0 || DKV_LDS > 0) {
        static bool configured = false;   // (more than 64 KB of LDS per workgroup needs this explicit opt-in)
        if (!configured) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(DQ_K), hipFuncAttributeMaxDynamicSharedMemorySize, DQ_LDS);
            if (e == hipSuccess)
                e = hipFuncSetAttribute(reinterpret_cast<const void*>(DKV_K), hipFuncAttributeMaxDynamicSharedMemorySize, DKV_LDS);
            if (e != hipSuccess) {
                set_error("%s: cannot reserve %d bytes of LDS: %s", entry, DQ_LDS > DKV_LDS ? DQ_LDS : DKV_LDS, hipGetErrorString(e));
                return TTTS_ERR_LAUNCH;
            }
            configured = true;
        }
    }
    hipLaunchKernelGGL(DQ_K, dim3(a.B * a.H, cdiv(a.Tq, QB), 1), dim3(256), DQ_LDS, stream, a);
    TTTS_LAUNCH_CHECK(dq_name);
    hipLaunchKernelGGL(DKV_K, dim3(a.B * a.H, cdiv(a.Tk, QB), gk_z), dim3(256), DKV_LDS, stream, a);
    TTTS_LAUNCH_CHECK(dkv_name);
    return TTTS_OK;
}
#define ATTN_LAUNCH_BWD(DQ_K, DQ_LDS, DKV_K, DKV_LDS, causal, ...)                                       \
    ((causal) ? attn_launch_bwd_pair<&DQ_K<true>, DQ_LDS, &DKV_K<true>, DKV_LDS>(__VA_ARGS__)          \
              : attn_launch_bwd_pair<&DQ_K<false>, DQ_LDS, &DKV_K<false>, DKV_LDS>(__VA_ARGS__))

}  // namespace ttts
