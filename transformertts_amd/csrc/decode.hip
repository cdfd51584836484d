// Autoregressive decoding (TransformerTTS.inference with K/V caches): the kernels of ONE frame, for M = B rows.
// At these row counts every GEMM is a weight-streaming GEMV: plain fp32 FMA chains, weights loaded straight to VGPRs with
// 16-byte loads before anything else (their latency overlaps the state read), no MFMA, no partial maxima, no pre-scales.
// Everything that changes from frame to frame or from call to call (frame index t, max_len, stop threshold, the stop frame)
// is read from the caller's ttts_decode_state when the kernel runs, so one captured HIP graph of a chunk of frames serves
// every frame and every call; every kernel returns at once when t >= t_end or a stop frame has been recorded.
// Summation orders are fixed (per lane in index order, then the wave butterfly, then waves / key blocks in index order) and
// depend on neither M, B nor the buffer capacities: a synthesized call is bitwise reproducible.  No atomics.
// The *_rows entry points add per-row state: row_end[b] > 0 says utterance b ended at that frame, and every per-row unit of
// work (an attention workgroup, a combine or LayerNorm wave, a GEMV row's loads and stores) returns before its first global
// load of that row; the rows still running compute exactly what they compute with no row ended.
#include "ttts_common.h"

namespace ttts {
namespace {

constexpr int DEC_ROWS = 4;       // rows of one decode-linear workgroup (grid.y covers M)
constexpr int DEC_KMAX = 4096;    // widest K (16 float4 per lane)
constexpr int ATTN_KEYS = 64;     // keys per attention workgroup (16 per wave, four lanes per key)
constexpr int LN_PER = 16;        // decode LayerNorm: d <= 64 * LN_PER

__device__ __forceinline__ bool decode_done(const ttts_decode_state* st, int64_t& t) {
    t = st->t;
    const int64_t t_end = st->t_end, stop_frame = st->stop_frame;      // one scalar read of the block, not two dependent ones
    return (t >= t_end) | (stop_frame >= 0);
}

// row_end == NULL (the entry points without per-row state): no row ever ends.  The load is unconditional (a field of the state
// stands in for a missing array) and every kernel issues it together with the state read, before the branch on either: the
// per-row state then costs no memory round trip of its own.
__device__ __forceinline__ bool row_ended(const int64_t* row_end, const ttts_decode_state* st, int m) {
    const int64_t* p = row_end != nullptr ? row_end + m : &st->stop_frame;
    const int64_t v = *p;
    return (row_end != nullptr) & (v > 0);
}

__device__ __forceinline__ float dot4(float4 a, float4 b, float acc) {
    acc = fmaf(a.x, b.x, acc);
    acc = fmaf(a.y, b.y, acc);
    acc = fmaf(a.z, b.z, acc);
    return fmaf(a.w, b.w, acc);
}

struct DecLinArgs {
    const float* x;          // row m at x + m * ldx + (t - 1) * x_ts
    long ldx, x_ts;
    const float* w;          // (N, K) state-dict layout, 16-byte aligned
    const float* bias;       // (N) or NULL
    const float* res;        // residual row m at res + m * ldr, or NULL
    long ldr;
    const float* pe;         // NULL, or y += alpha[0] * pe[(t - 1) * N + n] after the activation (positional encoding)
    const float* alpha;
    float* y;                // columns n < n_split: y + m * ldy + (t - 1) * y_ts + n
    long ldy, y_ts;
    float* y2;               // columns n >= n_split: y2 + m * ldy2 + (t - 1) * y2_ts + (n - n_split)
    long ldy2, y2_ts;
    int n_split, M, N, K, act;
    const ttts_decode_state* st;
    const int64_t* row_end;  // NULL, or (M rounded up to a multiple of 4): rows with row_end[m] > 0 are neither read nor written
};

// y[M,N] = act(x . w^T + b) (+ res) (+ alpha pe[t-1]).  Wave = NC output columns; lane l holds the float4 chunks l, l+64, ...
// of each column's weight row (KC of them); one workgroup = 4 waves x DEC_ROWS rows, its activation rows loaded up front.
// Ended rows (row_end) cost the workgroup nothing but the weight stream it shares with its other rows.
template <int KC, int NC>
__global__ __launch_bounds__(256) void decode_linear_kernel(const DecLinArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n0 = (blockIdx.x * 4 + wave) * NC;
    if (n0 >= a.N) return;
    const int K4 = a.K >> 2;
    float4 w[NC][KC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const float4* wr = reinterpret_cast<const float4*>(a.w + (long)min(n0 + c, a.N - 1) * a.K);
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            const int k4 = lane + 64 * j;
            w[c][j] = k4 < K4 ? wr[k4] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    const int m0 = blockIdx.y * DEC_ROWS;
    // the four rows' end frames in ONE scalar read issued with the state read (row_end is readable up to a multiple of four
    // entries; without it the 32-byte state block stands in and is ignored)
    const bool has_rows = a.row_end != nullptr;
    const int64_t* rp = has_rows ? a.row_end + m0 : reinterpret_cast<const int64_t*>(a.st);
    const int64_t re[DEC_ROWS] = {rp[0], rp[1], rp[2], rp[3]};
    int64_t t;
    const bool done = decode_done(a.st, t);
    bool ended[DEC_ROWS];
    bool all_ended = true;
#pragma unroll
    for (int r = 0; r < DEC_ROWS; ++r) {
        ended[r] = has_rows & (re[r] > 0);
        all_ended = all_ended & (ended[r] | (m0 + r >= a.M));
    }
    if (done | all_ended) return;             // (uniform over the workgroup)
    const long tr = (long)(t - 1);
    // the workgroup's rows: every activation load is issued before the first product (one L2 round trip, not one per row)
    float4 xv[DEC_ROWS][KC];
#pragma unroll
    for (int r = 0; r < DEC_ROWS; ++r) {
        const int m = min(m0 + r, a.M - 1);
        const float4* xr = reinterpret_cast<const float4*>(a.x + (long)m * a.ldx + tr * a.x_ts);
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            const int k4 = lane + 64 * j;
            xv[r][j] = (k4 < K4 && !ended[r]) ? xr[k4] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
#pragma unroll
    for (int r = 0; r < DEC_ROWS; ++r) {
        const int m = m0 + r;
        if (m >= a.M) break;
        float acc[NC];                        // (an ended row's products run on zeros: cheaper than a branch around them)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < KC; ++j) s = dot4(xv[r][j], w[c][j], s);
            acc[c] = wave_sum(s);
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int n = n0 + c;
            if (lane != c || n >= a.N || ended[r]) continue;
            float v = acc[c];
            if (a.bias != nullptr) v += a.bias[n];
            if (a.act == TTTS_ACT_RELU) v = fmaxf(v, 0.f);
            if (a.res != nullptr) v += a.res[(long)m * a.ldr + n];
            if (a.pe != nullptr) v += a.alpha[0] * a.pe[tr * a.N + n];
            if (n < a.n_split) a.y[(long)m * a.ldy + tr * a.y_ts + n] = v;
            else a.y2[(long)m * a.ldy2 + tr * a.y2_ts + (n - a.n_split)] = v;
        }
    }
}

template <int KC, int NC>
void launch_decode_linear_t(const DecLinArgs& a, hipStream_t stream) {
    const dim3 grid(cdiv(a.N, 4 * NC), cdiv(a.M, DEC_ROWS));
    hipLaunchKernelGGL((decode_linear_kernel<KC, NC>), grid, dim3(256), 0, stream, a);
}

template <int NC>
void launch_decode_linear_nc(const DecLinArgs& a, hipStream_t stream) {
    const int kc = cdiv(a.K, 256);
    if (kc <= 1) launch_decode_linear_t<1, NC>(a, stream);
    else if (kc <= 2) launch_decode_linear_t<2, NC>(a, stream);
    else if (kc <= 4) launch_decode_linear_t<4, NC>(a, stream);
    else if (kc <= 8) launch_decode_linear_t<8, (NC < 2 ? NC : 2)>(a, stream);
    else launch_decode_linear_t<16, 1>(a, stream);
}

// Four columns per wave once there are enough rows for the activation re-reads to matter; one column per wave (the most
// workgroups) below that.
int launch_decode_linear(const DecLinArgs& a, hipStream_t stream) {
    if (a.M >= 8) launch_decode_linear_nc<4>(a, stream);
    else launch_decode_linear_nc<1>(a, stream);
    TTTS_LAUNCH_CHECK("decode_linear");
    return TTTS_OK;
}

int check_decode_linear(const DecLinArgs& a, const char* what) {
    TTTS_REQUIRE(a.x && a.w && a.y && a.st, "%s: null pointer", what);
    TTTS_REQUIRE(a.M >= 1 && a.N >= 1 && a.K >= 4 && a.K % 4 == 0 && a.K <= DEC_KMAX,
                 "%s: bad sizes M=%d N=%d K=%d (M, N >= 1; 4 <= K <= %d, K %% 4 == 0)", what, a.M, a.N, a.K, DEC_KMAX);
    TTTS_REQUIRE((long)a.M <= 65535L * DEC_ROWS, "%s: M=%d too large", what, a.M);
    TTTS_REQUIRE(a.n_split >= 0 && a.n_split <= a.N, "%s: n_split=%d outside [0, N=%d]", what, a.n_split, a.N);
    TTTS_REQUIRE(a.n_split == a.N || a.y2 != nullptr, "%s: null pointer (y2 with n_split < N)", what);
    TTTS_REQUIRE(a.act == TTTS_ACT_NONE || a.act == TTTS_ACT_RELU, "%s: act=%d (NONE or RELU)", what, a.act);
    TTTS_REQUIRE(((uintptr_t)a.x & 15) == 0 && ((uintptr_t)a.w & 15) == 0 && a.ldx % 4 == 0 && a.x_ts % 4 == 0,
                 "%s: x and w must be 16-byte aligned, ldx and x_ts multiples of 4", what);
    TTTS_REQUIRE(a.ldx >= a.K || a.M == 1, "%s: ldx=%ld < K=%d", what, a.ldx, a.K);
    TTTS_REQUIRE(a.ldx >= 0 && a.x_ts >= 0 && a.ldr >= 0 && a.ldy >= 0 && a.y_ts >= 0 && a.ldy2 >= 0 && a.y2_ts >= 0,
                 "%s: negative stride", what);
    return TTTS_OK;
}

// ---------------------------------------------------------------- stop head + end of frame
// One workgroup: wave w takes rows 4w .. 4w+3, 4w+16 .. 4w+19, ...; stop[m, t-1] = x[m] . w + b; then the frame is an
// all-stop frame when every row has 1 / (1 + expf(-stop)) >= threshold (torch.sigmoid(stop) >= thr away from exact ties);
// thread 0 records it and advances t.
// With row_end: ended rows are neither read nor written.  Under TTTS_DECODE_PER_ROW (st->flags) a row that reaches the
// threshold has row_end[m] = t latched (its first crossing: it is skipped from then on), and the frame that leaves no row
// running is the stop frame; without the flag the decision is the all-rows-at-this-frame one above, over the running rows.
template <int KC>
__global__ __launch_bounds__(256) void decode_stop_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ b, float* __restrict__ stop, long ld_stop,
                                                          int M, int K, int64_t* row_end, ttts_decode_state* st) {
    __shared__ int all_rows[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K4 = K >> 2;
    const float4* w4 = reinterpret_cast<const float4*>(w);
    float4 wv[KC];
#pragma unroll
    for (int j = 0; j < KC; ++j) {
        const int k4 = lane + 64 * j;
        wv[j] = k4 < K4 ? w4[k4] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // the wave's first four rows: one scalar read issued with the state read, as in decode_linear_kernel
    const bool has_rows = row_end != nullptr;
    const int64_t* rp = (has_rows && wave * 4 < M) ? row_end + wave * 4 : reinterpret_cast<const int64_t*>(st);
    const int64_t first[4] = {rp[0], rp[1], rp[2], rp[3]};
    int64_t t;
    if (decode_done(st, t)) return;           // (uniform over the workgroup)
    const float thr = st->stop_threshold;
    const bool per_row = row_end != nullptr && (st->flags & TTTS_DECODE_PER_ROW) != 0;
    const float bias = b != nullptr ? b[0] : 0.f;
    int ok = 1;
    for (int mb = wave * 4; mb < M; mb += 16) {            // four rows per wave at a time, their loads issued together
        bool ended[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) ended[r] = has_rows & (((mb == wave * 4 || !has_rows) ? first[r] : row_end[mb + r]) > 0);
        float4 xv[4][KC];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float4* xr = reinterpret_cast<const float4*>(x + (long)min(mb + r, M - 1) * K);
#pragma unroll
            for (int j = 0; j < KC; ++j) {
                const int k4 = lane + 64 * j;
                xv[r][j] = (k4 < K4 && !ended[r]) ? xr[k4] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = mb + r;
            if (m >= M) break;
            if (ended[r]) continue;
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < KC; ++j) s = dot4(xv[r][j], wv[j], s);
            const float v = wave_sum(s) + bias;
            if (lane == 0) stop[(long)m * ld_stop + (t - 1)] = v;
            const float p = 1.0f / (1.0f + expf(-v));
            const bool cross = p >= thr;
            if (per_row && cross && lane == 0) row_end[m] = t;
            ok &= cross ? 1 : 0;
        }
    }
    if (lane == 0) all_rows[wave] = ok;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int all = all_rows[0] & all_rows[1] & all_rows[2] & all_rows[3];
        if (all) st->stop_frame = t;
        st->t = t + 1;
    }
}

// ---------------------------------------------------------------- LayerNorm of the decoder rows
__global__ __launch_bounds__(256) void decode_layernorm_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float* __restrict__ y, int M, int d,
                                                               float eps, const int64_t* __restrict__ row_end,
                                                               const ttts_decode_state* st) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wave;
    if (row >= M) return;
    const bool ended = row_ended(row_end, st, row);
    int64_t t;
    if (decode_done(st, t) | ended) return;   // (uniform over the wave)
    const float* xr = x + (long)row * d;
    float v[LN_PER];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < LN_PER; ++i) {
        v[i] = 0.f;
        if (lane + 64 * i < d) { v[i] = xr[lane + 64 * i]; s += v[i]; }
    }
    const float mean = wave_sum(s) / (float)d;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < LN_PER; ++i) {
        if (lane + 64 * i < d) { const float c = v[i] - mean; q = fmaf(c, c, q); }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)d + eps);
    float* yr = y + (long)row * d;
#pragma unroll
    for (int i = 0; i < LN_PER; ++i) {
        const int c = lane + 64 * i;
        if (c < d) yr[c] = (v[i] - mean) * rstd * gamma[c] + beta[c];
    }
}

// ---------------------------------------------------------------- attention, one query row per (utterance, head)
// Workgroup (s, h, b) takes keys [64 s, 64 s + 64): wave w keys 16 w .. 16 w + 15, four lanes per key, each lane a contiguous
// quarter of the head (HD / 16 float4).  Keys at or past the length are never loaded.  Partial (o[HD], max, sum) per block
// goes to the workspace; the combine kernel adds the blocks below the length in block order.
// MAPS: the unnormalised weight exp(s - m_block) of every key below the length also goes to row t - 1 of the (b, h) plane of
// the attention map; the combine rescales that row with the factors it forms for the context vector.
struct AttnMap {
    float* p;                // (B, H, rows, ld_row) floats: plane (b, h) at p + (b * H + h) * ld_head, NULL without MAPS
    long ld_head, ld_row;
    int rows;                // frames the planes hold: row t - 1 is written when t - 1 < rows
};

// WIN (ttts_decode_attention_window): this layer's ttts_decode_window and the per-utterance positions.  A constrained head
// (bit h of head_mask) sees keys [max(0, c - back), min(len - 1, c + ahead)] only, c = pos[b, t - 2] (0 at t = 1): the window
// struct is read with the state and row_end; the centre's address needs t, so it is read behind the state, with lens[b].  A block
// that does not meet the window returns before any K/V load, keys outside it are not loaded and score -inf like the keys past
// the length.  The guide head's blocks also store the index of their first maximum key (workspace slot HD + 2).
template <bool WIN>
struct AttnWin {};
template <>
struct AttnWin<true> {
    const ttts_decode_window* win;
    int32_t* pos;            // (B, ld_pos): frame t reads pos[b, t - 2], the guide head's combine writes pos[b, t - 1]
    long ld_pos;
};

// The centre of frame t: pos[b, t - 2], 0 at t = 1.  The load is unconditional (entry 0 stands in at t = 1 and is not used) and
// every head issues it, next to the length: the one read that needs t then shares its round trip with lens[b].
__device__ __forceinline__ long window_centre(const int32_t* pos, long ld_pos, int b, int64_t t) {
    const int32_t v = pos[(long)b * ld_pos + (long)(t >= 2 ? t - 2 : 0)];
    return t >= 2 ? (long)v : 0;
}

// keys [lo, hi] a constrained head sees around centre c (len >= 1): c is clamped into the keys, so the window is never empty
__device__ __forceinline__ void window_range(const ttts_decode_window& wn, long c, long len, long& lo, long& hi) {
    c = c < 0 ? 0 : (c > len - 1 ? len - 1 : c);
    lo = c - (long)wn.back;
    lo = lo < 0 ? 0 : lo;
    hi = c + (long)wn.ahead;
    hi = hi > len - 1 ? len - 1 : hi;
}

template <int HD, bool MAPS, bool WIN = false>
__global__ __launch_bounds__(256) void decode_attn_partial_kernel(const float* __restrict__ q, long ldq, const float* __restrict__ k,
                                                                  const float* __restrict__ v, long ld_row, long ld_batch,
                                                                  const int64_t* __restrict__ lens, float* __restrict__ ws, int H,
                                                                  int nsplit, int max_keys, float scale,
                                                                  const int64_t* __restrict__ row_end, const AttnMap map,
                                                                  const ttts_decode_state* st, const AttnWin<WIN> w) {
    constexpr int CH = HD / 16;               // float4 per lane
    constexpr int WS = HD + 4;                // workspace floats per block
    __shared__ float red_m[4], red_l[4];
    __shared__ float4 red_o[4][HD / 4];
    __shared__ int red_i[4];                  // (WIN: first maximum key of each wave)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const bool ended = row_ended(row_end, st, b);
    ttts_decode_window wn;
    bool no_window = false;                   // a struct with a negative reach: the launch does nothing.  Being part of the first
    if constexpr (WIN) {                      // branch is also what puts the struct's read into the scalar batch of the state
        wn = *w.win;
        no_window = (wn.back | wn.ahead) < 0;
    }
    int64_t t;
    if (decode_done(st, t) | ended | no_window) return;   // (uniform over the workgroup)
    long len, centre = 0;
    if constexpr (WIN) {                      // (lens is required: the length and the centre are one scalar batch)
        len = (long)lens[b];
        centre = window_centre(w.pos, w.ld_pos, b, t);
    } else {
        len = lens != nullptr ? (long)lens[b] : (long)t;
    }
    len = len < (long)max_keys ? len : (long)max_keys;
    const int key0 = s * ATTN_KEYS;
    if constexpr (!WIN) {
        if (key0 >= len) return;              // (uniform over the workgroup)
    }
    const int key = key0 + wave * 16 + (lane >> 2), sub = lane & 3;
    bool live = key < len;
    bool guide = false;
    if constexpr (WIN) {
        long lo, hi;                          // (selects, not a branch around the centre: its load stays next to the length's)
        window_range(wn, centre, len, lo, hi);
        const bool con = ((wn.head_mask >> h) & 1) & (len > 0);
        lo = con ? lo : 0;
        hi = con ? hi : len - 1;
        if ((key0 >= len) | ((long)key0 > hi) | ((long)key0 + ATTN_KEYS - 1 < lo)) return;   // (uniform over the workgroup)
        guide = h == wn.guide_head;
        live = live && (long)key >= lo && (long)key <= hi;
    }
    const long col = (long)h * HD + sub * (HD / 4);
    const float4* q4 = reinterpret_cast<const float4*>(q + (long)b * ldq + col);
    float4 kv[CH], vv[CH];
    const long kro = (long)b * ld_batch + (long)key * ld_row + col;
#pragma unroll
    for (int j = 0; j < CH; ++j) {
        kv[j] = live ? reinterpret_cast<const float4*>(k + kro)[j] : make_float4(0.f, 0.f, 0.f, 0.f);
        vv[j] = live ? reinterpret_cast<const float4*>(v + kro)[j] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float sc = 0.f;
#pragma unroll
    for (int j = 0; j < CH; ++j) {
        float4 qq = q4[j];
        qq.x *= scale; qq.y *= scale; qq.z *= scale; qq.w *= scale;
        sc = dot4(qq, kv[j], sc);
    }
    sc += __shfl_xor(sc, 1, 64);
    sc += __shfl_xor(sc, 2, 64);
    sc = live ? sc : -INFINITY;
    const float wm = wave_max(sc);
    if (lane == 0) red_m[wave] = wm;
    if constexpr (WIN) {
        if (guide) {                          // lowest live key that holds the wave's maximum (a butterfly of minima: fixed order)
            int cand = (live && sc == wm) ? key : 0x7fffffff;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const int other = __shfl_xor(cand, off, 64);
                cand = other < cand ? other : cand;
            }
            if (lane == 0) red_i[wave] = cand;
        }
    }
    __syncthreads();
    const float mb = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));   // finite: key0 < len
    const float p = live ? expf(sc - mb) : 0.f;
    if (MAPS) {
        if (live && sub == 0 && t - 1 < (int64_t)map.rows)
            map.p[((long)b * H + h) * map.ld_head + (long)(t - 1) * map.ld_row + key] = p;
    }
    const float wl = wave_sum(sub == 0 ? p : 0.f);
    float4 o[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) {
        float4 a = make_float4(p * vv[j].x, p * vv[j].y, p * vv[j].z, p * vv[j].w);
#pragma unroll
        for (int off = 4; off < 64; off <<= 1) {
            a.x += __shfl_xor(a.x, off, 64);
            a.y += __shfl_xor(a.y, off, 64);
            a.z += __shfl_xor(a.z, off, 64);
            a.w += __shfl_xor(a.w, off, 64);
        }
        o[j] = a;
    }
    if (lane < 4) {
#pragma unroll
        for (int j = 0; j < CH; ++j) red_o[wave][sub * CH + j] = o[j];
    }
    if (lane == 0) red_l[wave] = wl;
    __syncthreads();
    float* out = ws + (((long)b * H + h) * nsplit + s) * WS;
    if (threadIdx.x < HD / 4) {
        const int i = threadIdx.x;
        float4 r = red_o[0][i];
#pragma unroll
        for (int w2 = 1; w2 < 4; ++w2) {
            r.x += red_o[w2][i].x; r.y += red_o[w2][i].y; r.z += red_o[w2][i].z; r.w += red_o[w2][i].w;
        }
        reinterpret_cast<float4*>(out)[i] = r;
    }
    if (threadIdx.x == 0) {
        out[HD] = mb;
        out[HD + 1] = ((red_l[0] + red_l[1]) + red_l[2]) + red_l[3];
        if constexpr (WIN) {
            if (guide) {                      // the waves hold ascending keys: the first wave at the block maximum wins a tie
                const int idx = red_m[0] == mb ? red_i[0] : red_m[1] == mb ? red_i[1] : red_m[2] == mb ? red_i[2] : red_i[3];
                out[HD + 2] = __int_as_float(idx);
            }
        }
    }
}

// one wave per (head, utterance): out = sum_s o_s e^(m_s - m) / sum_s l_s e^(m_s - m) over the blocks below the length
// MAPS: map row t - 1, key j of block s = (its unnormalised weight * e^(m_s - m)) / l below the length, 0 from there to max_keys
// WIN: a constrained head walks the blocks that meet its window only (the others hold stale workspace); the guide head writes
// pos[b, t - 1] = the first maximum key of the lowest block at the largest block maximum; MAPS zeroes every key outside the window
template <int HD, bool MAPS, bool WIN = false>
__global__ __launch_bounds__(64) void decode_attn_combine_kernel(const float* __restrict__ ws, const int64_t* __restrict__ lens,
                                                                 float* __restrict__ out, long ldo, int H, int nsplit, int max_keys,
                                                                 const int64_t* __restrict__ row_end, const AttnMap map,
                                                                 const ttts_decode_state* st, const AttnWin<WIN> w) {
    constexpr int WS = HD + 4;
    const int lane = threadIdx.x, h = blockIdx.x, b = blockIdx.y;
    const bool ended = row_ended(row_end, st, b);
    ttts_decode_window wn;
    bool no_window = false;                   // (as in the partial kernel)
    if constexpr (WIN) {
        wn = *w.win;
        no_window = (wn.back | wn.ahead) < 0;
    }
    int64_t t;
    if (decode_done(st, t) | ended | no_window) return;   // (uniform over the wave)
    long len, centre = 0;
    if constexpr (WIN) {                      // (as in the partial kernel)
        len = (long)lens[b];
        centre = window_centre(w.pos, w.ld_pos, b, t);
    } else {
        len = lens != nullptr ? (long)lens[b] : (long)t;
    }
    len = len < (long)max_keys ? len : (long)max_keys;
    const int nblk = len > 0 ? (int)((len + ATTN_KEYS - 1) / ATTN_KEYS) : 0;
    const float* p = ws + ((long)b * H + h) * nsplit * WS;
    int s_lo = 0, s_end = nblk;               // the blocks [s_lo, s_end) that hold this frame's partials
    long lo = 0, hi = len - 1;                // the keys that carry weight
    if constexpr (WIN) {                      // (selects, as in the partial kernel)
        long wlo, whi;
        window_range(wn, centre, len, wlo, whi);
        const bool con = ((wn.head_mask >> h) & 1) & (len > 0);
        lo = con ? wlo : lo;
        hi = con ? whi : hi;
        s_lo = con ? (int)(wlo / ATTN_KEYS) : s_lo;
        s_end = con ? (int)(whi / ATTN_KEYS) + 1 : s_end;
    }
    float m = -INFINITY;
    for (int s = s_lo; s < s_end; ++s) m = fmaxf(m, p[s * WS + HD]);
    if constexpr (WIN) {
        if (h == wn.guide_head && lane == 0) {
            int idx = 0;
            for (int s = s_end - 1; s >= s_lo; --s)       // (descending: the lowest block at the maximum is the last one kept)
                if (p[s * WS + HD] == m) idx = __float_as_int(p[s * WS + HD + 2]);
            w.pos[(long)b * w.ld_pos + (long)(t - 1)] = idx;
        }
    }
    float l = 0.f, o0 = 0.f, o1 = 0.f;
    for (int s = s_lo; s < s_end; ++s) {
        const float e = expf(p[s * WS + HD] - m);
        l = fmaf(p[s * WS + HD + 1], e, l);
        if (lane < HD) o0 = fmaf(p[s * WS + lane], e, o0);
        if (lane + 64 < HD) o1 = fmaf(p[s * WS + lane + 64], e, o1);
    }
    const float inv = s_end > s_lo ? 1.0f / l : 0.f;
    float* orow = out + (long)b * ldo + (long)h * HD;
    if (lane < HD) orow[lane] = o0 * inv;
    if (lane + 64 < HD) orow[lane + 64] = o1 * inv;
    if (MAPS) {
        if (t - 1 >= (int64_t)map.rows) return;
        float* mrow = map.p + ((long)b * H + h) * map.ld_head + (long)(t - 1) * map.ld_row;
        for (int s = 0; s < nsplit; ++s) {
            const int key = s * ATTN_KEYS + lane;
            if (key >= max_keys) break;
            float a = 0.f;
            if (s >= s_lo && s < s_end && (long)key >= lo && (long)key <= hi) a = (mrow[key] * expf(p[s * WS + HD] - m)) * inv;
            mrow[key] = a;
        }
    }
}

int attn_nsplit(int max_keys) { return cdiv(max_keys, ATTN_KEYS); }

struct AttnArgs {
    const float *q, *k, *v;
    long ldq, ld_row, ld_batch;
    const int64_t* lens;
    float* out;
    long ldo;
    float* ws;
    int B, H, max_keys;
    const int64_t* row_end;
    AttnMap map;
    const ttts_decode_state* st;
    const ttts_decode_window* win;   // ttts_decode_attention_window only: NULL selects the kernels without window code
    int32_t* pos;
    long ld_pos;
};

template <int HD, bool MAPS, bool WIN>
void launch_decode_attention_tm(const AttnArgs& a, hipStream_t stream) {
    const int ns = attn_nsplit(a.max_keys);
    const float scale = 1.0f / sqrtf((float)HD);
    AttnWin<WIN> w;
    if constexpr (WIN) w = AttnWin<true>{a.win, a.pos, a.ld_pos};
    hipLaunchKernelGGL((decode_attn_partial_kernel<HD, MAPS, WIN>), dim3(ns, a.H, a.B), dim3(256), 0, stream, a.q, a.ldq, a.k, a.v,
                       a.ld_row, a.ld_batch, a.lens, a.ws, a.H, ns, a.max_keys, scale, a.row_end, a.map, a.st, w);
    hipLaunchKernelGGL((decode_attn_combine_kernel<HD, MAPS, WIN>), dim3(a.H, a.B), dim3(64), 0, stream, a.ws, a.lens, a.out, a.ldo,
                       a.H, ns, a.max_keys, a.row_end, a.map, a.st, w);
}

template <int HD>
void launch_decode_attention_t(const AttnArgs& a, hipStream_t stream) {
    if (a.win != nullptr) {
        if (a.map.p != nullptr) launch_decode_attention_tm<HD, true, true>(a, stream);
        else launch_decode_attention_tm<HD, false, true>(a, stream);
    } else if (a.map.p != nullptr) {
        launch_decode_attention_tm<HD, true, false>(a, stream);
    } else {
        launch_decode_attention_tm<HD, false, false>(a, stream);
    }
}

int check_decode_attention(const AttnArgs& a, int head_dim, size_t ws_bytes, const char* what) {
    TTTS_REQUIRE(a.q && a.k && a.v && a.out && a.ws && a.st, "%s: null pointer", what);
    TTTS_REQUIRE(a.B >= 1 && a.H >= 1 && a.B <= 65535 && a.H <= 65535 && a.max_keys >= 1, "%s: bad sizes B=%d H=%d max_keys=%d",
                 what, a.B, a.H, a.max_keys);
    TTTS_REQUIRE(head_dim >= 16 && head_dim <= 128 && head_dim % 16 == 0, "%s: head_dim=%d (a multiple of 16 up to 128)", what,
                 head_dim);
    TTTS_REQUIRE(a.ldq % 4 == 0 && a.ld_row % 4 == 0 && a.ld_batch % 4 == 0 && a.ldq >= (long)a.H * head_dim &&
                 a.ld_row >= (long)a.H * head_dim && a.ld_batch >= 0 && a.ldo >= (long)a.H * head_dim,
                 "%s: strides ldq=%ld ld_row=%ld ld_batch=%ld ldo=%ld (multiples of 4, >= H * head_dim)", what, a.ldq, a.ld_row,
                 a.ld_batch, a.ldo);
    TTTS_REQUIRE((((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.ws) & 15) == 0,
                 "%s: q, k, v and ws must be 16-byte aligned", what);
    TTTS_REQUIRE(ws_bytes >= ttts_decode_attention_workspace_bytes(a.B, a.H, head_dim, a.max_keys),
                 "%s: workspace of %zu bytes < %zu", what, ws_bytes,
                 ttts_decode_attention_workspace_bytes(a.B, a.H, head_dim, a.max_keys));
    return TTTS_OK;
}

int launch_decode_attention(const AttnArgs& a, int head_dim, hipStream_t s, const char* what) {
    switch (head_dim) {
        case 16: launch_decode_attention_t<16>(a, s); break;
        case 32: launch_decode_attention_t<32>(a, s); break;
        case 48: launch_decode_attention_t<48>(a, s); break;
        case 64: launch_decode_attention_t<64>(a, s); break;
        case 80: launch_decode_attention_t<80>(a, s); break;
        case 96: launch_decode_attention_t<96>(a, s); break;
        case 112: launch_decode_attention_t<112>(a, s); break;
        default: launch_decode_attention_t<128>(a, s); break;
    }
    TTTS_LAUNCH_CHECK(what);
    return TTTS_OK;
}

// ---------------------------------------------------------------- rows at or past a length := 0
// x is (outer, T, C); slice o keeps rows < lens[o / group].  Workgroup (c, o) strides over the tail of slice o, 16-byte
// stores when C and the slice offset allow it (VEC), single floats otherwise.
template <bool VEC>
__global__ __launch_bounds__(256) void mask_rows_kernel(float* __restrict__ x, const int64_t* __restrict__ lens, int group, long T,
                                                        long C) {
    const long o = blockIdx.y;
    long len = (long)lens[o / group];
    len = len < 0 ? 0 : (len > T ? T : len);
    float* base = x + o * T * C;
    const long first = len * C, total = T * C;
    const long step = (long)gridDim.x * blockDim.x;
    if (VEC) {
        float4* b4 = reinterpret_cast<float4*>(base);
        for (long i = (first >> 2) + (long)blockIdx.x * blockDim.x + threadIdx.x; i < (total >> 2); i += step)
            b4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        for (long i = first + (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) base[i] = 0.f;
    }
}

}  // namespace
}  // namespace ttts

using namespace ttts;

extern "C" {

// the stop kernel of the frame-out entry points
static int launch_decode_stop(const float* x, const float* w_stop, const float* b_stop, float* stop, long ld_stop, int B, int d,
                              int64_t* row_end, ttts_decode_state* st, hipStream_t s) {
    const int kc = cdiv(d, 256);
    if (kc <= 1) hipLaunchKernelGGL(decode_stop_kernel<1>, dim3(1), dim3(256), 0, s, x, w_stop, b_stop, stop, ld_stop, B, d, row_end, st);
    else if (kc <= 2) hipLaunchKernelGGL(decode_stop_kernel<2>, dim3(1), dim3(256), 0, s, x, w_stop, b_stop, stop, ld_stop, B, d, row_end, st);
    else if (kc <= 4) hipLaunchKernelGGL(decode_stop_kernel<4>, dim3(1), dim3(256), 0, s, x, w_stop, b_stop, stop, ld_stop, B, d, row_end, st);
    else if (kc <= 8) hipLaunchKernelGGL(decode_stop_kernel<8>, dim3(1), dim3(256), 0, s, x, w_stop, b_stop, stop, ld_stop, B, d, row_end, st);
    else hipLaunchKernelGGL(decode_stop_kernel<16>, dim3(1), dim3(256), 0, s, x, w_stop, b_stop, stop, ld_stop, B, d, row_end, st);
    return TTTS_OK;
}

static int decode_linear_impl(const char* what, const float* x, int64_t ldx, int64_t x_tstride, const float* w, const float* bias,
                              const float* residual, int64_t ldr, float* y, int64_t ldy, int64_t y_tstride, float* y2, int64_t ldy2,
                              int64_t y2_tstride, int n_split, int M, int N, int K, int act, const int64_t* row_end,
                              const ttts_decode_state* st, void* stream) {
    DecLinArgs a{x, (long)ldx, (long)x_tstride, w, bias, residual, (long)ldr, nullptr, nullptr, y, (long)ldy, (long)y_tstride,
                 y2, (long)ldy2, (long)y2_tstride, n_split, M, N, K, act, st, row_end};
    TTTS_REQUIRE(residual == nullptr || ldr >= N || M == 1, "%s: ldr=%ld < N=%d", what, (long)ldr, N);
    const int rc = check_decode_linear(a, what);
    if (rc != TTTS_OK) return rc;
    return launch_decode_linear(a, (hipStream_t)stream);
}

static int decode_frame_in_impl(const char* what, const float* ys, int64_t ld_ys, int n_mels, const float* w1, const float* b1,
                                const float* w2, const float* b2, const float* pe, const float* alpha, float* tmp, float* out, int B,
                                int d, const int64_t* row_end, const ttts_decode_state* st, void* stream) {
    TTTS_REQUIRE(ys && w1 && w2 && pe && alpha && tmp && out && st, "%s: null pointer", what);
    TTTS_REQUIRE(B >= 1 && d >= 4 && d % 4 == 0 && n_mels >= 4 && n_mels % 4 == 0 && ld_ys >= n_mels,
                 "%s: bad sizes B=%d d=%d n_mels=%d ld_ys=%ld (d, n_mels multiples of 4)", what, B, d, n_mels, (long)ld_ys);
    TTTS_REQUIRE(((uintptr_t)tmp & 15) == 0, "%s: tmp must be 16-byte aligned", what);
    DecLinArgs l1{ys, (long)ld_ys, (long)n_mels, w1, b1, nullptr, 0, nullptr, nullptr, tmp, (long)d, 0, nullptr, 0, 0, d, B, d,
                  n_mels, TTTS_ACT_RELU, st, row_end};
    DecLinArgs l2{tmp, (long)d, 0, w2, b2, nullptr, 0, pe, alpha, out, (long)d, 0, nullptr, 0, 0, d, B, d, d, TTTS_ACT_RELU, st,
                  row_end};
    char name[96];
    snprintf(name, sizeof name, "%s (pre-net linear1)", what);
    int rc = check_decode_linear(l1, name);
    snprintf(name, sizeof name, "%s (pre-net linear2)", what);
    if (rc == TTTS_OK) rc = check_decode_linear(l2, name);
    if (rc != TTTS_OK) return rc;
    rc = launch_decode_linear(l1, (hipStream_t)stream);
    if (rc != TTTS_OK) return rc;
    return launch_decode_linear(l2, (hipStream_t)stream);
}

static int decode_frame_out_impl(const char* what, const float* x, const float* w_mel, const float* b_mel, const float* w_stop,
                                 const float* b_stop, float* ys, int64_t ld_ys, float* stop, int64_t ld_stop, int B, int d,
                                 int n_mels, int64_t* row_end, ttts_decode_state* st, void* stream) {
    TTTS_REQUIRE(x && w_mel && w_stop && ys && stop && st, "%s: null pointer", what);
    TTTS_REQUIRE(B >= 1 && d >= 4 && d % 4 == 0 && d <= DEC_KMAX && n_mels >= 1 && ld_ys >= n_mels && ld_stop >= 1,
                 "%s: bad sizes B=%d d=%d n_mels=%d ld_ys=%ld ld_stop=%ld", what, B, d, n_mels, (long)ld_ys, (long)ld_stop);
    TTTS_REQUIRE(((uintptr_t)w_stop & 15) == 0, "%s: w_stop must be 16-byte aligned", what);
    // frame t of ys: row (t - 1) + 1
    DecLinArgs mel{x, (long)d, 0, w_mel, b_mel, nullptr, 0, nullptr, nullptr, ys + n_mels, (long)ld_ys, (long)n_mels, nullptr, 0, 0,
                   n_mels, B, n_mels, d, TTTS_ACT_NONE, st, row_end};
    char name[96];
    snprintf(name, sizeof name, "%s (mel head)", what);
    int rc = check_decode_linear(mel, name);
    if (rc != TTTS_OK) return rc;
    rc = launch_decode_linear(mel, (hipStream_t)stream);
    if (rc != TTTS_OK) return rc;
    launch_decode_stop(x, w_stop, b_stop, stop, (long)ld_stop, B, d, row_end, st, (hipStream_t)stream);
    TTTS_LAUNCH_CHECK(what);
    return TTTS_OK;
}

static int decode_layernorm_impl(const char* what, const float* x, const float* gamma, const float* beta, float* y, int M, int d,
                                 float eps, const int64_t* row_end, const ttts_decode_state* st, void* stream) {
    TTTS_REQUIRE(x && gamma && beta && y && st, "%s: null pointer", what);
    TTTS_REQUIRE(M >= 1 && d >= 1 && d <= 64 * LN_PER && M <= 4 * 65535, "%s: bad sizes M=%d d=%d (d <= %d)", what, M, d,
                 64 * LN_PER);
    hipLaunchKernelGGL(decode_layernorm_kernel, dim3(cdiv(M, 4)), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, y, M, d, eps,
                       row_end, st);
    TTTS_LAUNCH_CHECK(what);
    return TTTS_OK;
}

int ttts_decode_linear(const float* x, int64_t ldx, int64_t x_tstride, const float* w, const float* bias, const float* residual,
                       int64_t ldr, float* y, int64_t ldy, int64_t y_tstride, float* y2, int64_t ldy2, int64_t y2_tstride,
                       int n_split, int M, int N, int K, int act, const ttts_decode_state* st, void* stream) {
    return decode_linear_impl("decode_linear", x, ldx, x_tstride, w, bias, residual, ldr, y, ldy, y_tstride, y2, ldy2, y2_tstride,
                              n_split, M, N, K, act, nullptr, st, stream);
}

int ttts_decode_linear_rows(const float* x, int64_t ldx, int64_t x_tstride, const float* w, const float* bias,
                            const float* residual, int64_t ldr, float* y, int64_t ldy, int64_t y_tstride, float* y2, int64_t ldy2,
                            int64_t y2_tstride, int n_split, int M, int N, int K, int act, const int64_t* row_end,
                            const ttts_decode_state* st, void* stream) {
    TTTS_REQUIRE(row_end, "decode_linear_rows: null pointer (row_end)");
    return decode_linear_impl("decode_linear_rows", x, ldx, x_tstride, w, bias, residual, ldr, y, ldy, y_tstride, y2, ldy2,
                              y2_tstride, n_split, M, N, K, act, row_end, st, stream);
}

int ttts_decode_frame_in(const float* ys, int64_t ld_ys, int n_mels, const float* w1, const float* b1, const float* w2,
                         const float* b2, const float* pe, const float* alpha, float* tmp, float* out, int B, int d,
                         const ttts_decode_state* st, void* stream) {
    return decode_frame_in_impl("decode_frame_in", ys, ld_ys, n_mels, w1, b1, w2, b2, pe, alpha, tmp, out, B, d, nullptr, st, stream);
}

int ttts_decode_frame_in_rows(const float* ys, int64_t ld_ys, int n_mels, const float* w1, const float* b1, const float* w2,
                              const float* b2, const float* pe, const float* alpha, float* tmp, float* out, int B, int d,
                              const int64_t* row_end, const ttts_decode_state* st, void* stream) {
    TTTS_REQUIRE(row_end, "decode_frame_in_rows: null pointer (row_end)");
    return decode_frame_in_impl("decode_frame_in_rows", ys, ld_ys, n_mels, w1, b1, w2, b2, pe, alpha, tmp, out, B, d, row_end, st,
                                stream);
}

int ttts_decode_frame_out(const float* x, const float* w_mel, const float* b_mel, const float* w_stop, const float* b_stop,
                          float* ys, int64_t ld_ys, float* stop, int64_t ld_stop, int B, int d, int n_mels,
                          ttts_decode_state* st, void* stream) {
    return decode_frame_out_impl("decode_frame_out", x, w_mel, b_mel, w_stop, b_stop, ys, ld_ys, stop, ld_stop, B, d, n_mels,
                                 nullptr, st, stream);
}

int ttts_decode_frame_out_rows(const float* x, const float* w_mel, const float* b_mel, const float* w_stop, const float* b_stop,
                               float* ys, int64_t ld_ys, float* stop, int64_t ld_stop, int B, int d, int n_mels, int64_t* row_end,
                               ttts_decode_state* st, void* stream) {
    TTTS_REQUIRE(row_end, "decode_frame_out_rows: null pointer (row_end)");
    return decode_frame_out_impl("decode_frame_out_rows", x, w_mel, b_mel, w_stop, b_stop, ys, ld_ys, stop, ld_stop, B, d, n_mels,
                                 row_end, st, stream);
}

int ttts_decode_layernorm(const float* x, const float* gamma, const float* beta, float* y, int M, int d, float eps,
                          const ttts_decode_state* st, void* stream) {
    return decode_layernorm_impl("decode_layernorm", x, gamma, beta, y, M, d, eps, nullptr, st, stream);
}

int ttts_decode_layernorm_rows(const float* x, const float* gamma, const float* beta, float* y, int M, int d, float eps,
                               const int64_t* row_end, const ttts_decode_state* st, void* stream) {
    TTTS_REQUIRE(row_end, "decode_layernorm_rows: null pointer (row_end)");
    return decode_layernorm_impl("decode_layernorm_rows", x, gamma, beta, y, M, d, eps, row_end, st, stream);
}

size_t ttts_decode_attention_workspace_bytes(int B, int H, int head_dim, int max_keys) {
    if (B < 1 || H < 1 || head_dim < 16 || max_keys < 1) return 0;
    return (size_t)B * H * attn_nsplit(max_keys) * (head_dim + 4) * sizeof(float);
}

int ttts_decode_attention(const float* q, int64_t ldq, const float* k, const float* v, int64_t ld_row, int64_t ld_batch,
                          const int64_t* lens, float* out, int64_t ldo, float* ws, size_t ws_bytes, int B, int H, int head_dim,
                          int max_keys, const ttts_decode_state* st, void* stream) {
    const AttnArgs a{q, k, v, (long)ldq, (long)ld_row, (long)ld_batch, lens, out, (long)ldo, ws, B, H, max_keys, nullptr,
                     AttnMap{nullptr, 0, 0, 0}, st, nullptr, nullptr, 0};
    const int rc = check_decode_attention(a, head_dim, ws_bytes, "decode_attention");
    if (rc != TTTS_OK) return rc;
    return launch_decode_attention(a, head_dim, (hipStream_t)stream, "decode_attention");
}

int ttts_decode_attention_rows(const float* q, int64_t ldq, const float* k, const float* v, int64_t ld_row, int64_t ld_batch,
                               const int64_t* lens, float* out, int64_t ldo, float* ws, size_t ws_bytes, int B, int H, int head_dim,
                               int max_keys, const int64_t* row_end, float* map, int64_t map_ld_head, int64_t map_ld_row,
                               int map_rows, const ttts_decode_state* st, void* stream) {
    const AttnArgs a{q, k, v, (long)ldq, (long)ld_row, (long)ld_batch, lens, out, (long)ldo, ws, B, H, max_keys, row_end,
                     AttnMap{map, (long)map_ld_head, (long)map_ld_row, map_rows}, st, nullptr, nullptr, 0};
    TTTS_REQUIRE(row_end, "decode_attention_rows: null pointer (row_end)");
    const int rc = check_decode_attention(a, head_dim, ws_bytes, "decode_attention_rows");
    if (rc != TTTS_OK) return rc;
    TTTS_REQUIRE(map == nullptr || (map_rows >= 1 && map_ld_row >= max_keys && map_ld_head >= (int64_t)map_rows * map_ld_row),
                 "decode_attention_rows: map of %d rows, ld_row=%ld ld_head=%ld (rows >= 1, ld_row >= max_keys=%d, ld_head >= "
                 "rows * ld_row)", map_rows, (long)map_ld_row, (long)map_ld_head, max_keys);
    return launch_decode_attention(a, head_dim, (hipStream_t)stream, "decode_attention_rows");
}

int ttts_decode_attention_window(const float* q, int64_t ldq, const float* k, const float* v, int64_t ld_row, int64_t ld_batch,
                                 const int64_t* lens, float* out, int64_t ldo, float* ws, size_t ws_bytes, int B, int H,
                                 int head_dim, int max_keys, const int64_t* row_end, float* map, int64_t map_ld_head,
                                 int64_t map_ld_row, int map_rows, const ttts_decode_window* win, int32_t* pos, int64_t ld_pos,
                                 const ttts_decode_state* st, void* stream) {
    const AttnArgs a{q, k, v, (long)ldq, (long)ld_row, (long)ld_batch, lens, out, (long)ldo, ws, B, H, max_keys, row_end,
                     AttnMap{map, (long)map_ld_head, (long)map_ld_row, map_rows}, st, win, pos, (long)ld_pos};
    TTTS_REQUIRE(row_end, "decode_attention_window: null pointer (row_end)");
    TTTS_REQUIRE(lens, "decode_attention_window: null pointer (lens)");
    TTTS_REQUIRE(win, "decode_attention_window: null pointer (win)");
    TTTS_REQUIRE(pos, "decode_attention_window: null pointer (pos)");
    const int rc = check_decode_attention(a, head_dim, ws_bytes, "decode_attention_window");
    if (rc != TTTS_OK) return rc;
    TTTS_REQUIRE(H <= 64, "decode_attention_window: H=%d heads (head_mask holds 64)", H);
    TTTS_REQUIRE(ld_pos >= 1 && ((uintptr_t)win & 7) == 0 && ((uintptr_t)pos & 3) == 0,
                 "decode_attention_window: ld_pos=%ld (>= 1), win 8-byte and pos 4-byte aligned", (long)ld_pos);
    TTTS_REQUIRE(map == nullptr || (map_rows >= 1 && map_ld_row >= max_keys && map_ld_head >= (int64_t)map_rows * map_ld_row),
                 "decode_attention_window: map of %d rows, ld_row=%ld ld_head=%ld (rows >= 1, ld_row >= max_keys=%d, ld_head >= "
                 "rows * ld_row)", map_rows, (long)map_ld_row, (long)map_ld_head, max_keys);
    return launch_decode_attention(a, head_dim, (hipStream_t)stream, "decode_attention_window");
}

int ttts_mask_rows(float* x, const int64_t* lens, int64_t outer, int group, int64_t T, int64_t C, void* stream) {
    TTTS_REQUIRE(x && lens, "mask_rows: null pointer");
    TTTS_REQUIRE(outer >= 1 && outer <= 65535 && group >= 1 && T >= 1 && C >= 1,
                 "mask_rows: bad sizes outer=%ld group=%d T=%ld C=%ld (1 <= outer <= 65535)", (long)outer, group, (long)T, (long)C);
    TTTS_REQUIRE(((uintptr_t)x & 3) == 0, "mask_rows: x must be 4-byte aligned");
    const long total = (long)T * C;
    const int blocks = (int)(total / 1024 < 1 ? 1 : (total / 1024 > 64 ? 64 : total / 1024));
    const dim3 grid(blocks, (unsigned)outer);
    if (C % 4 == 0 && ((uintptr_t)x & 15) == 0)
        hipLaunchKernelGGL(mask_rows_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, lens, group, (long)T, (long)C);
    else
        hipLaunchKernelGGL(mask_rows_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, lens, group, (long)T, (long)C);
    TTTS_LAUNCH_CHECK("mask_rows");
    return TTTS_OK;
}

}  // extern "C"
