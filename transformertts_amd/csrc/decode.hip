// Autoregressive decoding (TransformerTTS.inference with K/V caches): the kernels of ONE frame, for M = B rows.
// At these row counts every GEMM is a weight-streaming GEMV: plain fp32 FMA chains, weights loaded straight to VGPRs with
// 16-byte loads before anything else (their latency overlaps the state read), no MFMA, no partial maxima, no pre-scales.
// Everything that changes from frame to frame or from call to call (frame index t, max_len, stop threshold, the stop frame)
// is read from the caller's ttts_decode_state when the kernel runs, so one captured HIP graph of a chunk of frames serves
// every frame and every call; every kernel returns at once when t >= t_end or a stop frame has been recorded.
// Summation orders are fixed (per lane in index order, then the wave butterfly, then waves / key blocks in index order) and
// depend on neither M, B nor the buffer capacities: a synthesized call is bitwise reproducible.  No atomics.
#include "ttts_common.h"

namespace ttts {
namespace {

constexpr int DEC_ROWS = 4;       // rows of one decode-linear workgroup (grid.y covers M)
constexpr int DEC_KMAX = 4096;    // widest K (16 float4 per lane)
constexpr int ATTN_KEYS = 64;     // keys per attention workgroup (16 per wave, four lanes per key)
constexpr int LN_PER = 16;        // decode LayerNorm: d <= 64 * LN_PER

__device__ __forceinline__ bool decode_done(const ttts_decode_state* st, int64_t& t) {
    t = st->t;
    return t >= st->t_end || st->stop_frame >= 0;
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
};

// y[M,N] = act(x . w^T + b) (+ res) (+ alpha pe[t-1]).  Wave = NC output columns; lane l holds the float4 chunks l, l+64, ...
// of each column's weight row (KC of them); one workgroup = 4 waves x DEC_ROWS rows, its activation rows loaded up front.
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
    int64_t t;
    if (decode_done(a.st, t)) return;
    const long tr = (long)(t - 1);
    // the workgroup's rows: every activation load is issued before the first product (one L2 round trip, not one per row)
    const int m0 = blockIdx.y * DEC_ROWS;
    float4 xv[DEC_ROWS][KC];
#pragma unroll
    for (int r = 0; r < DEC_ROWS; ++r) {
        const int m = min(m0 + r, a.M - 1);
        const float4* xr = reinterpret_cast<const float4*>(a.x + (long)m * a.ldx + tr * a.x_ts);
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            const int k4 = lane + 64 * j;
            xv[r][j] = k4 < K4 ? xr[k4] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
#pragma unroll
    for (int r = 0; r < DEC_ROWS; ++r) {
        const int m = m0 + r;
        if (m >= a.M) break;
        float acc[NC];
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
            if (lane != c || n >= a.N) continue;
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
template <int KC>
__global__ __launch_bounds__(256) void decode_stop_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ b, float* __restrict__ stop, long ld_stop,
                                                          int M, int K, ttts_decode_state* st) {
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
    int64_t t;
    if (decode_done(st, t)) return;           // (uniform over the workgroup)
    const float thr = st->stop_threshold;
    const float bias = b != nullptr ? b[0] : 0.f;
    int ok = 1;
    for (int mb = wave * 4; mb < M; mb += 16) {            // four rows per wave at a time, their loads issued together
        float4 xv[4][KC];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float4* xr = reinterpret_cast<const float4*>(x + (long)min(mb + r, M - 1) * K);
#pragma unroll
            for (int j = 0; j < KC; ++j) {
                const int k4 = lane + 64 * j;
                xv[r][j] = k4 < K4 ? xr[k4] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = mb + r;
            if (m >= M) break;
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < KC; ++j) s = dot4(xv[r][j], wv[j], s);
            const float v = wave_sum(s) + bias;
            if (lane == 0) stop[(long)m * ld_stop + (t - 1)] = v;
            const float p = 1.0f / (1.0f + expf(-v));
            ok &= (p >= thr) ? 1 : 0;
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
                                                               float eps, const ttts_decode_state* st) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wave;
    if (row >= M) return;
    int64_t t;
    if (decode_done(st, t)) return;
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
template <int HD>
__global__ __launch_bounds__(256) void decode_attn_partial_kernel(const float* __restrict__ q, long ldq, const float* __restrict__ k,
                                                                  const float* __restrict__ v, long ld_row, long ld_batch,
                                                                  const int64_t* __restrict__ lens, float* __restrict__ ws, int H,
                                                                  int nsplit, int max_keys, float scale, const ttts_decode_state* st) {
    constexpr int CH = HD / 16;               // float4 per lane
    constexpr int WS = HD + 4;                // workspace floats per block
    __shared__ float red_m[4], red_l[4];
    __shared__ float4 red_o[4][HD / 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    int64_t t;
    if (decode_done(st, t)) return;
    long len = lens != nullptr ? (long)lens[b] : (long)t;
    len = len < (long)max_keys ? len : (long)max_keys;
    const int key0 = s * ATTN_KEYS;
    if (key0 >= len) return;                  // (uniform over the workgroup)
    const int key = key0 + wave * 16 + (lane >> 2), sub = lane & 3;
    const long col = (long)h * HD + sub * (HD / 4);
    const float4* q4 = reinterpret_cast<const float4*>(q + (long)b * ldq + col);
    const bool live = key < len;
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
    __syncthreads();
    const float mb = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));   // finite: key0 < len
    const float p = live ? expf(sc - mb) : 0.f;
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
    }
}

// one wave per (head, utterance): out = sum_s o_s e^(m_s - m) / sum_s l_s e^(m_s - m) over the blocks below the length
template <int HD>
__global__ __launch_bounds__(64) void decode_attn_combine_kernel(const float* __restrict__ ws, const int64_t* __restrict__ lens,
                                                                 float* __restrict__ out, long ldo, int H, int nsplit, int max_keys,
                                                                 const ttts_decode_state* st) {
    constexpr int WS = HD + 4;
    const int lane = threadIdx.x, h = blockIdx.x, b = blockIdx.y;
    int64_t t;
    if (decode_done(st, t)) return;
    long len = lens != nullptr ? (long)lens[b] : (long)t;
    len = len < (long)max_keys ? len : (long)max_keys;
    const int nblk = len > 0 ? (int)((len + ATTN_KEYS - 1) / ATTN_KEYS) : 0;
    const float* p = ws + ((long)b * H + h) * nsplit * WS;
    float m = -INFINITY;
    for (int s = 0; s < nblk; ++s) m = fmaxf(m, p[s * WS + HD]);
    float l = 0.f, o0 = 0.f, o1 = 0.f;
    for (int s = 0; s < nblk; ++s) {
        const float e = expf(p[s * WS + HD] - m);
        l = fmaf(p[s * WS + HD + 1], e, l);
        if (lane < HD) o0 = fmaf(p[s * WS + lane], e, o0);
        if (lane + 64 < HD) o1 = fmaf(p[s * WS + lane + 64], e, o1);
    }
    const float inv = nblk > 0 ? 1.0f / l : 0.f;
    float* orow = out + (long)b * ldo + (long)h * HD;
    if (lane < HD) orow[lane] = o0 * inv;
    if (lane + 64 < HD) orow[lane + 64] = o1 * inv;
}

int attn_nsplit(int max_keys) { return cdiv(max_keys, ATTN_KEYS); }

template <int HD>
void launch_decode_attention_t(const float* q, long ldq, const float* k, const float* v, long ld_row, long ld_batch,
                               const int64_t* lens, float* out, long ldo, float* ws, int B, int H, int max_keys,
                               const ttts_decode_state* st, hipStream_t stream) {
    const int ns = attn_nsplit(max_keys);
    const float scale = 1.0f / sqrtf((float)HD);
    hipLaunchKernelGGL((decode_attn_partial_kernel<HD>), dim3(ns, H, B), dim3(256), 0, stream, q, ldq, k, v, ld_row, ld_batch,
                       lens, ws, H, ns, max_keys, scale, st);
    hipLaunchKernelGGL((decode_attn_combine_kernel<HD>), dim3(H, B), dim3(64), 0, stream, ws, lens, out, ldo, H, ns, max_keys, st);
}

}  // namespace
}  // namespace ttts

using namespace ttts;

extern "C" {

int ttts_decode_linear(const float* x, int64_t ldx, int64_t x_tstride, const float* w, const float* bias, const float* residual,
                       int64_t ldr, float* y, int64_t ldy, int64_t y_tstride, float* y2, int64_t ldy2, int64_t y2_tstride,
                       int n_split, int M, int N, int K, int act, const ttts_decode_state* st, void* stream) {
    DecLinArgs a{x, (long)ldx, (long)x_tstride, w, bias, residual, (long)ldr, nullptr, nullptr, y, (long)ldy, (long)y_tstride,
                 y2, (long)ldy2, (long)y2_tstride, n_split, M, N, K, act, st};
    TTTS_REQUIRE(residual == nullptr || ldr >= N || M == 1, "decode_linear: ldr=%ld < N=%d", (long)ldr, N);
    const int rc = check_decode_linear(a, "decode_linear");
    if (rc != TTTS_OK) return rc;
    return launch_decode_linear(a, (hipStream_t)stream);
}

int ttts_decode_frame_in(const float* ys, int64_t ld_ys, int n_mels, const float* w1, const float* b1, const float* w2,
                         const float* b2, const float* pe, const float* alpha, float* tmp, float* out, int B, int d,
                         const ttts_decode_state* st, void* stream) {
    TTTS_REQUIRE(ys && w1 && w2 && pe && alpha && tmp && out && st, "decode_frame_in: null pointer");
    TTTS_REQUIRE(B >= 1 && d >= 4 && d % 4 == 0 && n_mels >= 4 && n_mels % 4 == 0 && ld_ys >= n_mels,
                 "decode_frame_in: bad sizes B=%d d=%d n_mels=%d ld_ys=%ld (d, n_mels multiples of 4)", B, d, n_mels, (long)ld_ys);
    TTTS_REQUIRE(((uintptr_t)tmp & 15) == 0, "decode_frame_in: tmp must be 16-byte aligned");
    DecLinArgs l1{ys, (long)ld_ys, (long)n_mels, w1, b1, nullptr, 0, nullptr, nullptr, tmp, (long)d, 0, nullptr, 0, 0, d, B, d,
                  n_mels, TTTS_ACT_RELU, st};
    DecLinArgs l2{tmp, (long)d, 0, w2, b2, nullptr, 0, pe, alpha, out, (long)d, 0, nullptr, 0, 0, d, B, d, d, TTTS_ACT_RELU, st};
    int rc = check_decode_linear(l1, "decode_frame_in (pre-net linear1)");
    if (rc == TTTS_OK) rc = check_decode_linear(l2, "decode_frame_in (pre-net linear2)");
    if (rc != TTTS_OK) return rc;
    rc = launch_decode_linear(l1, (hipStream_t)stream);
    if (rc != TTTS_OK) return rc;
    return launch_decode_linear(l2, (hipStream_t)stream);
}

int ttts_decode_frame_out(const float* x, const float* w_mel, const float* b_mel, const float* w_stop, const float* b_stop,
                          float* ys, int64_t ld_ys, float* stop, int64_t ld_stop, int B, int d, int n_mels,
                          ttts_decode_state* st, void* stream) {
    TTTS_REQUIRE(x && w_mel && w_stop && ys && stop && st, "decode_frame_out: null pointer");
    TTTS_REQUIRE(B >= 1 && d >= 4 && d % 4 == 0 && d <= DEC_KMAX && n_mels >= 1 && ld_ys >= n_mels && ld_stop >= 1,
                 "decode_frame_out: bad sizes B=%d d=%d n_mels=%d ld_ys=%ld ld_stop=%ld", B, d, n_mels, (long)ld_ys, (long)ld_stop);
    TTTS_REQUIRE(((uintptr_t)w_stop & 15) == 0, "decode_frame_out: w_stop must be 16-byte aligned");
    // frame t of ys: row (t - 1) + 1
    DecLinArgs mel{x, (long)d, 0, w_mel, b_mel, nullptr, 0, nullptr, nullptr, ys + n_mels, (long)ld_ys, (long)n_mels, nullptr, 0, 0,
                   n_mels, B, n_mels, d, TTTS_ACT_NONE, st};
    int rc = check_decode_linear(mel, "decode_frame_out (mel head)");
    if (rc != TTTS_OK) return rc;
    rc = launch_decode_linear(mel, (hipStream_t)stream);
    if (rc != TTTS_OK) return rc;
    const int kc = cdiv(d, 256);
    hipStream_t s = (hipStream_t)stream;
    if (kc <= 1) hipLaunchKernelGGL(decode_stop_kernel<1>, dim3(1), dim3(256), 0, s, x, w_stop, b_stop, stop, (long)ld_stop, B, d, st);
    else if (kc <= 2) hipLaunchKernelGGL(decode_stop_kernel<2>, dim3(1), dim3(256), 0, s, x, w_stop, b_stop, stop, (long)ld_stop, B, d, st);
    else if (kc <= 4) hipLaunchKernelGGL(decode_stop_kernel<4>, dim3(1), dim3(256), 0, s, x, w_stop, b_stop, stop, (long)ld_stop, B, d, st);
    else if (kc <= 8) hipLaunchKernelGGL(decode_stop_kernel<8>, dim3(1), dim3(256), 0, s, x, w_stop, b_stop, stop, (long)ld_stop, B, d, st);
    else hipLaunchKernelGGL(decode_stop_kernel<16>, dim3(1), dim3(256), 0, s, x, w_stop, b_stop, stop, (long)ld_stop, B, d, st);
    TTTS_LAUNCH_CHECK("decode_frame_out");
    return TTTS_OK;
}

int ttts_decode_layernorm(const float* x, const float* gamma, const float* beta, float* y, int M, int d, float eps,
                          const ttts_decode_state* st, void* stream) {
    TTTS_REQUIRE(x && gamma && beta && y && st, "decode_layernorm: null pointer");
    TTTS_REQUIRE(M >= 1 && d >= 1 && d <= 64 * LN_PER && M <= 4 * 65535, "decode_layernorm: bad sizes M=%d d=%d (d <= %d)", M, d,
                 64 * LN_PER);
    hipLaunchKernelGGL(decode_layernorm_kernel, dim3(cdiv(M, 4)), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, y, M, d, eps, st);
    TTTS_LAUNCH_CHECK("decode_layernorm");
    return TTTS_OK;
}

size_t ttts_decode_attention_workspace_bytes(int B, int H, int head_dim, int max_keys) {
    if (B < 1 || H < 1 || head_dim < 16 || max_keys < 1) return 0;
    return (size_t)B * H * attn_nsplit(max_keys) * (head_dim + 4) * sizeof(float);
}

int ttts_decode_attention(const float* q, int64_t ldq, const float* k, const float* v, int64_t ld_row, int64_t ld_batch,
                          const int64_t* lens, float* out, int64_t ldo, float* ws, size_t ws_bytes, int B, int H, int head_dim,
                          int max_keys, const ttts_decode_state* st, void* stream) {
    TTTS_REQUIRE(q && k && v && out && ws && st, "decode_attention: null pointer");
    TTTS_REQUIRE(B >= 1 && H >= 1 && B <= 65535 && H <= 65535 && max_keys >= 1,
                 "decode_attention: bad sizes B=%d H=%d max_keys=%d", B, H, max_keys);
    TTTS_REQUIRE(head_dim >= 16 && head_dim <= 128 && head_dim % 16 == 0,
                 "decode_attention: head_dim=%d (a multiple of 16 up to 128)", head_dim);
    TTTS_REQUIRE(ldq % 4 == 0 && ld_row % 4 == 0 && ld_batch % 4 == 0 && ldq >= (int64_t)H * head_dim && ld_row >= (int64_t)H * head_dim &&
                 ld_batch >= 0 && ldo >= (int64_t)H * head_dim,
                 "decode_attention: strides ldq=%ld ld_row=%ld ld_batch=%ld ldo=%ld (multiples of 4, >= H * head_dim)", (long)ldq,
                 (long)ld_row, (long)ld_batch, (long)ldo);
    TTTS_REQUIRE((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)ws) & 15) == 0,
                 "decode_attention: q, k, v and ws must be 16-byte aligned");
    TTTS_REQUIRE(ws_bytes >= ttts_decode_attention_workspace_bytes(B, H, head_dim, max_keys),
                 "decode_attention: workspace of %zu bytes < %zu", ws_bytes, ttts_decode_attention_workspace_bytes(B, H, head_dim, max_keys));
    hipStream_t s = (hipStream_t)stream;
    switch (head_dim) {
        case 16: launch_decode_attention_t<16>(q, ldq, k, v, ld_row, ld_batch, lens, out, ldo, ws, B, H, max_keys, st, s); break;
        case 32: launch_decode_attention_t<32>(q, ldq, k, v, ld_row, ld_batch, lens, out, ldo, ws, B, H, max_keys, st, s); break;
        case 48: launch_decode_attention_t<48>(q, ldq, k, v, ld_row, ld_batch, lens, out, ldo, ws, B, H, max_keys, st, s); break;
        case 64: launch_decode_attention_t<64>(q, ldq, k, v, ld_row, ld_batch, lens, out, ldo, ws, B, H, max_keys, st, s); break;
        case 80: launch_decode_attention_t<80>(q, ldq, k, v, ld_row, ld_batch, lens, out, ldo, ws, B, H, max_keys, st, s); break;
        case 96: launch_decode_attention_t<96>(q, ldq, k, v, ld_row, ld_batch, lens, out, ldo, ws, B, H, max_keys, st, s); break;
        case 112: launch_decode_attention_t<112>(q, ldq, k, v, ld_row, ld_batch, lens, out, ldo, ws, B, H, max_keys, st, s); break;
        default: launch_decode_attention_t<128>(q, ldq, k, v, ld_row, ld_batch, lens, out, ldo, ws, B, H, max_keys, st, s); break;
    }
    TTTS_LAUNCH_CHECK("decode_attention");
    return TTTS_OK;
}

}  // extern "C"
