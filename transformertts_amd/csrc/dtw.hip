// Dynamic time warping between two ragged batches of feature sequences (gfx950): the number that compares a synthesised mel with
// its recording (mel-DTW on log-mels, MCD-DTW on mel-cepstra).  x is (B, Tx, C), y is (B, Ty, C); n_b = x_lens[b] clamped to
// [0, Tx], m_b = y_lens[b] clamped to [0, Ty].  Nothing at row >= n_b of x or row >= m_b of y is ever loaded.
//   cell cost    L1: c[i][j] = sum_k |x[i][k] - y[j][k]|,  L2: c[i][j] = sqrtf(sum_k (x[i][k] - y[j][k])^2),  k = 0 .. C-1 in order
//   recurrence   D[0][0] = c[0][0],  D[i][j] = c[i][j] + min(D[i-1][j-1], D[i-1][j], D[i][j-1]),  a missing predecessor = +inf
//   tie rule     the FIRST minimum wins in the order diagonal (i-1, j-1), then (i-1, j), then (i, j-1)
//   outputs      cost = D[n_b-1][m_b-1], the backtracked path from (n_b-1, m_b-1) to (0, 0), its number of cells, and
//                distance = cost / (path_len * C) (L1) or cost / path_len (L2); all zero / -1 for a row with a zero length
// Two launches per call.  dtw_cost_kernel stages the cells c[i][j], i < n_b, j < m_b, in the caller's workspace (a 64 x 64 tile
// per workgroup, operands through LDS, one fixed channel order per cell).  dtw_dp_kernel runs the recurrence with ONE wave per
// utterance in the shape of align_mas_kernel: lane l owns K neighbouring columns, the rows are skewed by one per lane (lane l
// works on row s - l at step s), so a step needs one __shfl_up from lane l - 1 and no barrier; a ring of DTW_PF steps of cost loads
// runs ahead of the dependent chain; the 2-bit directions of a lane's K cells go to one 32-bit word per lane and step.  Wider
// than 64 K columns: strips of 64 K columns one after the other, the last column of a strip handed on through Tx floats.  The
// backtrack reads the words back DTW_ROWS rows at a time through LDS, every lane alike.  All arithmetic fp32, no atomics, no host
// read, nothing depends on B, Tx, Ty or the strides beyond addressing: the call captures into a HIP graph and repeats bit for bit.
#include "ttts_common.h"

#include <math.h>

namespace ttts {

constexpr int DTW_MAX_LEN = 4096;        // frames per side
constexpr int DTW_MAX_LOGK = 4;          // up to 16 columns per lane: 32 direction bits
constexpr int DTW_TILE = 64;             // cost kernel: cells per side of a workgroup's tile
constexpr int DTW_CK = 32;               // cost kernel: channels staged in LDS at a time
constexpr int DTW_PF = 4;                // recurrence: steps of cost loads in flight ahead of the dependent chain
constexpr int DTW_ROWS = 64;             // backtrack: rows of direction words staged in LDS at a time

__host__ __device__ static inline int dtw_logk(int Ty) {
    int logk = 0;
    while (logk < DTW_MAX_LOGK && (64L << logk) < Ty) ++logk;
    return logk;
}
__host__ __device__ static inline long dtw_strips(int Ty) {
    const long W = 64L << dtw_logk(Ty);
    return (Ty + W - 1) / W;
}
// the workspace of one utterance in 4-byte words: costs (Tx, Ty) | direction words (strips, Tx + 63, 64) | strip edges (strips, Tx)
// | the path in backtrack order (Tx + Ty, 2)
__host__ __device__ static inline long dtw_words(int Tx, int Ty) {
    const long strips = dtw_strips(Ty);
    return (long)Tx * Ty + strips * (Tx + 63L) * 64 + strips * Tx + 2L * (Tx + Ty);
}

__device__ __forceinline__ int dtw_len(const int64_t* lens, int b, int cap) {
    long v = lens[b];
    return (int)(v < 0 ? 0 : v > cap ? cap : v);
}

// ---------------------------------------------------------------- cell costs
// One workgroup per 64 x 64 tile of cells of one utterance; thread (ty, tx) holds the 4 x 4 cells (ty + 16 r, tx + 16 c).  Every
// cell adds its channels in the order k = 0 .. C-1 whatever the tile, the batch or the strides.
template <int METRIC>
__global__ __launch_bounds__(256) void dtw_cost_kernel(const float* x, long ldx_row, long ldx_batch, const int64_t* x_lens,
                                                       const float* y, long ldy_row, long ldy_batch, const int64_t* y_lens, int Tx,
                                                       int Ty, int C, float* ws, long words) {
    __shared__ float xs[DTW_TILE][DTW_CK + 1], ys[DTW_TILE][DTW_CK + 1];
    const int b = blockIdx.z, i0 = blockIdx.y * DTW_TILE, j0 = blockIdx.x * DTW_TILE;
    const int n = dtw_len(x_lens, b, Tx), m = dtw_len(y_lens, b, Ty);
    if (i0 >= n || j0 >= m) return;                              // (uniform)
    const float* xb = x + b * ldx_batch;
    const float* yb = y + b * ldy_batch;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    float acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
    for (int c0 = 0; c0 < C; c0 += DTW_CK) {
        for (int e = threadIdx.x; e < DTW_TILE * DTW_CK; e += 256) {
            const int r = e / DTW_CK, k = e % DTW_CK;
            const bool ch = c0 + k < C;
            xs[r][k] = (ch && i0 + r < n) ? xb[(long)(i0 + r) * ldx_row + c0 + k] : 0.f;
            ys[r][k] = (ch && j0 + r < m) ? yb[(long)(j0 + r) * ldy_row + c0 + k] : 0.f;
        }
        __syncthreads();
        const int kn = C - c0 < DTW_CK ? C - c0 : DTW_CK;
        for (int k = 0; k < kn; ++k) {
            float xv[4], yv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) xv[r] = xs[ty + 16 * r][k];
#pragma unroll
            for (int c = 0; c < 4; ++c) yv[c] = ys[tx + 16 * c][k];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float d = xv[r] - yv[c];
                    acc[r][c] = METRIC == TTTS_DTW_L1 ? acc[r][c] + fabsf(d) : fmaf(d, d, acc[r][c]);
                }
        }
        __syncthreads();
    }
    float* costs = ws + (long)b * words;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = i0 + ty + 16 * r, j = j0 + tx + 16 * c;
            if (i < n && j < m) costs[(long)i * Ty + j] = METRIC == TTTS_DTW_L1 ? acc[r][c] : sqrtf(acc[r][c]);
        }
}

// ---------------------------------------------------------------- recurrence and backtrack
// One wave per utterance.  Within a strip of W = 64 K columns lane l holds D[i][j] of its columns j = j_first .. j_first + K - 1 for
// the row i = s - l it reached at step s; `left` is lane l - 1's last column on the same row (it was there one step earlier) and
// what `left` held the step before is the diagonal predecessor of the lane's first column.  Lane 0 takes both from the strip to
// its left (the edge array), or +inf in the first strip -- but for the diagonal of (0, 0), which holds 0 and makes D[0][0] =
// c[0][0].  Rows outside [0, n) and columns from m on hold +inf and are never acted on; their cost loads are clamped onto the
// last row / column of the utterance, so no load sits behind a branch.  Direction of a cell: 0 diagonal, 1 (i-1, j), 2 (i, j-1);
// a later candidate replaces only on `<`, which is the tie rule.
template <int LOGK>
__global__ __launch_bounds__(64) void dtw_dp_kernel(const int64_t* x_lens, const int64_t* y_lens, int Tx, int Ty, int C, int metric,
                                                    float* ws, long words, float* cost, int64_t* path_len, float* distance,
                                                    uint8_t* valid, int32_t* path) {
    constexpr int K = 1 << LOGK, W = 64 * K;
    __shared__ unsigned int bits[(DTW_ROWS + 63) * 64];
    const int lane = threadIdx.x, b = blockIdx.x;
    const int n = dtw_len(x_lens, b, Tx), m = dtw_len(y_lens, b, Ty);
    const long cells = (long)Tx + Ty - 1;
    int32_t* prow = path ? path + (long)b * cells * 2 : nullptr;
    if (n == 0 || m == 0) {
        if (lane == 0) {
            cost[b] = 0.f;
            path_len[b] = 0;
            distance[b] = 0.f;
            valid[b] = 0;
        }
        if (prow)
            for (long e = lane; e < cells * 2; e += 64) prow[e] = -1;
        return;
    }
    const long strips_all = dtw_strips(Ty);
    float* wsb = ws + (long)b * words;
    const float* costs = wsb;
    unsigned int* bitw = reinterpret_cast<unsigned int*>(wsb + (long)Tx * Ty);
    float* edges = wsb + (long)Tx * Ty + strips_all * (Tx + 63L) * 64;
    int32_t* rev = reinterpret_cast<int32_t*>(edges + strips_all * Tx);
    const long bit_strip = (Tx + 63L) * 64;

    const int strips = (m - 1) / W + 1;
    const int owner = ((m - 1) & (W - 1)) >> LOGK;             // the lane that holds column m - 1 in the last strip
    float fin = 0.f;
    for (int p = 0; p < strips; ++p) {
        const int j_first = p * W + lane * K;
        const int cols = m - p * W < W ? m - p * W : W;
        const int steps = n + ((cols - 1) >> LOGK);             // the last lane with a column reaches row n - 1 at steps - 1
        const float* ein = edges + (long)(p > 0 ? p - 1 : 0) * Tx;
        float* eout = edges + (long)p * Tx;
        unsigned int* bw = bitw + p * bit_strip;
        long col[K];
        float q[K], buf[DTW_PF][K], ebuf[DTW_PF];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            col[k] = j_first + k < m ? j_first + k : m - 1;
            q[k] = INFINITY;
        }
#pragma unroll
        for (int j = 0; j < DTW_PF; ++j) {
            const int r = j - lane;
            const long row = r < 0 ? 0 : r < n ? r : n - 1;
#pragma unroll
            for (int k = 0; k < K; ++k) buf[j][k] = costs[row * Ty + col[k]];
            ebuf[j] = p > 0 ? ein[j < n ? j : n - 1] : INFINITY; // (uniform: strip 0 has no strip to its left)
        }
        // the ring's first fill lands before the loop (see align_mas_kernel): vmcnt(0), the other counters untouched
        __builtin_amdgcn_s_waitcnt(0x0F70);
        float diag_in = (p == 0 && lane == 0) ? 0.f : INFINITY;

        for (int s0 = 0; s0 < steps; s0 += DTW_PF) {
#pragma unroll
            for (int j = 0; j < DTW_PF; ++j) {
                const int s = s0 + j;
                if (s < steps) {                                // (uniform)
                    float left = __shfl_up(q[K - 1], 1, 64);
                    if (lane == 0) left = ebuf[j];
                    const int i = s - lane;
                    const bool row_on = i >= 0 && i < n;
                    float dg = diag_in, lf = left;
                    unsigned int word = 0;
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        // off the chain: the better predecessor in the row above (the diagonal keeps a tie) and the cell's cost
                        const float up = q[k];
                        const bool take_up = up < dg;
                        const float above = take_up ? up : dg;
                        const float c = (row_on && j_first + k < m) ? buf[j][k] : INFINITY;
                        // the chain from cell to cell: one minimum and one add ((i, j-1) replaces only on `<`; the value is the
                        // same either way on a tie)
                        const bool take_left = lf < above;
                        const float v = c + fminf(lf, above);
                        word |= (take_left ? 2u : take_up ? 1u : 0u) << (2 * k);
                        dg = up;
                        lf = v;
                        q[k] = v;
                    }
                    diag_in = left;
                    if (i == n - 1 && lane == owner && p == strips - 1) {      // once: the last cell of the matrix
                        const int kk = (m - 1) & (K - 1);
                        fin = q[0];
#pragma unroll
                        for (int k = 1; k < K; ++k) fin = k == kk ? q[k] : fin;
                    }
                    if (row_on) {
                        bw[(long)s * 64 + lane] = word;
                        if (lane == 63 && p + 1 < strips) eout[i] = q[K - 1];
                    }
                }
                const int sn = s + DTW_PF;
                const int r = sn - lane;
                const long row = r < 0 ? 0 : r < n ? r : n - 1;
#pragma unroll
                for (int k = 0; k < K; ++k) buf[j][k] = costs[row * Ty + col[k]];
                if (p > 0) ebuf[j] = ein[sn < n ? sn : n - 1];
            }
        }
        // NOT a redundant barrier of a one-wave block: lane 63 stored the strip's last column and lane 0 reads it in the next
        // strip, every lane stored direction words that the whole wave reads back below.  What orders them is the workgroup-scope
        // fence __syncthreads() carries (as in align_mas_kernel).
        __syncthreads();
    }
    const float total = __shfl(fin, owner, 64);

    // backtrack, every lane alike; lane t & 63 keeps cell t of the walk and the wave stores 64 cells at a time
    int i = n - 1, j = m - 1, t = 0, mi = 0, mj = 0;
    int blk_p = -1, blk_lo = 0;
    for (;;) {
        if (lane == (t & 63)) { mi = i; mj = j; }
        ++t;
        if (prow && (t & 63) == 0) {
            rev[2L * (t - 64 + lane)] = mi;
            rev[2L * (t - 64 + lane) + 1] = mj;
        }
        if (i == 0 && j == 0) break;
        const int p = j >> (6 + LOGK);
        if (p != blk_p || i < blk_lo) {                          // (uniform) the words of rows blk_lo .. i of strip p
            __syncthreads();
            blk_p = p;
            blk_lo = i - (DTW_ROWS - 1) > 0 ? i - (DTW_ROWS - 1) : 0;
            const int nw = (i - blk_lo + 64) * 64;               // steps blk_lo .. i + 63
            const unsigned int* src = bitw + p * bit_strip + (long)blk_lo * 64;
            for (int e = lane; e < nw; e += 64) bits[e] = src[e];
            __syncthreads();
        }
        const int jl = j & (W - 1), ln = jl >> LOGK;
        unsigned int d = (bits[(i + ln - blk_lo) * 64 + ln] >> (2 * (jl & (K - 1)))) & 3u;
        if (i == 0) d = 2;                                       // the walk stays inside the matrix whatever the words hold
        else if (j == 0) d = 1;
        if (d != 2) --i;
        if (d != 1) --j;
    }
    if (prow) {
        const int rem = t & 63;
        if (lane < rem) {
            rev[2L * (t - rem + lane)] = mi;
            rev[2L * (t - rem + lane) + 1] = mj;
        }
        __syncthreads();                                         // (the same fence: other lanes read the cells back)
        for (long e = lane; e < cells; e += 64) {
            const bool in = e < t;
            prow[2 * e] = in ? rev[2L * (t - 1 - e)] : -1;
            prow[2 * e + 1] = in ? rev[2L * (t - 1 - e) + 1] : -1;
        }
    }
    if (lane == 0) {
        cost[b] = total;
        path_len[b] = t;
        distance[b] = metric == TTTS_DTW_L1 ? total / ((float)t * (float)C) : total / (float)t;
        valid[b] = 1;
    }
}

}  // namespace ttts

using namespace ttts;

extern "C" {

size_t ttts_dtw_workspace_bytes(int B, int Tx, int Ty) {
    if (B <= 0 || Tx <= 0 || Ty <= 0 || Tx > DTW_MAX_LEN || Ty > DTW_MAX_LEN) return 0;
    return (size_t)B * (size_t)dtw_words(Tx, Ty) * 4;
}

int ttts_dtw(const float* x, int64_t ldx_row, int64_t ldx_batch, const int64_t* x_lens, const float* y, int64_t ldy_row,
             int64_t ldy_batch, const int64_t* y_lens, int B, int Tx, int Ty, int C, int metric, void* ws, size_t ws_bytes, float* cost,
             int64_t* path_len, float* distance, uint8_t* valid, int32_t* path, void* stream) {
    const char* name = "dtw";
    TTTS_REQUIRE(x && x_lens && y && y_lens && ws && cost && path_len && distance && valid, "%s: null pointer", name);
    TTTS_REQUIRE(B > 0 && Tx > 0 && Ty > 0 && C > 0, "%s: sizes must be positive (B %d, Tx %d, Ty %d, C %d)", name, B, Tx, Ty, C);
    TTTS_REQUIRE(ldx_row >= C && ldy_row >= C, "%s: the row strides must be >= C (ldx_row %lld, ldy_row %lld, C %d)", name,
                 (long long)ldx_row, (long long)ldy_row, C);
    TTTS_REQUIRE(ldx_batch >= 0 && ldy_batch >= 0, "%s: strides must not be negative (ldx_batch %lld, ldy_batch %lld)", name,
                 (long long)ldx_batch, (long long)ldy_batch);
    TTTS_REQUIRE(metric == TTTS_DTW_L1 || metric == TTTS_DTW_L2, "%s: unknown metric %d", name, metric);
    TTTS_REQUIRE(Tx <= DTW_MAX_LEN && Ty <= DTW_MAX_LEN, "%s: lengths above %d frames are not supported (Tx %d, Ty %d)", name,
                 DTW_MAX_LEN, Tx, Ty);
    TTTS_REQUIRE(B <= 65535, "%s: grid too large (B %d, at most 65535 utterances a call)", name, B);
    TTTS_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 3) == 0, "%s: the workspace must be 4-byte aligned", name);
    const size_t need = ttts_dtw_workspace_bytes(B, Tx, Ty);
    TTTS_REQUIRE(ws_bytes >= need, "%s: workspace too small (%zu bytes, %zu needed)", name, ws_bytes, need);
    const long words = dtw_words(Tx, Ty);
    float* w = static_cast<float*>(ws);
    const dim3 cgrid((unsigned)cdiv(Ty, DTW_TILE), (unsigned)cdiv(Tx, DTW_TILE), (unsigned)B);
    if (metric == TTTS_DTW_L1)
        hipLaunchKernelGGL(dtw_cost_kernel<TTTS_DTW_L1>, cgrid, dim3(256), 0, (hipStream_t)stream, x, (long)ldx_row, (long)ldx_batch,
                           x_lens, y, (long)ldy_row, (long)ldy_batch, y_lens, Tx, Ty, C, w, words);
    else
        hipLaunchKernelGGL(dtw_cost_kernel<TTTS_DTW_L2>, cgrid, dim3(256), 0, (hipStream_t)stream, x, (long)ldx_row, (long)ldx_batch,
                           x_lens, y, (long)ldy_row, (long)ldy_batch, y_lens, Tx, Ty, C, w, words);
    TTTS_LAUNCH_CHECK("dtw_cost_kernel");
#define TTTS_DTW_LAUNCH(LOGK)                                                                                                  \
    hipLaunchKernelGGL(dtw_dp_kernel<LOGK>, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, x_lens, y_lens, Tx, Ty, C, metric, w, \
                       words, cost, path_len, distance, valid, path)
    switch (dtw_logk(Ty)) {
        case 0: TTTS_DTW_LAUNCH(0); break;
        case 1: TTTS_DTW_LAUNCH(1); break;
        case 2: TTTS_DTW_LAUNCH(2); break;
        case 3: TTTS_DTW_LAUNCH(3); break;
        default: TTTS_DTW_LAUNCH(4); break;
    }
#undef TTTS_DTW_LAUNCH
    TTTS_LAUNCH_CHECK("dtw_dp_kernel");
    return TTTS_OK;
}

}  // extern "C"
