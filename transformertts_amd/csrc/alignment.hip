// Phoneme durations read off the decoder's alignment maps (gfx950): what a Transformer-TTS teacher hands a non-autoregressive
// student.  Per decoder layer one (B,H,Tm,Tp) map A; T_b = melspec_lens[b], N_b = phoneme_lens[b], clamped to the maps' extent.
//   row statistics   one wave per (b, h, t) row: max_n A[t][n] over n < N_b and its FIRST argmax (torch.argmax's tie rule)
//   focus rate       F[layer][b][h] = (1 / T_b) sum_{t < T_b} max_n A[t][n]       (0 when T_b = 0 or N_b = 0)
//   head choice      per utterance / one for the batch / given: choice[b] = layer * H + head, decided on the device
//   argmax durations dur[b][n] = #{t < T_b : argmax[choice[b]][b][t] = n}
//   MAS              the best monotonic path through log A of the chosen plane (Glow-TTS), durations >= 1 that sum to T_b
// Nothing at t >= T_b or n >= N_b is ever loaded.  Sums run in a fixed order (lane order, then the xor tree), counts are integer
// adds in LDS, no atomics on global memory, nothing is read back: the whole extraction captures into a HIP graph and repeats bit
// for bit.  Maps are addressed through (ld_row, ld_head, ld_batch) with unit column stride and dword loads: no alignment asked.
#include "ttts_common.h"

#include <limits.h>
#include <math.h>

namespace ttts {

constexpr int ALIGN_MAX_MAPS = TTTS_ALIGN_MAX_MAPS;
constexpr int ALIGN_COUNT_TP = 4096;     // argmax durations: one LDS counter per phoneme
constexpr int ALIGN_MAS_TP = 1024;       // MAS: one wave per utterance, up to 16 phonemes per lane
constexpr int ALIGN_SELECT_MAX = 1024;   // batch mode: one LDS float per (layer, head)
constexpr int MAS_PF = 8;                // MAS: map rows in flight ahead of the dependent chain
constexpr int MAS_ROWS = 64;             // MAS backtrack: rows of decision bits staged in LDS at a time

struct AlignMaps {
    const float* p[ALIGN_MAX_MAPS];
};

__device__ __forceinline__ int align_len(const int64_t* lens, int b, int cap) {
    long v = lens[b];
    return (int)(v < 0 ? 0 : v > cap ? cap : v);
}

// ---------------------------------------------------------------- row statistics and focus rate
// amax[row] = first argmax of row (b, h, t) over n < N_b, rmax[row] = its maximum; 0 / 0 for a row past T_b or with N_b = 0.
// A lane walks its columns upwards and replaces only on `>`, so it keeps its first maximum; two lanes meet on (larger value,
// then smaller index), which is symmetric: every lane of the xor tree ends with the row's first maximum.
__global__ __launch_bounds__(256) void align_rows_kernel(const float* attn, long ld_row, long ld_head, long ld_batch,
                                                         const int64_t* plens, const int64_t* mlens, int H, int Tm, int Tp, long rows,
                                                         int* amax, float* rmax) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int t = (int)(row % Tm), h = (int)((row / Tm) % H), b = (int)(row / ((long)Tm * H));
    const int T = align_len(mlens, b, Tm), N = align_len(plens, b, Tp);
    float v = -INFINITY;
    int idx = INT_MAX;
    const bool on = t < T && N > 0;
    if (on) {
        const float* ar = attn + b * ld_batch + h * ld_head + t * ld_row;
        for (int n0 = 0; n0 < N; n0 += 256) {
            float x[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {                  // four loads in flight per lane
                const int n = n0 + j * 64 + lane;
                x[j] = n < N ? ar[n] : -INFINITY;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x[j] > v) { v = x[j]; idx = n0 + j * 64 + lane; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(v, o, 64);
            const int oi = __shfl_xor(idx, o, 64);
            if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
        }
        if (idx >= N) { idx = 0; v = 0.f; }                // a row without one value above -inf (no softmax output is)
    }
    if (lane == 0) {
        amax[row] = on ? idx : 0;
        rmax[row] = on ? v : 0.f;
    }
}

// focus[plane] = (sum_{t < T_b} rmax[plane][t]) / T_b: one wave per (b, h) plane, lane j taking t = j, j + 64, ..., then the tree
__global__ __launch_bounds__(256) void align_focus_kernel(const float* rmax, const int64_t* plens, const int64_t* mlens, int H, int Tm,
                                                          int Tp, int planes, float* focus) {
    const int lane = threadIdx.x & 63;
    const int plane = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (plane >= planes) return;
    const int b = plane / H;
    const int T = align_len(mlens, b, Tm), N = align_len(plens, b, Tp);
    float acc = 0.f;
    if (N > 0)
        for (int t = lane; t < T; t += 64) acc += rmax[(long)plane * Tm + t];
    acc = wave_sum(acc);
    if (lane == 0) focus[plane] = (T > 0 && N > 0) ? acc / (float)T : 0.f;
}

// ---------------------------------------------------------------- head choice
// focus is (L, B, H); candidate c = layer * H + head; the first maximum wins (a later candidate replaces only on `>`)
__global__ __launch_bounds__(256) void align_select_kernel(const float* focus, const int64_t* plens, const int64_t* mlens, int L, int B,
                                                           int H, int mode, int fixed, int64_t* choice, int64_t* pairs) {
    __shared__ float tot[ALIGN_SELECT_MAX];
    const int C = L * H;
    if (mode == TTTS_ALIGN_SELECT_BATCH) {
        for (int c = threadIdx.x; c < C; c += 256) {
            const int l = c / H, h = c % H;
            float s = 0.f;
            for (int b = 0; b < B; ++b)                     // in b order, over the utterances that have a map at all
                if (mlens[b] > 0 && plens[b] > 0) s += focus[((long)l * B + b) * H + h];
            tot[c] = s;
        }
        __syncthreads();
    }
    for (int b = threadIdx.x; b < B; b += 256) {
        int best = fixed;
        if (mode != TTTS_ALIGN_SELECT_FIXED) {
            float bv = 0.f;
            best = 0;
            for (int c = 0; c < C; ++c) {
                const float f = mode == TTTS_ALIGN_SELECT_BATCH ? tot[c] : focus[((long)(c / H) * B + b) * H + c % H];
                if (c == 0 || f > bv) { bv = f; best = c; }
            }
        }
        choice[b] = best;
        if (pairs) {
            pairs[2 * b] = best / H;
            pairs[2 * b + 1] = best % H;
        }
    }
}

__device__ __forceinline__ int align_choice(const int64_t* choice, int b, int C) {
    const long c = choice[b];
    return (int)(c < 0 ? 0 : c >= C ? C - 1 : c);          // (a choice this library did not write stays inside the maps)
}

// ---------------------------------------------------------------- argmax durations
// one workgroup per utterance: integer counts in LDS (order-free), then the whole (Tp) row is written, zeros from N_b on
__global__ __launch_bounds__(256) void align_count_kernel(const int* amax, const int64_t* choice, const int64_t* plens,
                                                          const int64_t* mlens, int L, int B, int H, int Tm, int Tp, int64_t* dur,
                                                          uint8_t* valid) {
    __shared__ int cnt[ALIGN_COUNT_TP];
    const int b = blockIdx.x;
    const int T = align_len(mlens, b, Tm), N = align_len(plens, b, Tp);
    for (int n = threadIdx.x; n < N; n += 256) cnt[n] = 0;
    __syncthreads();
    const int c = align_choice(choice, b, L * H);
    const int* ar = amax + (((long)(c / H) * B + b) * H + c % H) * Tm;
    for (int t = threadIdx.x; t < T; t += 256) {
        const int a = ar[t];
        if (a >= 0 && a < N) atomicAdd(&cnt[a], 1);
    }
    __syncthreads();
    for (int n = threadIdx.x; n < Tp; n += 256) dur[(long)b * Tp + n] = n < N ? cnt[n] : 0;
    if (threadIdx.x == 0 && valid) valid[b] = T > 0 && N > 0;
}

// ---------------------------------------------------------------- monotonic alignment search
// One wave per utterance; lane j holds the K = 1 << LOGK neighbouring phonemes n = j K .. j K + K - 1, so a step of the recurrence
//   Q[t][n] = s[t][n] + max(Q[t-1][n], Q[t-1][n-1]),  s = logf(fmaxf(A, 1e-30f)),
// needs ONE value from another lane (lane j - 1's last Q) and no barrier.  Cells from which (T-1, N-1) cannot be reached, or that
// (0, 0) cannot reach, hold -inf; the row before the first holds 0 at n = 0, which makes Q[0][0] = s[0][0].  Stay wins a tie.
// MAS_PF rows of the map are in flight ahead of the row being added (a row's loads do not depend on the chain).  The stay bits of
// row t go to K 64-bit words (word k, bit j = phoneme j K + k), lane k storing word k; after the last row the wave reads them
// back MAS_ROWS rows at a time through LDS and walks from (T-1, N-1) to (0, 0), every lane alike, lane 0 writing the run lengths.
template <int LOGK>
__global__ __launch_bounds__(64) void align_mas_kernel(AlignMaps maps, int L, long ld_row, long ld_head, long ld_batch,
                                                       const int64_t* choice, const int64_t* plens, const int64_t* mlens, int B, int H,
                                                       int Tm, int Tp, unsigned long long* ws, int64_t* dur, uint8_t* valid) {
    constexpr int K = 1 << LOGK;
    __shared__ unsigned long long bits[MAS_ROWS * K];
    const int lane = threadIdx.x, b = blockIdx.x;
    const int T = align_len(mlens, b, Tm), N = align_len(plens, b, Tp);
    int64_t* drow = dur + (long)b * Tp;
    const bool ok = N > 0 && T >= N;
    if (lane == 0) valid[b] = ok;
    for (int n = (ok ? N : 0) + lane; n < Tp; n += 64) drow[n] = 0;
    if (!ok) return;
    const int c = align_choice(choice, b, L * H);
    const float* plane = maps.p[c / H] + b * ld_batch + (c % H) * ld_head;
    unsigned long long* wsb = ws + (long)b * Tm * K;
    const int n_first = lane * K;

    float q[K], buf[MAS_PF][K];
#pragma unroll
    for (int k = 0; k < K; ++k) q[k] = (n_first + k == 0) ? 0.f : -INFINITY;
    // loads past the utterance are clamped onto its last frame / phoneme (never acted on): no load sits behind a branch
    long col[K];
#pragma unroll
    for (int k = 0; k < K; ++k) col[k] = n_first + k < N ? n_first + k : N - 1;
#pragma unroll
    for (int j = 0; j < MAS_PF; ++j)
#pragma unroll
        for (int k = 0; k < K; ++k) buf[j][k] = plane[(long)(j < T ? j : T - 1) * ld_row + col[k]];
    // The ring's first fill lands before the loop: the compiler counts a wait from the worst of the paths into a point, and with
    // these loads still in flight at the loop's head it would drain the ring at the first of every MAS_PF rows.  (The builtin,
    // not inline assembly: the pass that places the waits has to see it.)  vmcnt(0), the other counters untouched.
    __builtin_amdgcn_s_waitcnt(0x0F70);

    for (int t0 = 0; t0 < T; t0 += MAS_PF) {
#pragma unroll
        for (int j = 0; j < MAS_PF; ++j) {
            const int t = t0 + j;
            if (t < T) {                                    // (uniform)
                float left = __shfl_up(q[K - 1], 1, 64);
                if (lane == 0) left = -INFINITY;
                const int lo = N - T + t;                   // phonemes below lo can no longer reach the end
                unsigned long long word = 0;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const int n = n_first + k;
                    const float keep = q[k];
                    const bool stay = keep >= left;
                    const float best = stay ? keep : left;
                    const bool in = n <= t && n >= lo && n < N;
                    const float sc = logf(fmaxf(buf[j][k], 1e-30f)) + best;
                    q[k] = in ? sc : -INFINITY;
                    left = keep;
                    const unsigned long long m = __ballot(stay);
                    if (lane == k) word = m;
                }
                if (lane < K) wsb[(long)t * K + lane] = word;
            }
            const long tn = t + MAS_PF < T ? t + MAS_PF : T - 1;
#pragma unroll
            for (int k = 0; k < K; ++k) buf[j][k] = plane[tn * ld_row + col[k]];
        }
    }
    // NOT a redundant barrier of a one-wave block: lanes 0 .. K-1 stored the stay words to global memory and OTHER lanes read them
    // back below.  What orders the two is the workgroup-scope fence __syncthreads() carries (the wave waits for its stores,
    // s_waitcnt vmcnt(0), before it goes on); the s_barrier itself does nothing for one wave.
    __syncthreads();

    int n = N - 1, run = 0;
    for (int t_hi = T - 1; t_hi >= 0; t_hi -= MAS_ROWS) {
        const int t_lo = t_hi - (MAS_ROWS - 1) > 0 ? t_hi - (MAS_ROWS - 1) : 0;
        const int words = (t_hi - t_lo + 1) * K;
        for (int i = lane; i < words; i += 64) bits[i] = wsb[(long)t_lo * K + i];
        __syncthreads();
        for (int t = t_hi; t >= t_lo; --t) {
            const bool stay = (bits[(t - t_lo) * K + (n & (K - 1))] >> (n >> LOGK)) & 1u;
            ++run;
            if (!stay && n > 0) {                           // frame t is the first of phoneme n
                if (lane == 0) drow[n] = run;
                --n;
                run = 0;
            }
        }
        __syncthreads();
    }
    if (lane == 0) drow[n] = run;                           // n == 0: the band leaves the path nowhere else to be at t = 0
}

static inline int mas_logk(int Tp) {
    int logk = 0;
    while ((64L << logk) < Tp) ++logk;
    return logk;
}

static int align_check(const char* name, const void* plens, const void* mlens, int B, int H, int Tm, int Tp) {
    TTTS_REQUIRE(plens && mlens, "%s: null pointer", name);
    TTTS_REQUIRE(B > 0 && H > 0 && Tm > 0 && Tp > 0, "%s: sizes must be positive (B %d, H %d, Tm %d, Tp %d)", name, B, H, Tm, Tp);
    return TTTS_OK;
}
static int align_check_layers(const char* name, int L) {
    TTTS_REQUIRE(L > 0, "%s: sizes must be positive (L %d)", name, L);
    TTTS_REQUIRE(L <= ALIGN_MAX_MAPS, "%s: at most %d maps (L %d)", name, ALIGN_MAX_MAPS, L);
    return TTTS_OK;
}
static int align_check_strides(const char* name, int64_t ld_row, int64_t ld_head, int64_t ld_batch, int Tp) {
    TTTS_REQUIRE(ld_row >= Tp, "%s: the row stride must be >= Tp (ld_row %lld, Tp %d)", name, (long long)ld_row, Tp);
    TTTS_REQUIRE(ld_head >= 0 && ld_batch >= 0, "%s: strides must not be negative (ld_head %lld, ld_batch %lld)", name,
                 (long long)ld_head, (long long)ld_batch);
    return TTTS_OK;
}

}  // namespace ttts

using namespace ttts;

extern "C" {

int ttts_alignment_rowstats(const float* attn, int64_t ld_row, int64_t ld_head, int64_t ld_batch, const int64_t* phoneme_lens,
                            const int64_t* melspec_lens, int B, int H, int Tm, int Tp, int layer, int L, int32_t* argmax,
                            float* rowmax, float* focus, void* stream) {
    const char* name = "alignment_rowstats";
    TTTS_REQUIRE(attn && argmax && rowmax && focus, "%s: null pointer", name);
    int rc = align_check(name, phoneme_lens, melspec_lens, B, H, Tm, Tp);
    if (rc) return rc;
    if ((rc = align_check_layers(name, L))) return rc;
    TTTS_REQUIRE(layer >= 0 && layer < L, "%s: layer %d is outside [0, L %d)", name, layer, L);
    if ((rc = align_check_strides(name, ld_row, ld_head, ld_batch, Tp))) return rc;
    const long rows = (long)B * H * Tm;
    TTTS_REQUIRE(rows < (1L << 31), "%s: grid too large (B*H*Tm %ld)", name, rows);
    hipLaunchKernelGGL(align_rows_kernel, dim3((unsigned)cdiv(rows, 4L)), dim3(256), 0, (hipStream_t)stream, attn, (long)ld_row,
                       (long)ld_head, (long)ld_batch, phoneme_lens, melspec_lens, H, Tm, Tp, rows, argmax + (long)layer * rows, rowmax);
    TTTS_LAUNCH_CHECK("align_rows_kernel");
    hipLaunchKernelGGL(align_focus_kernel, dim3((unsigned)cdiv((long)B * H, 4L)), dim3(256), 0, (hipStream_t)stream, rowmax,
                       phoneme_lens, melspec_lens, H, Tm, Tp, B * H, focus + (long)layer * B * H);
    TTTS_LAUNCH_CHECK("align_focus_kernel");
    return TTTS_OK;
}

int ttts_alignment_select(const float* focus, const int64_t* phoneme_lens, const int64_t* melspec_lens, int L, int B, int H, int mode,
                          int layer, int head, int64_t* choice, int64_t* choice_pairs, void* stream) {
    const char* name = "alignment_select";
    TTTS_REQUIRE(focus && phoneme_lens && melspec_lens && choice, "%s: null pointer", name);
    TTTS_REQUIRE(B > 0 && H > 0, "%s: sizes must be positive (B %d, H %d)", name, B, H);
    int rc = align_check_layers(name, L);
    if (rc) return rc;
    TTTS_REQUIRE(mode == TTTS_ALIGN_SELECT_UTTERANCE || mode == TTTS_ALIGN_SELECT_BATCH || mode == TTTS_ALIGN_SELECT_FIXED,
                 "%s: unknown mode %d", name, mode);
    if (mode == TTTS_ALIGN_SELECT_FIXED)
        TTTS_REQUIRE(layer >= 0 && layer < L && head >= 0 && head < H, "%s: (layer %d, head %d) is outside (L %d, H %d)", name, layer,
                     head, L, H);
    TTTS_REQUIRE((long)L * H <= ALIGN_SELECT_MAX, "%s: at most %d (layer, head) pairs (L*H %ld)", name, ALIGN_SELECT_MAX, (long)L * H);
    hipLaunchKernelGGL(align_select_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, focus, phoneme_lens, melspec_lens, L, B, H, mode,
                       mode == TTTS_ALIGN_SELECT_FIXED ? layer * H + head : 0, choice, choice_pairs);
    TTTS_LAUNCH_CHECK("align_select_kernel");
    return TTTS_OK;
}

int ttts_alignment_durations_argmax(const int32_t* argmax, const int64_t* choice, const int64_t* phoneme_lens,
                                    const int64_t* melspec_lens, int L, int B, int H, int Tm, int Tp, int64_t* durations, uint8_t* valid,
                                    void* stream) {
    const char* name = "alignment_durations_argmax";
    TTTS_REQUIRE(argmax && choice && durations, "%s: null pointer", name);
    int rc = align_check(name, phoneme_lens, melspec_lens, B, H, Tm, Tp);
    if (rc) return rc;
    if ((rc = align_check_layers(name, L))) return rc;
    TTTS_REQUIRE(Tp <= ALIGN_COUNT_TP, "%s: Tp %d is above the %d phonemes the counters hold", name, Tp, ALIGN_COUNT_TP);
    hipLaunchKernelGGL(align_count_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, argmax, choice, phoneme_lens,
                       melspec_lens, L, B, H, Tm, Tp, durations, valid);
    TTTS_LAUNCH_CHECK("align_count_kernel");
    return TTTS_OK;
}

size_t ttts_alignment_mas_workspace_bytes(int B, int Tm, int Tp) {
    if (B <= 0 || Tm <= 0 || Tp <= 0) return 0;
    return (size_t)B * (size_t)Tm * ((size_t)8 << mas_logk(Tp));
}

int ttts_alignment_mas(const float* const* maps, int L, int64_t ld_row, int64_t ld_head, int64_t ld_batch, const int64_t* choice,
                       const int64_t* phoneme_lens, const int64_t* melspec_lens, int B, int H, int Tm, int Tp, void* ws,
                       size_t ws_bytes, int64_t* durations, uint8_t* valid, void* stream) {
    const char* name = "alignment_mas";
    TTTS_REQUIRE(maps && choice && ws && durations && valid, "%s: null pointer", name);
    int rc = align_check(name, phoneme_lens, melspec_lens, B, H, Tm, Tp);
    if (rc) return rc;
    if ((rc = align_check_layers(name, L))) return rc;
    AlignMaps m;
    for (int i = 0; i < ALIGN_MAX_MAPS; ++i) {
        TTTS_REQUIRE(i >= L || maps[i], "%s: null pointer (map %d)", name, i);
        m.p[i] = maps[i < L ? i : 0];
    }
    if ((rc = align_check_strides(name, ld_row, ld_head, ld_batch, Tp))) return rc;
    TTTS_REQUIRE(Tp <= ALIGN_MAS_TP, "%s: Tp %d is above the %d phonemes one wave holds", name, Tp, ALIGN_MAS_TP);
    TTTS_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "%s: the workspace must be 8-byte aligned", name);
    const size_t need = ttts_alignment_mas_workspace_bytes(B, Tm, Tp);
    TTTS_REQUIRE(ws_bytes >= need, "%s: workspace too small (%zu bytes, %zu needed)", name, ws_bytes, need);
    const dim3 grid((unsigned)B), block(64);
    unsigned long long* w = static_cast<unsigned long long*>(ws);
#define TTTS_MAS_LAUNCH(LOGK)                                                                                                     \
    hipLaunchKernelGGL(align_mas_kernel<LOGK>, grid, block, 0, (hipStream_t)stream, m, L, (long)ld_row, (long)ld_head, (long)ld_batch, \
                       choice, phoneme_lens, melspec_lens, B, H, Tm, Tp, w, durations, valid)
    switch (mas_logk(Tp)) {
        case 0: TTTS_MAS_LAUNCH(0); break;
        case 1: TTTS_MAS_LAUNCH(1); break;
        case 2: TTTS_MAS_LAUNCH(2); break;
        case 3: TTTS_MAS_LAUNCH(3); break;
        default: TTTS_MAS_LAUNCH(4); break;
    }
#undef TTTS_MAS_LAUNCH
    TTTS_LAUNCH_CHECK("align_mas_kernel");
    return TTTS_OK;
}

}  // extern "C"
