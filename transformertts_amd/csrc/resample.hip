// Band-limited resampler (gfx950): a ragged batch of waveforms from one rate to another in one launch, windowed-sinc (Kaiser)
// interpolation in polyphase form (the family of resampy's kaiser_best and torchaudio's sinc_interp_kaiser, restated).
//   rates       L = new / gcd, M = orig / gcd, L != M.  Output j of utterance b sits at input time j M / L:
//               q = floor(j M / L), phase r = j mod L (the fraction is ((r M) mod L) / L).
//   sum         y[b, j] = sum_{k = 0 .. K-1} h[r][k] x[b, q - W + k], W = K/2 - 1, ascending k from 0.f with fmaf: the bits of a
//               sample depend on neither the grid, the batch nor the call.  x counts as 0 outside [0, len_b) and such a sample
//               is never loaded.
//   weights     from the host (fp64, rounded to fp32 once), tap-major: table[k L + r].  No sinf, no Bessel function here.
//   lengths     len_b = clamp(wave_lens[b], 0, Nmax), out_len_b = ceil(len_b L / M), Nout = ceil(Nmax L / M); outputs from
//               out_len_b to Nout are zeros.  j M is formed in 64 bits once per workgroup; inside a tile 32 bits hold everything.
// A workgroup of 256 threads owns RESAMPLE_TILE consecutive outputs of one utterance.  It stages the input span of its tile
// in LDS (the zeros of the utterance's two ends applied there), then every thread carries up to RESAMPLE_SHARE outputs of the
// SAME phase -- u, u + S L, u + 2 S L, ... with S L about a quarter of the tile -- so that one weight, read coalesced from the
// L2-resident table (neighbouring lanes are neighbouring phases), feeds RESAMPLE_SHARE FMAs whose inputs come from LDS at
// distances of S M floats.  RESAMPLE_SHARE = 1 is the plain form (one output per thread and pass): every FMA then costs a
// 256-byte weight request per wave, which is what bounds it (DESIGN.md 23 has both numbers).
#include "ttts_common.h"

namespace ttts {

constexpr int RESAMPLE_TILE = 1024;      // outputs a workgroup owns
constexpr int RESAMPLE_THREADS = 256;
#ifndef TTTS_RESAMPLE_SHARE
#define TTTS_RESAMPLE_SHARE 4            // outputs of one phase per thread (1: the plain form, for measurements)
#endif
constexpr int RESAMPLE_SHARE = TTTS_RESAMPLE_SHARE;
// what keeps a tile's span (at most (TILE - 1) * 8 + 2 + 1280 floats = 37 KB of LDS) and the table (L K floats) small
constexpr int RESAMPLE_MAX_L = 1024, RESAMPLE_MAX_K = 1280, RESAMPLE_MAX_RATIO = 8;

__host__ __device__ static inline long resample_span_floats(int L, int M, int K) {
    return ((long)(RESAMPLE_TILE - 1) * M) / L + 2 + K;
}

// R outputs of one phase: xp[k + m step] are their inputs, wp[k L] the weights they share
template <int R>
__device__ __forceinline__ void resample_item(const float* __restrict__ wp, const float* xp, int K, int L, int step,
                                              float* __restrict__ op, int stride_e) {
    float acc[R];
#pragma unroll
    for (int m = 0; m < R; ++m) acc[m] = 0.f;
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
        const float w = wp[(long)k * L];
#pragma unroll
        for (int m = 0; m < R; ++m) acc[m] = fmaf(w, xp[k + m * step], acc[m]);
    }
#pragma unroll
    for (int m = 0; m < R; ++m) op[(long)m * stride_e] = acc[m];
}

template <int RMAX>
__global__ __launch_bounds__(RESAMPLE_THREADS) void resample_kernel(const float* __restrict__ wave, long ld_batch,
                                                                    const int64_t* __restrict__ wave_lens, int Nmax, int L, int M,
                                                                    int K, long Nout, const float* __restrict__ table,
                                                                    float* __restrict__ out, long ld_out,
                                                                    int64_t* __restrict__ out_lens) {
    extern __shared__ float xs[];
    const int tid = threadIdx.x, b = blockIdx.y;
    const long j0 = (long)blockIdx.x * RESAMPLE_TILE;
    const long len64 = wave_lens[b];
    const long len = len64 < 0 ? 0 : len64 > Nmax ? Nmax : len64;
    const long out_len = (len * L + M - 1) / M;                      // <= Nout
    if (blockIdx.x == 0 && tid == 0) out_lens[b] = out_len;
    float* ob = out + (long)b * ld_out + j0;
    const int width = (int)(Nout - j0 < RESAMPLE_TILE ? Nout - j0 : RESAMPLE_TILE);     // outputs of this tile inside the row
    const long left = out_len - j0;
    const int limit = (int)(left < 0 ? 0 : left > width ? width : left);                // the first `limit` of them are computed
    for (int e = limit + tid; e < width; e += RESAMPLE_THREADS) ob[e] = 0.f;
    if (limit == 0) return;                                          // (uniform) wholly behind out_len: only its zeros

    // the span: inputs q0 - W .. q(limit - 1) - W + K - 1, xs[i] = x[q0 - W + i]
    const int W = K / 2 - 1;
    const long t0 = j0 * M;                                          // up to 2^33 * 2^13: 64 bits
    const long q0 = t0 / L;
    const int p0 = (int)(t0 - q0 * L);                               // (j0 M) mod L; p0 + e M < 2^24 for every e of the tile
    const int r0 = (int)(j0 % L);
    const int span = (p0 + (limit - 1) * M) / L + K;                 // <= resample_span_floats
    const long first = q0 - W;
    const float* wb = wave + (long)b * ld_batch;
    for (int i = tid; i < span; i += RESAMPLE_THREADS) {
        const long g = first + i;
        xs[i] = g >= 0 && g < len ? wb[g] : 0.f;
    }
    __syncthreads();

    // thread u carries outputs u + m stride_e, m < RMAX: stride_e = S L is a multiple of L (one phase, inputs S M apart) and
    // RMAX stride_e covers the tile
    const int periods = (RESAMPLE_TILE + L - 1) / L;
    const int S = (periods + RMAX - 1) / RMAX;
    const int stride_e = S * L, step = S * M;
    const int items = stride_e < limit ? stride_e : limit;
    for (int u = tid; u < items; u += RESAMPLE_THREADS) {
        int r = r0 + u % L;
        r = r >= L ? r - L : r;
        const float* wp = table + r;
        const float* xp = xs + (p0 + u * M) / L;
        float* op = ob + u;
        if constexpr (RMAX == 1) {
            resample_item<1>(wp, xp, K, L, step, op, stride_e);
        } else {
            static_assert(RMAX == 4, "the switch below lists the counts of RMAX = 4");
            switch (1 + (limit - 1 - u) / stride_e) {                // outputs of this thread inside the limit (>= 1)
                case 1: resample_item<1>(wp, xp, K, L, step, op, stride_e); break;
                case 2: resample_item<2>(wp, xp, K, L, step, op, stride_e); break;
                case 3: resample_item<3>(wp, xp, K, L, step, op, stride_e); break;
                default: resample_item<4>(wp, xp, K, L, step, op, stride_e); break;
            }
        }
    }
}

static long resample_gcd(long a, long b) {
    while (b) {
        const long t = a % b;
        a = b;
        b = t;
    }
    return a;
}

}  // namespace ttts

using namespace ttts;

extern "C" {

size_t ttts_resample_table_bytes(int L, int K) {
    if (L < 1 || K < 4 || (K & 1)) return 0;
    return (size_t)L * (size_t)K * 4;
}

int ttts_resample_table_check(const void* host_table, size_t bytes, int L, int M, int K) {
    const char* name = "resample_table_check";
    TTTS_REQUIRE(host_table, "%s: null pointer", name);
    TTTS_REQUIRE(L >= 1 && M >= 1, "%s: rates must be positive (L %d, M %d)", name, L, M);
    TTTS_REQUIRE(K >= 4 && (K & 1) == 0, "%s: K must be even and at least 4, got %d", name, K);
    TTTS_REQUIRE(resample_gcd(L, M) == 1, "%s: L and M must be coprime (L %d, M %d, gcd %ld)", name, L, M, resample_gcd(L, M));
    TTTS_REQUIRE((reinterpret_cast<uintptr_t>(host_table) & 3) == 0, "%s: the table must be 4-byte aligned", name);
    const size_t need = ttts_resample_table_bytes(L, K);
    TTTS_REQUIRE(bytes == need, "%s: the table holds %zu bytes, %zu expected", name, bytes, need);
    const float* t = static_cast<const float*>(host_table);
    for (size_t i = 0; i < (size_t)L * K; ++i)
        TTTS_REQUIRE(t[i] - t[i] == 0.f, "%s: weight %zu (tap %zu, phase %zu) is not finite", name, i, i / L, i % L);
    return TTTS_OK;
}

int ttts_resample_tile(void) { return RESAMPLE_TILE; }

int ttts_resample(const float* wave, int64_t ld_batch, const int64_t* wave_lens, int B, int Nmax, int L, int M, int K,
                  const float* table, float* out, int64_t ld_out, int64_t* out_lens, void* stream) {
    const char* name = "resample";
    TTTS_REQUIRE(wave && wave_lens && table && out && out_lens, "%s: null pointer", name);
    TTTS_REQUIRE(B >= 1 && B <= 65535, "%s: B must be in [1, 65535] (one grid row per utterance), got %d", name, B);
    TTTS_REQUIRE(Nmax >= 1 && Nmax <= (1 << 30), "%s: Nmax must be in [1, 2^30] samples per utterance, got %d", name, Nmax);
    TTTS_REQUIRE(L >= 1 && M >= 1, "%s: rates must be positive (L %d, M %d)", name, L, M);
    TTTS_REQUIRE(L != M, "%s: L == M (%d) is the identity: nothing to launch", name, L);
    TTTS_REQUIRE(L <= RESAMPLE_MAX_L, "%s: at most %d phases, got L %d", name, RESAMPLE_MAX_L, L);
    TTTS_REQUIRE((long)L <= (long)RESAMPLE_MAX_RATIO * M && (long)M <= (long)RESAMPLE_MAX_RATIO * L,
                 "%s: the rates may differ by a factor of %d at the most (L %d, M %d)", name, RESAMPLE_MAX_RATIO, L, M);
    TTTS_REQUIRE(K >= 4 && (K & 1) == 0, "%s: K must be even and at least 4, got %d", name, K);
    TTTS_REQUIRE(K <= RESAMPLE_MAX_K, "%s: at most %d taps, got K %d", name, RESAMPLE_MAX_K, K);
    const long Nout = ((long)Nmax * L + M - 1) / M;
    TTTS_REQUIRE(ld_batch >= Nmax || (B == 1 && ld_batch >= 0), "%s: the batch stride must be >= Nmax (ld_batch %lld, Nmax %d)", name,
                 (long long)ld_batch, Nmax);
    TTTS_REQUIRE(ld_out >= Nout || (B == 1 && ld_out >= 0), "%s: the output stride must be >= Nout (ld_out %lld, Nout %ld)", name,
                 (long long)ld_out, Nout);
    TTTS_REQUIRE(((reinterpret_cast<uintptr_t>(wave) | reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(out)) & 3) == 0,
                 "%s: wave, table and out must be 4-byte aligned", name);
    TTTS_REQUIRE(((reinterpret_cast<uintptr_t>(wave_lens) | reinterpret_cast<uintptr_t>(out_lens)) & 7) == 0,
                 "%s: wave_lens and out_lens must be 8-byte aligned", name);
    const dim3 grid((unsigned)((Nout + RESAMPLE_TILE - 1) / RESAMPLE_TILE), (unsigned)B);     // <= 2^23 tiles
    hipLaunchKernelGGL(resample_kernel<RESAMPLE_SHARE>, grid, dim3(RESAMPLE_THREADS), (size_t)resample_span_floats(L, M, K) * 4,
                       (hipStream_t)stream, wave, (long)ld_batch, wave_lens, Nmax, L, M, K, Nout, table, out, (long)ld_out, out_lens);
    TTTS_LAUNCH_CHECK("resample_kernel");
    return TTTS_OK;
}

}  // extern "C"
