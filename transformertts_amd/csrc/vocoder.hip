// Griffin-Lim vocoder (gfx950): a ragged batch of (normalised) log-mels to waveforms, the way back from audio.hip on the same
// tables.  Three kernels; a call of n_iter iterations is one magnitude launch, n_iter + 1 inverse and n_iter forward launches.
//   magnitude   x = mel[b, t, :] (with statistics x * (std + 1e-8) + mean), m[f] = expf(x[f]), mag[k] = max(sum_f pinv[k, f] m[f],
//               floor), f ascending, pinv the (bins, n_mels) pseudo-inverse of the mel basis.  frames_b = melspec_lens[b] clamped
//               to [0, Tmax]; a row is vocodable iff (frames_b - 1) hop > n_fft/2 (the front end could reflect what comes back),
//               otherwise its effective frames are 0.  The kernel writes the effective frames; the transforms read only those.
//   inverse     x_t = irfft(spec[b, t], n_fft) (the imaginary parts of bins 0 and n_fft/2 ignored, 1/n_fft applied here);
//               y[g'] = sum_t w[n] x_t[n], env[g'] = sum_t w[n]^2 over the frames t < frames_b with g' = t hop + n, both in
//               ascending t; wave[b, g] = env > FLT_MIN ? y / env : y at g' = g + n_fft/2 for g < wave_lens[b] =
//               (frames_b - 1) hop, zeros from there to Nmax = (Tmax - 1) hop.
//   forward     reb = STFT(wave) as audio.hip frames, reflects, windows and transforms it; without `mag` reb is stored (the complex
//               STFT); with it t = reb - momentum / (1 + momentum) prev, prev <- reb, spec = mag * (|t|^2 > 1e-30 ? t / |t| : 1).
// The inverse is a gather: a workgroup of audio_threads(n_fft) threads owns VOCODER_SPAN consecutive output samples in LDS and
// walks the frames that touch them in ascending t (the ceil(n_fft / hop) - 1 frames that reach in from the left included:
// they are recomputed).  Per frame: the bins are folded into the packed M = n_fft/2 point spectrum Z[k] = E[k] + i O[k], E =
// (X[k] + conj X[M-k]) / 2, O = (X[k] - conj X[M-k]) / 2 conj(w^k) -- the inverse of audio_unpack_real, on the same w^k table
// conjugated -- then fft_lds<M, FFT_INVERSE>, then x[2m] = Re z[m], x[2m+1] = Im z[m] times the window values held in registers
// are added to the span.  The FFT's barriers lie between one frame's adds and the next one's, so a sample's sum has one order
// whatever the grid: no atomics, the same bits on every call and for a row alone or in a batch.
#include "fft_lds.h"
#include "audio_common.h"
#include "ttts_common.h"

#include <float.h>
#include <math.h>

namespace ttts {

#ifndef TTTS_VOCODER_SPAN_MULT
#define TTTS_VOCODER_SPAN_MULT 2
#endif
constexpr int VOCODER_SPAN_MULT = TTTS_VOCODER_SPAN_MULT;   // output samples a workgroup owns, in units of n_fft (audio.py SPAN_MULT)
constexpr int VOCODER_FRAMES = 8;                           // frames a forward / magnitude workgroup carries
constexpr int VOCODER_MAG_THREADS = 256;

// frames of a row as the transforms take them: the array's value clamped to [0, Tmax]
__device__ __forceinline__ int vocoder_frames(const int64_t* __restrict__ frames, int b, int Tmax) {
    const long f = frames[b];
    return (int)(f < 0 ? 0 : f > Tmax ? Tmax : f);
}

__global__ __launch_bounds__(VOCODER_MAG_THREADS) void mel_to_magnitude_kernel(
    const float* __restrict__ mel, long ld_row, long ld_batch, const int64_t* __restrict__ mel_lens, int Tmax, int bins, int hop,
    int n_mels, const float* __restrict__ pinv, const float* __restrict__ mean_std, float floor_val, float* __restrict__ mag,
    int64_t* __restrict__ frames_out) {
    __shared__ float m[VOCODER_FRAMES][AUDIO_MAX_MELS];
    const int tid = threadIdx.x, b = blockIdx.y, t0 = blockIdx.x * VOCODER_FRAMES;
    int frames = vocoder_frames(mel_lens, b, Tmax);
    if ((long)(frames - 1) * hop <= bins - 1) frames = 0;        // the front end could not reflect (frames - 1) hop samples
    if (blockIdx.x == 0 && tid == 0) frames_out[b] = frames;
    const int t1 = t0 + VOCODER_FRAMES < Tmax ? t0 + VOCODER_FRAMES : Tmax;
    const int tv = t1 < frames ? t1 : frames;                        // rows t0 .. tv - 1 are computed, tv .. t1 - 1 are zeros
    float* ob = mag + (long)b * Tmax * bins;
    {
        const int z0 = t0 > tv ? t0 : tv;
        float* zp = ob + (long)z0 * bins;
        for (long e = tid; e < (long)(t1 - z0) * bins; e += VOCODER_MAG_THREADS) zp[e] = 0.f;
    }
    if (t0 >= tv) return;                                            // (uniform)
    const int rows = tv - t0;
    const float sdev = mean_std != nullptr ? mean_std[1] + 1e-8f : 1.f, mean = mean_std != nullptr ? mean_std[0] : 0.f;
    const float* mb = mel + (long)b * ld_batch;
    for (int e = tid; e < rows * n_mels; e += VOCODER_MAG_THREADS) {
        const int r = e / n_mels, f = e - r * n_mels;
        float x = mb[(long)(t0 + r) * ld_row + f];
        if (mean_std != nullptr) x = x * sdev + mean;
        m[r][f] = expf(x);
    }
    __syncthreads();
    for (int k = tid; k < bins; k += VOCODER_MAG_THREADS) {
        const float* pk = pinv + (long)k * n_mels;
        float acc[VOCODER_FRAMES];
#pragma unroll
        for (int r = 0; r < VOCODER_FRAMES; ++r) acc[r] = 0.f;
        for (int f = 0; f < n_mels; ++f) {
            const float p = pk[f];
#pragma unroll
            for (int r = 0; r < VOCODER_FRAMES; ++r) acc[r] = fmaf(p, m[r][f], acc[r]);   // (rows past `rows` hold stale values, not stored)
        }
#pragma unroll
        for (int r = 0; r < VOCODER_FRAMES; ++r)
            if (r < rows) ob[(long)(t0 + r) * bins + k] = fmaxf(acc[r], floor_val);
    }
}

template <int N>
__global__ __launch_bounds__(audio_threads(N)) void istft_kernel(const float* __restrict__ spec, const int64_t* __restrict__ frames_in,
                                                                 int Tmax, int hop, const float* __restrict__ tables,
                                                                 float* __restrict__ wave, int64_t* __restrict__ wave_lens) {
    constexpr int M = N / 2, P = fft_padded_size(M), THREADS = audio_threads(N), PER_LANE = N / THREADS, SPAN = VOCODER_SPAN_MULT * N;
    __shared__ float a_re[P], a_im[P], b_re[P], b_im[P], w_re[P], w_im[P], pw[2 * (M / 2 + 1)], acc[SPAN];
    const int lane = threadIdx.x, b = blockIdx.y, g0 = blockIdx.x * SPAN;    // g0 < Nmax <= 2^30
    const int Nmax = (Tmax - 1) * hop;
    const int frames = vocoder_frames(frames_in, b, Tmax);
    const int len = frames > 0 ? (frames - 1) * hop : 0;
    if (blockIdx.x == 0 && lane == 0) wave_lens[b] = len;
    float* ob = wave + (long)b * Nmax;
    const int g1 = g0 + SPAN < Nmax ? g0 + SPAN : Nmax;              // this workgroup stores samples g0 .. g1 - 1
    const int gv = g1 < len ? g1 : len;                              // g0 .. gv - 1 are computed, the rest are zeros
    for (int g = (g0 > gv ? g0 : gv) + lane; g < g1; g += THREADS) ob[g] = 0.f;
    if (g0 >= gv) return;                                            // (uniform)

    const AudioTables tb = audio_tables(N, 0, 0);
    float* pw_re = pw;
    float* pw_im = pw + M / 2 + 1;
    audio_stage_roots<N>(tables, tb, w_re, w_im, pw_re, lane);
    float win[PER_LANE];
    audio_load_window<N>(tables, tb, win, lane);
    for (int e = lane; e < SPAN; e += THREADS) acc[e] = 0.f;
    const float* z_re = fft_result_in_second(M) ? b_re : a_re;
    const float* z_im = fft_result_in_second(M) ? b_im : a_im;
    // in the padded coordinate g' = g + M the span is [s0, s0 + SPAN); frame t covers [t hop, t hop + N)
    const int s0 = g0 + M;
    const int t_lo = s0 - N < 0 ? 0 : (s0 - N) / hop + 1;            // the first t with t hop + N > s0
    int t_hi = (s0 + (gv - g0) + hop - 1) / hop;                     // the first t with t hop >= s0 + (gv - g0)
    t_hi = t_hi < frames ? t_hi : frames;
    const float2* sb = reinterpret_cast<const float2*>(spec) + (long)b * Tmax * (M + 1);
    constexpr float inv_n = 1.0f / (float)N;

    for (int t = t_lo; t < t_hi; ++t) {
        const float2* row = sb + (long)t * (M + 1);
        for (int k = lane; k <= M / 2; k += THREADS) {
            const int mz = (M - k) & (M - 1);
            float2 xa = row[k], xb = row[M - k];
            if (k == 0) {                                            // bins 0 and n_fft/2 are real
                xa.y = 0.f;
                xb.y = 0.f;
            }
            const float er = xa.x + xb.x, ei = xa.y - xb.y;          // 2 E = X[k] + conj X[M-k]
            const float dr = xa.x - xb.x, di = xa.y + xb.y;          // 2 D = X[k] - conj X[M-k]
            const float wr = pw_re[k], wi = pw_im[k];
            const float pr = dr * wr + di * wi, pi = di * wr - dr * wi;         // 2 O = 2 D conj(w^k)
            a_re[fft_pad(k)] = er - pi;                              // 2 Z[k] = 2 (E + i O)
            a_im[fft_pad(k)] = ei + pr;
            if (mz != k) {                                           // 2 Z[M-k] = 2 (conj E + i conj O)
                a_re[fft_pad(mz)] = er + pi;
                a_im[fft_pad(mz)] = pr - ei;
            }
        }
        fft_lds<M, FFT_INVERSE, THREADS>(a_re, a_im, b_re, b_im, w_re, w_im, lane);
        const int off = t * hop - s0;                                // sample n of the frame is span element off + n
#pragma unroll
        for (int i = 0; i < PER_LANE; ++i) {
            const int n = lane + THREADS * i, e = off + n;
            const float v = ((n & 1) ? z_im : z_re)[fft_pad(n >> 1)] * inv_n;
            if (e >= 0 && e < SPAN) acc[e] += win[i] * v;
        }
        if (!fft_result_in_second(M)) __syncthreads();               // the next frame's spectrum overwrites what was just read
    }
    __syncthreads();
    // the envelope of sample g' = sum of w[g' - t hop]^2 over the frames that cover it, t ascending, from the table
    for (int g = g0 + lane; g < gv; g += THREADS) {
        const int gp = g + M;
        int ta = gp - N < 0 ? 0 : (gp - N) / hop + 1, tz = gp / hop + 1;
        tz = tz < frames ? tz : frames;
        float env = 0.f;
        for (int t = ta; t < tz; ++t) {
            const float w = tables[tb.window + gp - t * hop];
            env = fmaf(w, w, env);
        }
        const float y = acc[g - g0];
        ob[g] = env > FLT_MIN ? y / env : y;
    }
}

template <int N>
__global__ __launch_bounds__(audio_threads(N)) void stft_project_kernel(const float* __restrict__ wave, long ld_batch,
                                                                        const int64_t* __restrict__ wave_lens,
                                                                        const int64_t* __restrict__ frames_in, int Nmax, int hop, int Tmax,
                                                                        const float* __restrict__ tables, const float* __restrict__ mag,
                                                                        float* __restrict__ prev, float mom, float* __restrict__ spec,
                                                                        int64_t* __restrict__ frames_out) {
    constexpr int M = N / 2, P = fft_padded_size(M), THREADS = audio_threads(N), PER_LANE = N / THREADS;
    __shared__ float a_re[P], a_im[P], b_re[P], b_im[P], w_re[P], w_im[P], pw[2 * (M / 2 + 1)];
    const int lane = threadIdx.x, b = blockIdx.y, t0 = blockIdx.x * VOCODER_FRAMES;
    int len, frames;
    if (wave_lens != nullptr) {                                      // the front end's rule
        const long len64 = wave_lens[b];
        len = (int)(len64 < 0 ? 0 : len64 > Nmax ? Nmax : len64);
        frames = len > M ? 1 + len / hop : 0;
    } else {                                                         // the vocoder's: the frames are given, the length follows
        frames = vocoder_frames(frames_in, b, Tmax);
        len = frames > 0 ? (frames - 1) * hop : 0;                   // <= Nmax
        if (len <= M) frames = 0;
    }
    if (frames_out != nullptr && blockIdx.x == 0 && lane == 0) frames_out[b] = frames;
    const int t1 = t0 + VOCODER_FRAMES < Tmax ? t0 + VOCODER_FRAMES : Tmax;
    const int tv = t1 < frames ? t1 : frames;
    float2* ob = reinterpret_cast<float2*>(spec) + (long)b * Tmax * (M + 1);
    if (mag == nullptr) {                                            // the public transform: rows beyond the frames are zeros
        const int z0 = t0 > tv ? t0 : tv;
        float2* zp = ob + (long)z0 * (M + 1);
        for (long e = lane; e < (long)(t1 - z0) * (M + 1); e += THREADS) zp[e] = make_float2(0.f, 0.f);
    }
    if (t0 >= tv) return;                                            // (uniform)

    const AudioTables tb = audio_tables(N, 0, 0);
    float* pw_re = pw;
    float* pw_im = pw + M / 2 + 1;
    audio_stage_roots<N>(tables, tb, w_re, w_im, pw_re, lane);
    float win[PER_LANE];
    audio_load_window<N>(tables, tb, win, lane);
    const float* wb = wave + (long)b * ld_batch;
    const float* z_re = fft_result_in_second(M) ? b_re : a_re;
    const float* z_im = fft_result_in_second(M) ? b_im : a_im;
    const float* mb = mag != nullptr ? mag + (long)b * Tmax * (M + 1) : nullptr;
    float2* pb = prev != nullptr ? reinterpret_cast<float2*>(prev) + (long)b * Tmax * (M + 1) : nullptr;

    auto put = [&](long at, float xr, float xi) {
        if (mb != nullptr) {
            float tr = xr, ti = xi;
            if (pb != nullptr) {
                const float2 p = pb[at];
                tr = xr - mom * p.x;
                ti = xi - mom * p.y;
                pb[at] = make_float2(xr, xi);
            }
            const float a2 = tr * tr + ti * ti, g = mb[at];
            const float s = rsqrtf(a2);
            xr = a2 > 1e-30f ? g * (tr * s) : g;
            xi = a2 > 1e-30f ? g * (ti * s) : 0.f;
        }
        ob[at] = make_float2(xr, xi);
    };

    for (int t = t0; t < tv; ++t) {
        audio_load_frame<N>(wb, len, t * hop - M, win, a_re, a_im, lane);
        fft_lds<M, FFT_FORWARD, THREADS>(a_re, a_im, b_re, b_im, w_re, w_im, lane);
        const long at = (long)t * (M + 1);
        audio_unpack_real<N>(z_re, z_im, pw_re, pw_im, lane, [&](int k, float xr, float xi, float yr, float yi) {
            if (2 * k != M) put(at + k, xr, xi);                     // (bin n_fft/4 once, in the form audio.hip keeps)
            put(at + M - k, yr, -yi);
        });
        __syncthreads();                                             // the next frame's samples overwrite what was just read
    }
}

static int vocoder_check_config(const char* name, int B, int n_fft, int hop) {
    TTTS_REQUIRE(B >= 1, "%s: sizes must be positive (B %d)", name, B);
    TTTS_REQUIRE(audio_n_fft_ok(n_fft), "%s: n_fft must be one of 256, 512, 1024, 2048, got %d", name, n_fft);
    TTTS_REQUIRE(hop >= 1 && hop <= n_fft, "%s: hop must be in [1, n_fft] (hop %d, n_fft %d)", name, hop, n_fft);
    TTTS_REQUIRE(B <= 65535, "%s: grid too large (B %d, at most 65535 utterances a call)", name, B);
    return TTTS_OK;
}
static int vocoder_check_tmax(const char* name, long Tmax, int hop) {
    TTTS_REQUIRE(Tmax >= 2, "%s: Tmax must be at least 2, got %ld", name, Tmax);
    TTTS_REQUIRE((Tmax - 1) * hop <= (1L << 30), "%s: more than 2^30 samples per utterance are not supported (Tmax %ld, hop %d)", name,
                 Tmax, hop);
    return TTTS_OK;
}

}  // namespace ttts

using namespace ttts;

extern "C" {

int ttts_vocoder_pinv_check(const void* host_pinv, size_t bytes, int n_fft, int n_mels) {
    const char* name = "vocoder_pinv_check";
    TTTS_REQUIRE(host_pinv, "%s: null pointer", name);
    TTTS_REQUIRE(audio_n_fft_ok(n_fft), "%s: n_fft must be one of 256, 512, 1024, 2048, got %d", name, n_fft);
    TTTS_REQUIRE(n_mels >= 1, "%s: sizes must be positive (n_mels %d)", name, n_mels);
    TTTS_REQUIRE(n_mels <= AUDIO_MAX_MELS, "%s: at most %d filters (n_mels %d)", name, AUDIO_MAX_MELS, n_mels);
    TTTS_REQUIRE((reinterpret_cast<uintptr_t>(host_pinv) & 3) == 0, "%s: the matrix must be 4-byte aligned", name);
    const size_t need = (size_t)(n_fft / 2 + 1) * n_mels * 4;
    TTTS_REQUIRE(bytes == need, "%s: the matrix holds %zu bytes, %zu expected ((n_fft/2 + 1) x n_mels floats)", name, bytes, need);
    const float* p = static_cast<const float*>(host_pinv);
    for (size_t i = 0; i < need / 4; ++i)
        TTTS_REQUIRE(isfinite(p[i]), "%s: element (%zu, %zu) is not finite", name, i / n_mels, i % n_mels);
    return TTTS_OK;
}

int ttts_mel_to_magnitude(const float* mel, int64_t ld_row, int64_t ld_batch, const int64_t* melspec_lens, int B, int Tmax, int n_fft,
                          int hop, int n_mels, const float* pinv, const float* mean_std, float floor, float* mag, int64_t* frames,
                          void* stream) {
    const char* name = "mel_to_magnitude";
    TTTS_REQUIRE(mel && melspec_lens && pinv && mag && frames, "%s: null pointer", name);
    if (int rc = vocoder_check_config(name, B, n_fft, hop)) return rc;
    if (int rc = vocoder_check_tmax(name, Tmax, hop)) return rc;
    TTTS_REQUIRE(n_mels >= 1, "%s: sizes must be positive (n_mels %d)", name, n_mels);
    TTTS_REQUIRE(n_mels <= AUDIO_MAX_MELS, "%s: at most %d filters (n_mels %d)", name, AUDIO_MAX_MELS, n_mels);
    TTTS_REQUIRE(ld_row >= n_mels && (B == 1 || ld_batch >= (int64_t)(Tmax - 1) * ld_row + n_mels),
                 "%s: the strides must cover a row and a batch (ld_row %lld, ld_batch %lld, n_mels %d, Tmax %d)", name, (long long)ld_row,
                 (long long)ld_batch, n_mels, Tmax);
    TTTS_REQUIRE(floor > 0.f, "%s: floor must be positive, got %g", name, (double)floor);
    TTTS_REQUIRE(((reinterpret_cast<uintptr_t>(mel) | reinterpret_cast<uintptr_t>(pinv) | reinterpret_cast<uintptr_t>(mag) |
                   reinterpret_cast<uintptr_t>(mean_std)) & 3) == 0,
                 "%s: mel, pinv, mean_std and mag must be 4-byte aligned", name);
    TTTS_REQUIRE(((reinterpret_cast<uintptr_t>(melspec_lens) | reinterpret_cast<uintptr_t>(frames)) & 7) == 0,
                 "%s: melspec_lens and frames must be 8-byte aligned", name);
    const dim3 grid((unsigned)cdiv(Tmax, VOCODER_FRAMES), (unsigned)B);
    hipLaunchKernelGGL(mel_to_magnitude_kernel, grid, dim3(VOCODER_MAG_THREADS), 0, (hipStream_t)stream, mel, (long)ld_row, (long)ld_batch,
                       melspec_lens, Tmax, n_fft / 2 + 1, hop, n_mels, pinv, mean_std, floor, mag, frames);
    TTTS_LAUNCH_CHECK("mel_to_magnitude_kernel");
    return TTTS_OK;
}

int ttts_istft(const float* spec, const int64_t* frames, int B, int Tmax, int n_fft, int hop, const void* tables, float* wave,
               int64_t* wave_lens, void* stream) {
    const char* name = "istft";
    TTTS_REQUIRE(spec && frames && tables && wave && wave_lens, "%s: null pointer", name);
    if (int rc = vocoder_check_config(name, B, n_fft, hop)) return rc;
    if (int rc = vocoder_check_tmax(name, Tmax, hop)) return rc;
    TTTS_REQUIRE((reinterpret_cast<uintptr_t>(spec) & 7) == 0, "%s: spec must be 8-byte aligned (complex pairs)", name);
    TTTS_REQUIRE(((reinterpret_cast<uintptr_t>(tables) | reinterpret_cast<uintptr_t>(wave)) & 3) == 0,
                 "%s: tables and wave must be 4-byte aligned", name);
    TTTS_REQUIRE(((reinterpret_cast<uintptr_t>(frames) | reinterpret_cast<uintptr_t>(wave_lens)) & 7) == 0,
                 "%s: frames and wave_lens must be 8-byte aligned", name);
    const long Nmax = (long)(Tmax - 1) * hop;
    const dim3 grid((unsigned)cdiv(Nmax, (long)VOCODER_SPAN_MULT * n_fft), (unsigned)B);
    const float* tb = static_cast<const float*>(tables);
#define TTTS_ISTFT_LAUNCH(N) \
    hipLaunchKernelGGL(istft_kernel<N>, grid, dim3(audio_threads(N)), 0, (hipStream_t)stream, spec, frames, Tmax, hop, tb, wave, wave_lens)
    switch (n_fft) {
        case 256: TTTS_ISTFT_LAUNCH(256); break;
        case 512: TTTS_ISTFT_LAUNCH(512); break;
        case 1024: TTTS_ISTFT_LAUNCH(1024); break;
        default: TTTS_ISTFT_LAUNCH(2048); break;
    }
#undef TTTS_ISTFT_LAUNCH
    TTTS_LAUNCH_CHECK("istft_kernel");
    return TTTS_OK;
}

int ttts_stft_project(const float* wave, int64_t ld_batch, const int64_t* wave_lens, const int64_t* frames, int B, int Nmax, int n_fft,
                      int hop, const void* tables, const float* mag, float* prev, float momentum, float* spec, int64_t* frames_out,
                      void* stream) {
    const char* name = "stft_project";
    TTTS_REQUIRE(wave && tables && spec, "%s: null pointer", name);
    TTTS_REQUIRE((wave_lens != nullptr) != (frames != nullptr), "%s: give wave_lens or frames, one of them", name);
    if (int rc = vocoder_check_config(name, B, n_fft, hop)) return rc;
    TTTS_REQUIRE(Nmax >= 1, "%s: sizes must be positive (Nmax %d)", name, Nmax);
    TTTS_REQUIRE(Nmax <= (1 << 30), "%s: more than 2^30 samples per utterance are not supported (Nmax %d)", name, Nmax);
    const int Tmax = 1 + Nmax / hop;
    if (int rc = vocoder_check_tmax(name, Tmax, hop)) return rc;
    TTTS_REQUIRE(ld_batch >= Nmax || (B == 1 && ld_batch >= 0), "%s: the batch stride must be >= Nmax (ld_batch %lld, Nmax %d)", name,
                 (long long)ld_batch, Nmax);
    TTTS_REQUIRE(momentum >= 0.f && momentum < 1.f, "%s: momentum must be in [0, 1), got %g", name, (double)momentum);
    TTTS_REQUIRE(mag != nullptr || (prev == nullptr && momentum == 0.f), "%s: prev and momentum need mag (the projection)", name);
    TTTS_REQUIRE(!(momentum > 0.f) || prev != nullptr, "%s: momentum %g needs prev", name, (double)momentum);
    TTTS_REQUIRE(((reinterpret_cast<uintptr_t>(spec) | reinterpret_cast<uintptr_t>(prev)) & 7) == 0,
                 "%s: spec and prev must be 8-byte aligned (complex pairs)", name);
    TTTS_REQUIRE(((reinterpret_cast<uintptr_t>(wave) | reinterpret_cast<uintptr_t>(tables) | reinterpret_cast<uintptr_t>(mag)) & 3) == 0,
                 "%s: wave, tables and mag must be 4-byte aligned", name);
    TTTS_REQUIRE(((reinterpret_cast<uintptr_t>(wave_lens) | reinterpret_cast<uintptr_t>(frames) | reinterpret_cast<uintptr_t>(frames_out)) & 7) == 0,
                 "%s: wave_lens, frames and frames_out must be 8-byte aligned", name);
    const dim3 grid((unsigned)cdiv(Tmax, VOCODER_FRAMES), (unsigned)B);
    const float* tb = static_cast<const float*>(tables);
    const float mom = momentum / (1.f + momentum);
#define TTTS_STFT_LAUNCH(N)                                                                                                         \
    hipLaunchKernelGGL(stft_project_kernel<N>, grid, dim3(audio_threads(N)), 0, (hipStream_t)stream, wave, (long)ld_batch, wave_lens, \
                       frames, Nmax, hop, Tmax, tb, mag, prev, mom, spec, frames_out)
    switch (n_fft) {
        case 256: TTTS_STFT_LAUNCH(256); break;
        case 512: TTTS_STFT_LAUNCH(512); break;
        case 1024: TTTS_STFT_LAUNCH(1024); break;
        default: TTTS_STFT_LAUNCH(2048); break;
    }
#undef TTTS_STFT_LAUNCH
    TTTS_LAUNCH_CHECK("stft_project_kernel");
    return TTTS_OK;
}

}  // extern "C"
