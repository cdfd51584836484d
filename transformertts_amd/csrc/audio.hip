// Log-mel front end (gfx950): a ragged batch of waveforms to the model-ready (B, Tmax, n_mels) log-mel batch in one pass, the
// restatement of librosa.stft(center=True, pad_mode='reflect', window='hann') -> |.| -> slaney mel basis -> log(clip) [-> normalise].
//   framing     frame t of utterance b covers samples g = t hop - n_fft/2 + n, n = 0 .. n_fft - 1, of its len = wave_lens[b]
//               (clamped to [0, Nmax]); g < 0 reads sample -g, g >= len reads sample 2 (len - 1) - g: the reflection that does not
//               repeat the edge.  len >= n_fft/2 + 1 makes one reflection per index enough (len = n_fft/2 + 1: frame 0 reflects on
//               both sides).  frames = 1 + len / hop; len <= n_fft/2 cannot be reflected: 0 frames.  Nothing at or past len is read
//               and there is no padded copy of the signal anywhere.
//   window      periodic Hann of win_length, 0.5 - 0.5 cos(2 pi n / win_length), centred in n_fft (left pad (n_fft - win_length)/2),
//               from the host's table
//   transform   z[m] = x[2m] + i x[2m+1], one complex FFT of M = n_fft/2 points in LDS (fft_lds.h), then with Z[M] = Z[0]
//               E = (Z[k] + conj Z[M-k]) / 2, O = -i (Z[k] - conj Z[M-k]) / 2, X[k] = E + w^k O, X[M-k] = conj(E - w^k O),
//               w = exp(-2 pi i / n_fft): the n_fft/2 + 1 magnitudes |X[k]| stay in LDS
//   mel         filter f = sum_i weights[off_f + i] * |X[first_f + i]|, i < count_f in order, from the packed table
//   value       mel <= clip_val ? logf(clip_val) : logf(mel), then with statistics (x - mean) / (std + 1e-8)
// A workgroup of n_fft / 8 threads (64 at the least) carries AUDIO_FRAMES consecutive frames of one utterance, one after the
// other, all its threads on the same frame: a thread holds the window values of its samples tid + THREADS i in registers and
// the workgroup's LDS holds the roots, w^k and the packed filters, all loaded once; a frame's samples are loaded THREADS
// neighbouring floats at a time (each sample is asked for n_fft / hop times, all but the first from L2); a stage of the FFT is
// one radix-4 butterfly per thread, the mel projection one filter per thread.  Rows from frames[b] to Tmax are written as zeros
// by the workgroup that owns them.  The statistics kernel adds x and x^2 of an utterance's valid rows in double, one
// workgroup per utterance and a fixed tree: no atomics, the same bits every call.
#include "fft_lds.h"
#include "audio_common.h"
#include "ttts_common.h"

#include <math.h>

namespace ttts {

constexpr int AUDIO_FRAMES = 8;          // frames a workgroup carries
constexpr int AUDIO_MAX_NNZ = 4096;      // weights a workgroup stages in LDS (a triangular bank holds about 2 per bin)

// (the table layout, audio_threads, the frame load and the real-FFT unpacking: audio_common.h, shared with vocoder.hip)
template <int N>
__global__ __launch_bounds__(audio_threads(N)) void logmel_kernel(const float* __restrict__ wave, long ld_batch,
                                                                  const int64_t* __restrict__ wave_lens, int Nmax, int hop, int Tmax,
                                                                  int n_mels, int nnz, const float* __restrict__ tables, float clip_val,
                                                                  float log_clip, const float* __restrict__ mean_std,
                                                                  float* __restrict__ out, int64_t* __restrict__ mel_lens, int mode) {
    constexpr int M = N / 2, P = fft_padded_size(M), THREADS = audio_threads(N), PER_LANE = N / THREADS;
    __shared__ float a_re[P], a_im[P], b_re[P], b_im[P], w_re[P], w_im[P];
    const int lane = threadIdx.x, b = blockIdx.y, t0 = blockIdx.x * AUDIO_FRAMES;
    const long len64 = wave_lens[b];
    const int len = (int)(len64 < 0 ? 0 : len64 > Nmax ? Nmax : len64);      // Nmax <= 2^30: every index below fits an int
    const int frames = len > M ? 1 + len / hop : 0;                  // <= Tmax = 1 + Nmax / hop
    if (blockIdx.x == 0 && lane == 0) mel_lens[b] = frames;
    const int width = mode == TTTS_AUDIO_MAGNITUDE ? M + 1 : n_mels;
    float* ob = out + (long)b * Tmax * width;
    const int t1 = t0 + AUDIO_FRAMES < Tmax ? t0 + AUDIO_FRAMES : Tmax;
    const int tv = t1 < frames ? t1 : frames;                        // frames t0 .. tv - 1 are computed, tv .. t1 - 1 are zeros
    {
        const int z0 = t0 > tv ? t0 : tv;
        float* zp = ob + (long)z0 * width;
        for (long e = lane; e < (long)(t1 - z0) * width; e += THREADS) zp[e] = 0.f;
    }
    if (t0 >= tv) return;                                            // (uniform)

    // staged once per workgroup: the roots (padded layout), w^k, and the packed filters
    extern __shared__ float dyn[];
    float* pw_re = dyn;
    float* pw_im = pw_re + M / 2 + 1;
    float* weights = pw_im + M / 2 + 1;
    int32_t* f_first = reinterpret_cast<int32_t*>(weights + nnz);
    int32_t* f_count = f_first + n_mels;
    int32_t* f_off = f_count + n_mels;
    const AudioTables tb = audio_tables(N, n_mels, nnz);
    audio_stage_roots<N>(tables, tb, w_re, w_im, pw_re, lane);
    if (mode == TTTS_AUDIO_LOGMEL) {                                 // (uniform)
        const int32_t* ti = reinterpret_cast<const int32_t*>(tables);
        for (int k = lane; k < 3 * n_mels; k += THREADS) f_first[k] = ti[tb.first + k];   // (count, offset behind it)
        for (int k = lane; k < nnz; k += THREADS) weights[k] = tables[tb.weights + k];
    }
    float win[PER_LANE];
    audio_load_window<N>(tables, tb, win, lane);
    const bool norm = mean_std != nullptr && mode == TTTS_AUDIO_LOGMEL;
    const float mean = norm ? mean_std[0] : 0.f, sdev = norm ? mean_std[1] + 1e-8f : 1.f;
    const float* wb = wave + (long)b * ld_batch;
    // the spectrum lands in (z_re, z_im); the magnitudes go to the real array of the other pair
    float* z_re = fft_result_in_second(M) ? b_re : a_re;
    float* z_im = fft_result_in_second(M) ? b_im : a_im;
    float* mag = fft_result_in_second(M) ? a_re : b_re;

    for (int t = t0; t < tv; ++t) {
        audio_load_frame<N>(wb, len, t * hop - M, win, a_re, a_im, lane);
        fft_lds<M, FFT_FORWARD, THREADS>(a_re, a_im, b_re, b_im, w_re, w_im, lane);
        audio_unpack_real<N>(z_re, z_im, pw_re, pw_im, lane, [&](int k, float xr, float xi, float yr, float yi) {
            mag[k] = sqrtf(xr * xr + xi * xi);
            mag[M - k] = sqrtf(yr * yr + yi * yi);
        });
        __syncthreads();
        if (mode == TTTS_AUDIO_MAGNITUDE) {                          // (uniform)
            float* row = ob + (long)t * (M + 1);
            for (int k = lane; k <= M; k += THREADS) row[k] = mag[k];
        } else {
            float* row = ob + (long)t * n_mels;
            for (int f = lane; f < n_mels; f += THREADS) {
                int first = f_first[f], count = f_count[f], off = f_off[f];
                first = first < 0 ? 0 : first > M ? M : first;       // a table that passed ttts_audio_tables_check is left as it is
                off = off < 0 ? 0 : off > nnz ? nnz : off;
                count = count < 0 ? 0 : count;
                count = count > M + 1 - first ? M + 1 - first : count;
                count = count > nnz - off ? nnz - off : count;
                float acc = 0.f;
#pragma unroll 4
                for (int i = 0; i < count; ++i) acc = fmaf(weights[off + i], mag[first + i], acc);
                float v = acc <= clip_val ? log_clip : logf(acc);
                if (norm) v = (v - mean) / sdev;
                row[f] = v;
            }
        }
        __syncthreads();                                             // the next frame's samples overwrite what was just read
    }
}

__global__ __launch_bounds__(256) void logmel_stats_kernel(const float* __restrict__ mel, const int64_t* __restrict__ mel_lens, int Tmax,
                                                           int n_mels, double* __restrict__ sums) {
    __shared__ double ss[256], qq[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    long frames = mel_lens[b];
    frames = frames < 0 ? 0 : frames > Tmax ? Tmax : frames;
    const long n = frames * n_mels;
    const float* p = mel + (long)b * Tmax * n_mels;
    double s = 0.0, q = 0.0;
    for (long e = tid; e < n; e += 256) {
        const double v = (double)p[e];
        s += v;
        q += v * v;
    }
    ss[tid] = s;
    qq[tid] = q;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            ss[tid] += ss[tid + o];
            qq[tid] += qq[tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        sums[2 * b] = ss[0];
        sums[2 * b + 1] = qq[0];
    }
}

}  // namespace ttts

using namespace ttts;

extern "C" {

size_t ttts_audio_tables_bytes(int n_fft, int n_mels, int nnz) {
    if (!audio_n_fft_ok(n_fft) || n_mels < 1 || nnz < 1) return 0;
    return (size_t)audio_tables(n_fft, n_mels, nnz).words * 4;
}

int ttts_audio_tables_check(const void* host_tables, size_t bytes, int n_fft, int win_length, int n_mels, int nnz) {
    const char* name = "audio_tables_check";
    TTTS_REQUIRE(host_tables, "%s: null pointer", name);
    TTTS_REQUIRE(audio_n_fft_ok(n_fft), "%s: n_fft must be one of 256, 512, 1024, 2048, got %d", name, n_fft);
    TTTS_REQUIRE(win_length >= 1 && win_length <= n_fft, "%s: win_length must be in [1, n_fft] (win_length %d, n_fft %d)", name,
                 win_length, n_fft);
    TTTS_REQUIRE(n_mels >= 1 && nnz >= 1, "%s: sizes must be positive (n_mels %d, nnz %d)", name, n_mels, nnz);
    TTTS_REQUIRE((reinterpret_cast<uintptr_t>(host_tables) & 3) == 0, "%s: the tables must be 4-byte aligned", name);
    const size_t need = ttts_audio_tables_bytes(n_fft, n_mels, nnz);
    TTTS_REQUIRE(bytes == need, "%s: the tables hold %zu bytes, %zu expected", name, bytes, need);
    const uint32_t* h = static_cast<const uint32_t*>(host_tables);
    TTTS_REQUIRE(h[0] == AUDIO_MAGIC && (int)h[1] == n_fft && (int)h[2] == win_length && (int)h[3] == n_mels && (int)h[4] == nnz,
                 "%s: the header does not match (n_fft %d, win_length %d, n_mels %d, nnz %d)", name, n_fft, win_length, n_mels, nnz);
    const AudioTables tb = audio_tables(n_fft, n_mels, nnz);
    const int32_t* w = static_cast<const int32_t*>(host_tables);
    long at = 0;
    for (int f = 0; f < n_mels; ++f) {
        const long first = w[tb.first + f], count = w[tb.count + f], off = w[tb.offset + f];
        TTTS_REQUIRE(first >= 0 && count >= 0 && first + count <= n_fft / 2 + 1, "%s: filter %d leaves the %d bins (first %ld, count %ld)",
                     name, f, n_fft / 2 + 1, first, count);
        TTTS_REQUIRE(off == at, "%s: filter %d starts at weight %ld, %ld expected", name, f, off, at);
        at += count;
    }
    TTTS_REQUIRE(at == nnz, "%s: the filters hold %ld weights, nnz is %d", name, at, nnz);
    return TTTS_OK;
}

int ttts_logmel(const float* wave, int64_t ld_batch, const int64_t* wave_lens, int B, int Nmax, int n_fft, int hop, int n_mels,
                int nnz, const void* tables, float clip_val, const float* mean_std, float* out, int64_t* mel_lens, int mode,
                void* stream) {
    const char* name = "logmel";
    TTTS_REQUIRE(wave && wave_lens && tables && out && mel_lens, "%s: null pointer", name);
    TTTS_REQUIRE(B >= 1 && Nmax >= 1, "%s: sizes must be positive (B %d, Nmax %d)", name, B, Nmax);
    TTTS_REQUIRE(Nmax <= (1 << 30), "%s: more than 2^30 samples per utterance are not supported (Nmax %d)", name, Nmax);
    TTTS_REQUIRE(audio_n_fft_ok(n_fft), "%s: n_fft must be one of 256, 512, 1024, 2048, got %d", name, n_fft);
    TTTS_REQUIRE(hop >= 1 && hop <= n_fft, "%s: hop must be in [1, n_fft] (hop %d, n_fft %d)", name, hop, n_fft);
    TTTS_REQUIRE(n_mels >= 1 && nnz >= 1, "%s: sizes must be positive (n_mels %d, nnz %d)", name, n_mels, nnz);
    TTTS_REQUIRE(n_mels <= AUDIO_MAX_MELS && nnz <= AUDIO_MAX_NNZ, "%s: at most %d filters and %d weights (n_mels %d, nnz %d)", name,
                 AUDIO_MAX_MELS, AUDIO_MAX_NNZ, n_mels, nnz);
    TTTS_REQUIRE(mode == TTTS_AUDIO_LOGMEL || mode == TTTS_AUDIO_MAGNITUDE, "%s: unknown mode %d", name, mode);
    TTTS_REQUIRE(ld_batch >= Nmax || (B == 1 && ld_batch >= 0), "%s: the batch stride must be >= Nmax (ld_batch %lld, Nmax %d)", name,
                 (long long)ld_batch, Nmax);
    TTTS_REQUIRE(clip_val > 0.f, "%s: clip_val must be positive, got %g", name, (double)clip_val);
    TTTS_REQUIRE(((reinterpret_cast<uintptr_t>(wave) | reinterpret_cast<uintptr_t>(tables) | reinterpret_cast<uintptr_t>(out) |
                   reinterpret_cast<uintptr_t>(mean_std)) & 3) == 0,
                 "%s: wave, tables, mean_std and out must be 4-byte aligned", name);
    TTTS_REQUIRE(((reinterpret_cast<uintptr_t>(wave_lens) | reinterpret_cast<uintptr_t>(mel_lens)) & 7) == 0,
                 "%s: wave_lens and mel_lens must be 8-byte aligned", name);
    TTTS_REQUIRE(B <= 65535, "%s: grid too large (B %d, at most 65535 utterances a call)", name, B);
    const int Tmax = 1 + Nmax / hop;
    const dim3 grid((unsigned)cdiv(Tmax, AUDIO_FRAMES), (unsigned)B);
    const float log_clip = (float)log((double)clip_val);
    const float* tb = static_cast<const float*>(tables);
#define TTTS_LOGMEL_LAUNCH(N)                                                                                                   \
    hipLaunchKernelGGL(logmel_kernel<N>, grid, dim3(audio_threads(N)), (size_t)(2 * (N / 4 + 1) + nnz + 3 * n_mels) * 4,        \
                       (hipStream_t)stream, wave, (long)ld_batch, wave_lens, Nmax, hop, Tmax, n_mels, nnz, tb, clip_val, log_clip, \
                       mean_std, out, mel_lens, mode)
    switch (n_fft) {
        case 256: TTTS_LOGMEL_LAUNCH(256); break;
        case 512: TTTS_LOGMEL_LAUNCH(512); break;
        case 1024: TTTS_LOGMEL_LAUNCH(1024); break;
        default: TTTS_LOGMEL_LAUNCH(2048); break;
    }
#undef TTTS_LOGMEL_LAUNCH
    TTTS_LAUNCH_CHECK("logmel_kernel");
    return TTTS_OK;
}

int ttts_logmel_stats(const float* mel, const int64_t* mel_lens, int B, int Tmax, int n_mels, double* sums, void* stream) {
    const char* name = "logmel_stats";
    TTTS_REQUIRE(mel && mel_lens && sums, "%s: null pointer", name);
    TTTS_REQUIRE(B >= 1 && Tmax >= 1 && n_mels >= 1, "%s: sizes must be positive (B %d, Tmax %d, n_mels %d)", name, B, Tmax, n_mels);
    TTTS_REQUIRE((reinterpret_cast<uintptr_t>(mel) & 3) == 0, "%s: mel must be 4-byte aligned", name);
    TTTS_REQUIRE(((reinterpret_cast<uintptr_t>(mel_lens) | reinterpret_cast<uintptr_t>(sums)) & 7) == 0,
                 "%s: mel_lens and sums must be 8-byte aligned", name);
    hipLaunchKernelGGL(logmel_stats_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, mel, mel_lens, Tmax, n_mels, sums);
    TTTS_LAUNCH_CHECK("logmel_stats_kernel");
    return TTTS_OK;
}

}  // extern "C"
