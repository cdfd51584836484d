// What the log-mel front end (audio.hip) and the vocoder (vocoder.hip) share: the table buffer's layout, the workgroup size of a
// frame, the load of one windowed frame with reflection into the packed FFT input, and the unpacking of the packed M = n_fft/2
// point spectrum into the n_fft/2 + 1 bins of the real transform.  Everything here is inlined into the caller's frame loop.
#pragma once
#include "fft_lds.h"

#include <stdint.h>

namespace ttts {

constexpr int AUDIO_HEADER = 8;          // words in front of the tables
constexpr uint32_t AUDIO_MAGIC = 0x4C454D54u;
constexpr int AUDIO_MAX_MELS = 512;      // static + staged LDS stay under 64 KB at n_fft 2048

// threads that share a frame: 8 samples and one or two butterflies of a stage per thread
__host__ __device__ constexpr int audio_threads(int n_fft) { return n_fft / 8 < 64 ? 64 : n_fft / 8; }
__host__ __device__ static inline bool audio_n_fft_ok(int n) { return n == 256 || n == 512 || n == 1024 || n == 2048; }
// the table buffer in 4-byte words: header | window (n_fft) | roots re, im (M each) | w^k re, im (M/2 + 1 each) | first, count,
// offset (n_mels each, int32) | weights (nnz).  The sections up to w^k depend on n_fft alone.
struct AudioTables {
    long window, tw_re, tw_im, pw_re, pw_im, first, count, offset, weights, words;
};
__host__ __device__ static inline AudioTables audio_tables(int n_fft, int n_mels, int nnz) {
    const long M = n_fft / 2;
    AudioTables t;
    t.window = AUDIO_HEADER;
    t.tw_re = t.window + n_fft;
    t.tw_im = t.tw_re + M;
    t.pw_re = t.tw_im + M;
    t.pw_im = t.pw_re + M / 2 + 1;
    t.first = t.pw_im + M / 2 + 1;
    t.count = t.first + n_mels;
    t.offset = t.count + n_mels;
    t.weights = t.offset + n_mels;
    t.words = t.weights + nnz;
    return t;
}

// the roots of the M-point FFT into the padded LDS layout and w^k (re, im back to back) behind `pw_re`; the caller's first
// barrier (fft_lds holds one) orders them before their use
template <int N>
__device__ __forceinline__ void audio_stage_roots(const float* __restrict__ tables, const AudioTables& tb, float* w_re, float* w_im,
                                                  float* pw_re, int lane) {
    constexpr int M = N / 2, THREADS = audio_threads(N);
    for (int k = lane; k < M; k += THREADS) {
        w_re[fft_pad(k)] = tables[tb.tw_re + k];
        w_im[fft_pad(k)] = tables[tb.tw_im + k];
    }
    for (int k = lane; k < 2 * (M / 2 + 1); k += THREADS) pw_re[k] = tables[tb.pw_re + k];   // (re, im back to back)
}

// the window values of this thread's samples lane + THREADS i
template <int N>
__device__ __forceinline__ void audio_load_window(const float* __restrict__ tables, const AudioTables& tb,
                                                  float (&win)[N / audio_threads(N)], int lane) {
    constexpr int THREADS = audio_threads(N), PER_LANE = N / THREADS;
#pragma unroll
    for (int i = 0; i < PER_LANE; ++i) win[i] = tables[tb.window + lane + THREADS * i];
}

// frame samples g = start + n, n < N, of the len samples at wb, reflected without repeating the edge (g < 0 reads -g, g >= len
// reads 2 (len - 1) - g), times the window, packed as z[m] = x[2m] + i x[2m+1] into (a_re, a_im)
template <int N>
__device__ __forceinline__ void audio_load_frame(const float* __restrict__ wb, int len, int start,
                                                 const float (&win)[N / audio_threads(N)], float* a_re, float* a_im, int lane) {
    constexpr int THREADS = audio_threads(N), PER_LANE = N / THREADS;
#pragma unroll
    for (int i = 0; i < PER_LANE; ++i) {
        const int n = lane + THREADS * i;
        int g = start + n;
        g = g < 0 ? -g : g;
        g = g >= len ? 2 * (len - 1) - g : g;
        g = g < 0 ? 0 : g > len - 1 ? len - 1 : g;               // (never acts for len >= n_fft/2 + 1; keeps every load inside)
        const float v = wb[g] * win[i];
        ((n & 1) ? a_im : a_re)[fft_pad(n >> 1)] = v;
    }
}

// With Z the M-point spectrum of the packed frame and Z[M] = Z[0]: E = (Z[k] + conj Z[M-k]) / 2, O = -i (Z[k] - conj Z[M-k]) / 2,
// X[k] = E + w^k O, X[M-k] = conj(E - w^k O).  emit(k, xr, xi, yr, yi) with X[k] = (xr, xi) and X[M-k] = (yr, -yi) for this
// thread's k <= M/2 (k = M/2 meets itself: both values are the same bin).
template <int N, class Emit>
__device__ __forceinline__ void audio_unpack_real(const float* z_re, const float* z_im, const float* pw_re, const float* pw_im,
                                                  int lane, Emit&& emit) {
    constexpr int M = N / 2, THREADS = audio_threads(N);
    for (int k = lane; k <= M / 2; k += THREADS) {
        const int m = (M - k) & (M - 1);
        const float zkr = z_re[fft_pad(k)], zki = z_im[fft_pad(k)], zmr = z_re[fft_pad(m)], zmi = z_im[fft_pad(m)];
        const float er = 0.5f * (zkr + zmr), ei = 0.5f * (zki - zmi);
        const float dr = 0.5f * (zkr - zmr), di = 0.5f * (zki + zmi);
        const float wr = pw_re[k], wi = pw_im[k];
        const float pr = di * wr + dr * wi, pi = di * wi - dr * wr;         // w^k O, O = (di, -dr)
        const float xr = er + pr, xi = ei + pi, yr = er - pr, yi = ei - pi;
        emit(k, xr, xi, yr, yi);
    }
}

}  // namespace ttts
