// A complex M-point FFT in LDS, M a power of two from 8 up, worked by all THREADS threads of a workgroup (gfx950).  Stockham
// autosort, radix 4 with one closing radix-2 stage when log2 M is odd (128 = 4.4.4.2, 256 = 4^4, 512 = 4^4.2, 1024 = 4^5): no bit
// reversal, every stage reads one buffer and writes the other, one barrier per stage.  Radix 4 and not 8: a radix-4 butterfly has
// no multiplication of its own (+-1, +-i), holds 8 live floats and so leaves the registers to the caller's frame loop; radix 8
// would save one of five passes over LDS at M = 512 and need sqrt(1/2) rotations and twice the registers.
//
// Layout: split real and imaginary arrays (4-byte accesses: 32 banks, two groups of 32 lanes per instruction) and one dword of
// padding after every 32, element i at fft_pad(i) = i + (i >> 5).  Stage with sub-transform length NS, butterfly j of M / R:
//   reads   in[j + r M/R], r < R: neighbouring lanes read neighbouring dwords and M/R is a multiple of 32, so a lane group never
//           crosses a padding dword out of step: conflict-free
//   writes  out[(j - k) R + k + r NS], k = j mod NS: without the padding the first stage (NS = 1) writes at a stride of 4 dwords,
//           4 lanes to a bank; with it the 32 lanes of a group fall on 32 banks for NS = 1 and NS >= 32, and two lanes share a
//           bank for NS = 4 and 16, which a 4-byte store absorbs without extra cycles
//   twiddles  w[k r M / (NS R)] from a table of all M roots in the same padded layout (strides of 8 and 32 entries otherwise land
//           on 4 and 1 banks)
// The table holds the FORWARD roots exp(-2 pi i k / M) = (cos, -sin), built by the host in fp64 and rounded to fp32; DIR =
// FFT_INVERSE conjugates them on the fly (and leaves the 1/M to the caller).  No sincosf anywhere.
#pragma once
#include <hip/hip_runtime.h>

namespace ttts {

constexpr int FFT_FORWARD = -1;
constexpr int FFT_INVERSE = 1;

__host__ __device__ constexpr int fft_pad(int i) { return i + (i >> 5); }
// floats an array of M padded elements takes
__host__ __device__ constexpr int fft_padded_size(int M) { return M + (M >> 5) + 1; }
__host__ __device__ constexpr int fft_stages(int M) {
    int s = 0;
    for (int ns = 1; ns < M; ns *= (M / ns >= 4 ? 4 : 2)) ++s;
    return s;
}
// after fft_lds the spectrum lies in the second pair of arrays iff the number of stages is odd
__host__ __device__ constexpr bool fft_result_in_second(int M) { return (fft_stages(M) & 1) != 0; }

template <int M, int R, int NS, int DIR, int THREADS>
__device__ __forceinline__ void fft_stage(const float* in_re, const float* in_im, float* out_re, float* out_im, const float* w_re,
                                          const float* w_im, int tid) {
    static_assert(R == 4 || R == 2, "radix 4 or 2");
    constexpr int Q = M / R;
#pragma unroll
    for (int j0 = 0; j0 < Q; j0 += THREADS) {
        const int j = j0 + tid;
        if (Q % THREADS != 0 && j >= Q) break;
        const int k = j & (NS - 1);
        float vr[R], vi[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            vr[r] = in_re[fft_pad(j + r * Q)];
            vi[r] = in_im[fft_pad(j + r * Q)];
        }
        if (NS > 1) {
#pragma unroll
            for (int r = 1; r < R; ++r) {
                const int idx = fft_pad(k * r * (M / (NS * R)));
                const float wr = w_re[idx], wi = DIR == FFT_FORWARD ? w_im[idx] : -w_im[idx];
                const float xr = vr[r], xi = vi[r];
                vr[r] = xr * wr - xi * wi;
                vi[r] = xr * wi + xi * wr;
            }
        }
        const int base = (j - k) * R + k;
        if (R == 2) {
            out_re[fft_pad(base)] = vr[0] + vr[1];
            out_im[fft_pad(base)] = vi[0] + vi[1];
            out_re[fft_pad(base + NS)] = vr[0] - vr[1];
            out_im[fft_pad(base + NS)] = vi[0] - vi[1];
        } else {
            const float ar = vr[0] + vr[R / 2], ai = vi[0] + vi[R / 2], br = vr[0] - vr[R / 2], bi = vi[0] - vi[R / 2];
            const float cr = vr[1] + vr[R - 1], ci = vi[1] + vi[R - 1], dr = vr[1] - vr[R - 1], di = vi[1] - vi[R - 1];
            // forward: V1 = b - i d, V3 = b + i d; inverse: the other way round
            const float er = DIR == FFT_FORWARD ? di : -di, ei = DIR == FFT_FORWARD ? -dr : dr;
            out_re[fft_pad(base)] = ar + cr;
            out_im[fft_pad(base)] = ai + ci;
            out_re[fft_pad(base + NS)] = br + er;
            out_im[fft_pad(base + NS)] = bi + ei;
            out_re[fft_pad(base + 2 * NS)] = ar - cr;
            out_im[fft_pad(base + 2 * NS)] = ai - ci;
            out_re[fft_pad(base + 3 * NS)] = br - er;
            out_im[fft_pad(base + 3 * NS)] = bi - ei;
        }
    }
}

template <int M, int NS, int DIR, int THREADS>
__device__ __forceinline__ void fft_stages_from(float* a_re, float* a_im, float* b_re, float* b_im, const float* w_re,
                                                const float* w_im, int tid) {
    if constexpr (NS < M) {
        constexpr int R = M / NS >= 4 ? 4 : 2;
        fft_stage<M, R, NS, DIR, THREADS>(a_re, a_im, b_re, b_im, w_re, w_im, tid);
        __syncthreads();
        fft_stages_from<M, NS * R, DIR, THREADS>(b_re, b_im, a_re, a_im, w_re, w_im, tid);
    }
}

// X[k] = sum_n x[n] exp(DIR 2 pi i k n / M) of the M values in (a_re, a_im), all four arrays of fft_padded_size(M) floats in LDS,
// (w_re, w_im) the forward roots in the padded layout.  Every thread of the workgroup calls it (it holds barriers; the first one
// orders the caller's stores of x and of the roots before the first stage).  The result lies in (b_re, b_im) if
// fft_result_in_second(M), else in (a_re, a_im); the other pair holds garbage.  A barrier closes the last stage.
template <int M, int DIR, int THREADS>
__device__ __forceinline__ void fft_lds(float* a_re, float* a_im, float* b_re, float* b_im, const float* w_re, const float* w_im,
                                        int tid) {
    static_assert(M >= 8 && (M & (M - 1)) == 0, "M must be a power of two");
    static_assert(DIR == FFT_FORWARD || DIR == FFT_INVERSE, "direction");
    __syncthreads();
    fft_stages_from<M, 1, DIR, THREADS>(a_re, a_im, b_re, b_im, w_re, w_im, tid);
}

}  // namespace ttts
