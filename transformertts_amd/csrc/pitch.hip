// Frame pitch and energy (gfx950): YIN F0, voicing and aperiodicity plus the STFT frame energy of a ragged batch of waveforms
// in one launch, and the phoneme-level means of such frame values.  YIN restated from its definition:
//   framing     the front end's (audio.hip): pitch frame t of utterance b holds x_n = wave[g], g = t hop - F/2 + n, n < F; the
//               energy frame is the n_fft samples centred at t hop.  g < 0 reads -g, g >= len reads 2 (len - 1) - g.
//               len_b = clamp(wave_lens[b], 0, Nmax), frames_b = len_b > max(F, n_fft) / 2 ? 1 + len_b / hop : 0, Tmax = 1 + Nmax / hop,
//               rows from frames_b to Tmax are zeros; nothing at or past len_b is read.
//   difference  d(tau) = sum_{j < W} (x_j - x_{j+tau})^2, tau = 1 .. tau_max, as differences squared in fp32 (never e(0) + e(tau)
//               - 2 acf(tau)).  The sum runs over blocks of BL samples, ascending j with fmaf from 0.f inside a block, the block
//               partials then added in ascending block order: BL = hop when hop divides W, W / hop <= 8 and the shared partials
//               fit the workgroup's LDS beside at least as many frames as without them, else BL = W (ttts_pitch_block).
//   normalised  d'(tau) = d(tau) * tau / sum_{k <= tau} d(k), 1 where that sum is 0.  The running sum goes over tiles of 64 lags:
//               a shuffle scan inside a tile (lag k adds lags k-1, k-2, k-4, ... in that order), tiles carried in ascending order.
//   lag         tau_0 = the first tau in [tau_min, tau_max] with d' < threshold: voiced, and tau* is reached from tau_0 by stepping
//               up while d'(tau + 1) < d'(tau); without one: unvoiced, tau* = the first argmin of d' over the range.
//   outputs     aperiodicity = d'(tau*); f0 = sample_rate / (tau* + s) when voiced, else 0; s = clamp(0.5 (a - c) / (a - 2 b + c),
//               -0.5, 0.5) with a, b, c = d'(tau* - 1, tau*, tau* + 1) when tau_min < tau* < tau_max and a - 2 b + c > 0, else 0.
//   energy      sqrt(sum_{k <= n_fft/2} |X[k]|^2) of the front end's STFT, without a transform: with y_n = w_n x_n the sum is
//               (n_fft sum y^2 + (sum y)^2 + (sum (-1)^n y)^2) / 2.  A lane adds its samples lane + 64 i in ascending i, the
//               64 lanes meet in a fixed butterfly.
// A workgroup of 256 threads owns R consecutive frames of one utterance (R <= 8, what its LDS admits).  It stages their span
// once, reflection applied there, then works in two phases.  Phase 1: block i (at span offset o + i hop) times a group of
// PITCH_LAGS neighbouring lags is one item of a thread; the thread walks j, reads x_j as a broadcast and slides x_{j+tau}
// through registers, so PITCH_LAGS subtract-and-FMA pairs cost 2 / PITCH_LAGS + a little LDS reads instead of 2.  Neighbouring
// lanes sit PITCH_LAGS floats apart: an odd count keeps them on distinct banks.  With BL = hop neighbouring frames share
// their block partials (R + W / hop - 1 blocks instead of R W / hop).  Phase 2: one wave per frame sums the frame's
// partials, scans, finds the crossing, walks or takes the argmin (ties to the lowest lag) and adds the three energy sums; lane
// 0 writes the four values.  No atomics, no host read; the bits of a frame depend on neither the grid, the batch nor the call.
#include "ttts_common.h"

#include <limits.h>
#include <math.h>

namespace ttts {

constexpr int PITCH_THREADS = 256;
constexpr int PITCH_WAVES = PITCH_THREADS / 64;
constexpr int PITCH_MAX_FRAMES = 8;        // frames a workgroup owns at the most
constexpr int PITCH_MAX_F = 4096;          // frame_length
constexpr int PITCH_MAX_SHARE = 8;         // block partials a frame adds at the most in the shared form
constexpr int PITCH_PAD = 8;               // zeros behind the span: the lags of a group's tail past tau_max read them
constexpr int PITCH_UNROLL = 4;            // samples j per step of the sliding window
constexpr size_t PITCH_LDS_BYTES = 60 * 1024;
#ifndef TTTS_PITCH_LAGS
#define TTTS_PITCH_LAGS 7                  // neighbouring lags a thread carries (1: the plain form; even counts meet bank conflicts)
#endif
#ifndef TTTS_PITCH_SHARE
#define TTTS_PITCH_SHARE 1                 // 0: every frame sums its own W samples (for measurements)
#endif
constexpr int PITCH_LAGS = TTTS_PITCH_LAGS;
static_assert(PITCH_LAGS >= 1 && PITCH_LAGS <= PITCH_PAD, "a group's tail must stay inside the pad");

struct PitchPlan {
    int frames, block, nb, half, span, waves;     // R, BL, W / BL, max(F, n_fft) / 2, staged floats incl. the pad, phase-2 buffers
    size_t lds;
};
static inline PitchPlan pitch_plan(int F, int n_fft, int hop, int W, int tau_max) {
    PitchPlan p;
    p.half = (F > n_fft ? F : n_fft) / 2;
    const bool can_share = TTTS_PITCH_SHARE && W % hop == 0 && W / hop <= PITCH_MAX_SHARE;
    for (int R = PITCH_MAX_FRAMES; R >= 1; --R)
        for (int share = can_share ? 1 : 0; share >= 0; --share) {
            p.frames = R;
            p.block = share ? hop : W;
            p.nb = W / p.block;
            p.span = (R - 1) * hop + 2 * p.half + PITCH_PAD;
            p.waves = R < PITCH_WAVES ? R : PITCH_WAVES;
            p.lds = ((size_t)p.span + (size_t)(R + p.nb - 1 + p.waves) * tau_max) * 4;
            if (p.lds <= PITCH_LDS_BYTES) return p;
        }
    return p;                                      // (R = 1 unshared is at most 4104 + 2 * 4095 floats: always fits)
}

__device__ __forceinline__ int wave_min_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int u = __shfl_xor(v, o, 64);
        v = u < v ? u : v;
    }
    return v;
}

// one block partial of G neighbouring lags: acc[g] = sum_{j < BL} (xp[j] - xp[j + tau + g])^2, ascending j
template <int G>
__device__ __forceinline__ void pitch_item(const float* xp, int tau, int BL, float* __restrict__ row, int tau_max) {
    constexpr int U = PITCH_UNROLL;
    const float* yp = xp + tau;
    float acc[G], w[G + U - 1];
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = 0.f;
#pragma unroll
    for (int k = 0; k < G - 1; ++k) w[k] = yp[k];
    int j = 0;
    for (; j + U <= BL; j += U) {
        float x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            x[u] = xp[j + u];
            w[G - 1 + u] = yp[j + G - 1 + u];
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const float d = x[u] - w[u + g];
                acc[g] = fmaf(d, d, acc[g]);
            }
#pragma unroll
        for (int k = 0; k < G - 1; ++k) w[k] = w[k + U];
    }
    for (; j < BL; ++j) {
        const float x = xp[j];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float d = x - yp[j + g];
            acc[g] = fmaf(d, d, acc[g]);
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g)
        if (tau + g <= tau_max) row[tau + g - 1] = acc[g];
}

__global__ __launch_bounds__(PITCH_THREADS) void pitch_energy_kernel(
    const float* __restrict__ wave, long ld_batch, const int64_t* __restrict__ wave_lens, int Nmax, int n_fft, int hop, int F, int W,
    int tau_min, int tau_max, float sample_rate, float threshold, const float* __restrict__ hann, int Tmax, int R, int BL, int nb,
    int half, int span_floats, float* __restrict__ f0, uint8_t* __restrict__ voiced, float* __restrict__ aper,
    float* __restrict__ energy, int64_t* __restrict__ frames_out) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.y, t0 = blockIdx.x * R;
    const long len64 = wave_lens[b];
    const int len = (int)(len64 < 0 ? 0 : len64 > Nmax ? Nmax : len64);      // Nmax <= 2^30: every index below fits an int
    const int frames = len > half ? 1 + len / hop : 0;                       // <= Tmax
    if (blockIdx.x == 0 && tid == 0) frames_out[b] = frames;
    const int t1 = t0 + R < Tmax ? t0 + R : Tmax;
    const int tv = t1 < frames ? t1 : frames;                                // frames t0 .. tv - 1 are computed, tv .. t1 - 1 zeros
    const long row = (long)b * Tmax;
    for (int t = (t0 > tv ? t0 : tv) + tid; t < t1; t += PITCH_THREADS) {
        f0[row + t] = 0.f;
        voiced[row + t] = 0;
        aper[row + t] = 0.f;
        energy[row + t] = 0.f;
    }
    if (t0 >= tv) return;                                                    // (uniform)
    const int Rv = tv - t0;

    // the span: xs[i] = x[t0 hop - half + i], i < (Rv - 1) hop + 2 half, reflected; PITCH_PAD zeros behind it
    float* xs = lds;
    float* part = lds + span_floats;                                         // block partials, [block][tau - 1], stride tau_max
    float* dps = part + (long)(R + nb - 1) * tau_max;                        // d' of the frame a wave is on, [wave][tau - 1]
    const int spanv = (Rv - 1) * hop + 2 * half;                             // <= span_floats - PITCH_PAD
    const float* wb = wave + (long)b * ld_batch;
    const int first = t0 * hop - half;
    for (int i = tid; i < spanv + PITCH_PAD; i += PITCH_THREADS) {
        int g = first + i;
        g = g < 0 ? -g : g;
        g = g >= len ? 2 * (len - 1) - g : g;
        g = g < 0 ? 0 : g > len - 1 ? len - 1 : g;                           // (never acts for len > half; keeps every load inside)
        xs[i] = i < spanv ? wb[g] : 0.f;
    }
    __syncthreads();

    // phase 1: item (block i, lag group q): lags 1 + G q .. G + G q of the BL samples at span offset o + i hop
    const int o = half - F / 2;
    const int groups = (tau_max + PITCH_LAGS - 1) / PITCH_LAGS;
    const int items = (Rv + nb - 1) * groups;
    for (int e = tid; e < items; e += PITCH_THREADS) {
        const int i = e / groups, q = e - i * groups;
        pitch_item<PITCH_LAGS>(xs + o + i * hop, 1 + PITCH_LAGS * q, BL, part + (long)i * tau_max, tau_max);
    }
    __syncthreads();

    // phase 2: wave wv takes frames wv, wv + 4, ... of the workgroup
    float* dp = dps + (long)wv * tau_max;                                    // (wv < min(4, R) whenever the wave has a frame)
    for (int r = wv; r < Rv; r += PITCH_WAVES) {
        const float* p0 = part + (long)r * tau_max;
        float carry = 0.f, best = INFINITY;
        int cross = INT_MAX, best_tau = INT_MAX;
        for (int base = 1; base <= tau_max; base += 64) {
            const int tau = base + lane;
            const bool in = tau <= tau_max;
            float d = 0.f;
            if (in) {
                d = p0[tau - 1];
                for (int k = 1; k < nb; ++k) d += p0[(long)k * tau_max + tau - 1];
            }
            float cs = d;
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) {
                const float u = __shfl_up(cs, s, 64);
                cs = lane >= s ? cs + u : cs;
            }
            cs += carry;
            carry = __shfl(cs, 63, 64);
            const float v = cs == 0.f ? 1.f : d * (float)tau / cs;
            if (in) {
                dp[tau - 1] = v;
                if (tau >= tau_min) {
                    if (v < threshold && tau < cross) cross = tau;
                    if (v < best) {
                        best = v;
                        best_tau = tau;
                    }
                }
            }
        }
        cross = wave_min_int(cross);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");               // the wave's d' row is written: every lane may read it
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        int tau_s;
        if (cross != INT_MAX) {                                              // (wave-uniform) voiced: walk down the dip
            tau_s = INT_MAX;
            for (int base = cross; base <= tau_max && tau_s == INT_MAX; base += 64) {
                const int tau = base + lane;
                const bool stop = tau <= tau_max && (tau == tau_max || !(dp[tau] < dp[tau - 1]));
                tau_s = wave_min_int(stop ? tau : INT_MAX);
            }
        } else {                                                             // unvoiced: the first argmin
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) {
                const float ub = __shfl_xor(best, s, 64);
                const int ut = __shfl_xor(best_tau, s, 64);
                if (ub < best || (ub == best && ut < best_tau)) {
                    best = ub;
                    best_tau = ut;
                }
            }
            tau_s = best_tau == INT_MAX ? tau_min : best_tau;                // (every d' NaN: cannot happen on finite input)
        }
        // energy: the n_fft samples centred at t hop, windowed
        const float* ex = xs + r * hop + half - n_fft / 2;
        float s2 = 0.f, s1 = 0.f, sa = 0.f;
        for (int n = lane; n < n_fft; n += 64) {                             // (64 is even: a lane's samples share the sign)
            const float y = hann[n] * ex[n];
            s2 = fmaf(y, y, s2);
            s1 += y;
        }
        sa = (lane & 1) ? -s1 : s1;
        s2 = wave_sum(s2);
        s1 = wave_sum(s1);
        sa = wave_sum(sa);
        if (lane == 0) {
            const float bq = dp[tau_s - 1];
            float shift = 0.f;
            if (tau_s > tau_min && tau_s < tau_max) {
                const float a = dp[tau_s - 2], c = dp[tau_s];
                const float den = a - 2.f * bq + c;
                if (den > 0.f) {
                    shift = 0.5f * (a - c) / den;
                    shift = shift < -0.5f ? -0.5f : shift > 0.5f ? 0.5f : shift;
                }
            }
            const bool v = cross != INT_MAX;
            const long at = row + t0 + r;
            f0[at] = v ? sample_rate / ((float)tau_s + shift) : 0.f;
            voiced[at] = v ? 1 : 0;
            aper[at] = bq;
            energy[at] = sqrtf(0.5f * (fmaf((float)n_fft, s2, s1 * s1) + sa * sa));
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");               // lane 0 has read dp before the next frame overwrites it
        __builtin_amdgcn_wave_barrier();
    }
}

// One wave per utterance: the exclusive prefix sum of the durations over tiles of 64 phonemes, then lane p adds the frames
// [c_p, c_p + dur_p) clipped to frames_b in ascending order, those with a non-zero mask when one is given.
__global__ __launch_bounds__(64) void segment_mean_kernel(const float* __restrict__ values, long ld_values,
                                                          const int64_t* __restrict__ durations, const int64_t* __restrict__ phoneme_lens,
                                                          const int64_t* __restrict__ frames, const uint8_t* __restrict__ mask,
                                                          long ld_mask, int Tmax, int Pmax, float* __restrict__ mean,
                                                          int32_t* __restrict__ counts) {
    const int b = blockIdx.x, lane = threadIdx.x;
    long fr = frames[b], pl = phoneme_lens[b];
    fr = fr < 0 ? 0 : fr > Tmax ? Tmax : fr;
    pl = pl < 0 ? 0 : pl > Pmax ? Pmax : pl;
    const float* vb = values + (long)b * ld_values;
    const uint8_t* mb = mask ? mask + (long)b * ld_mask : nullptr;
    long carry = 0;
    for (int base = 0; base < Pmax; base += 64) {
        const int p = base + lane;
        long dur = p < pl ? durations[(long)b * Pmax + p] : 0;
        dur = dur < 0 ? 0 : dur > Tmax ? Tmax : dur;                         // (a longer one is clipped to frames_b anyway)
        long cs = dur;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const long u = __shfl_up(cs, s, 64);
            cs = lane >= s ? cs + u : cs;
        }
        cs += carry;
        carry = __shfl(cs, 63, 64);
        if (p < Pmax) {
            long a = cs - dur, e = cs;
            a = a > fr ? fr : a;
            e = e > fr ? fr : e;
            float acc = 0.f;
            int n = 0;
            for (long t = a; t < e; ++t)
                if (!mb || mb[t]) {
                    acc += vb[t];
                    ++n;
                }
            mean[(long)b * Pmax + p] = n > 0 ? acc / (float)n : 0.f;
            counts[(long)b * Pmax + p] = n;
        }
    }
}

}  // namespace ttts

using namespace ttts;

extern "C" {

int ttts_pitch_lags(void) { return PITCH_LAGS; }

int ttts_pitch_frames(int n_fft, int hop, int frame_length, int window, int tau_max) {
    if (n_fft < 2 || hop < 1 || frame_length < 2 || frame_length > PITCH_MAX_F || window < 1 || tau_max < 1 ||
        (long)window + tau_max > frame_length)
        return 0;
    return pitch_plan(frame_length, n_fft, hop, window, tau_max).frames;
}

int ttts_pitch_block(int n_fft, int hop, int frame_length, int window, int tau_max) {
    if (ttts_pitch_frames(n_fft, hop, frame_length, window, tau_max) == 0) return 0;
    return pitch_plan(frame_length, n_fft, hop, window, tau_max).block;
}

int ttts_pitch_energy(const float* wave, int64_t ld_batch, const int64_t* wave_lens, int B, int Nmax, int n_fft, int win_length, int hop,
                      int frame_length, int window, int tau_min, int tau_max, float sample_rate, float threshold, const float* hann,
                      float* f0, uint8_t* voiced, float* aperiodicity, float* energy, int64_t* frames, void* stream) {
    const char* name = "pitch_energy";
    const int F = frame_length, W = window;
    TTTS_REQUIRE(wave && wave_lens && hann && f0 && voiced && aperiodicity && energy && frames, "%s: null pointer", name);
    TTTS_REQUIRE(B >= 1 && B <= 65535, "%s: B must be in [1, 65535] (one grid row per utterance), got %d", name, B);
    TTTS_REQUIRE(Nmax >= 1 && Nmax <= (1 << 30), "%s: Nmax must be in [1, 2^30] samples per utterance, got %d", name, Nmax);
    TTTS_REQUIRE(n_fft == 256 || n_fft == 512 || n_fft == 1024 || n_fft == 2048, "%s: n_fft must be one of 256, 512, 1024, 2048, got %d",
                 name, n_fft);
    TTTS_REQUIRE(win_length >= 1 && win_length <= n_fft, "%s: win_length must be in [1, n_fft] (win_length %d, n_fft %d)", name,
                 win_length, n_fft);
    TTTS_REQUIRE(F >= 2 && (F & 1) == 0 && F <= PITCH_MAX_F, "%s: frame_length must be even and in [2, %d], got %d", name, PITCH_MAX_F, F);
    TTTS_REQUIRE(hop >= 1 && hop <= F, "%s: hop must be in [1, frame_length] (hop %d, frame_length %d)", name, hop, F);
    TTTS_REQUIRE(W >= 1, "%s: window must be positive, got %d", name, W);
    TTTS_REQUIRE(tau_min >= 2, "%s: tau_min must be at least 2 (fmax too high for the sample rate), got %d", name, tau_min);
    TTTS_REQUIRE(tau_min < tau_max, "%s: tau_min must be below tau_max (tau_min %d, tau_max %d)", name, tau_min, tau_max);
    TTTS_REQUIRE((long)W + tau_max <= F, "%s: window + tau_max must fit the frame (window %d, tau_max %d, frame_length %d)", name, W,
                 tau_max, F);
    TTTS_REQUIRE(threshold > 0.f && threshold < 1.f, "%s: threshold must be in (0, 1), got %g", name, (double)threshold);
    TTTS_REQUIRE(sample_rate > 0.f && sample_rate - sample_rate == 0.f, "%s: sample_rate must be positive and finite, got %g", name,
                 (double)sample_rate);
    TTTS_REQUIRE(ld_batch >= Nmax || (B == 1 && ld_batch >= 0), "%s: the batch stride must be >= Nmax (ld_batch %lld, Nmax %d)", name,
                 (long long)ld_batch, Nmax);
    TTTS_REQUIRE(((reinterpret_cast<uintptr_t>(wave) | reinterpret_cast<uintptr_t>(hann) | reinterpret_cast<uintptr_t>(f0) |
                   reinterpret_cast<uintptr_t>(aperiodicity) | reinterpret_cast<uintptr_t>(energy)) & 3) == 0,
                 "%s: wave, hann, f0, aperiodicity and energy must be 4-byte aligned", name);
    TTTS_REQUIRE(((reinterpret_cast<uintptr_t>(wave_lens) | reinterpret_cast<uintptr_t>(frames)) & 7) == 0,
                 "%s: wave_lens and frames must be 8-byte aligned", name);
    const PitchPlan p = pitch_plan(F, n_fft, hop, W, tau_max);
    const int Tmax = 1 + Nmax / hop;
    const dim3 grid((unsigned)cdiv(Tmax, p.frames), (unsigned)B);
    hipLaunchKernelGGL(pitch_energy_kernel, grid, dim3(PITCH_THREADS), p.lds, (hipStream_t)stream, wave, (long)ld_batch, wave_lens, Nmax,
                       n_fft, hop, F, W, tau_min, tau_max, sample_rate, threshold, hann, Tmax, p.frames, p.block, p.nb, p.half, p.span, f0,
                       voiced, aperiodicity, energy, frames);
    TTTS_LAUNCH_CHECK("pitch_energy_kernel");
    return TTTS_OK;
}

int ttts_segment_mean(const float* values, int64_t ld_values, const int64_t* durations, const int64_t* phoneme_lens,
                      const int64_t* frames, const uint8_t* mask, int64_t ld_mask, int B, int Tmax, int Pmax, float* mean,
                      int32_t* counts, void* stream) {
    const char* name = "segment_mean";
    TTTS_REQUIRE(values && durations && phoneme_lens && frames && mean && counts, "%s: null pointer", name);
    TTTS_REQUIRE(B >= 1 && B <= 65535, "%s: B must be in [1, 65535] (one workgroup per utterance), got %d", name, B);
    TTTS_REQUIRE(Tmax >= 1 && Tmax <= (1 << 30), "%s: Tmax must be in [1, 2^30] frames, got %d", name, Tmax);
    TTTS_REQUIRE(Pmax >= 1 && Pmax <= (1 << 20), "%s: Pmax must be in [1, 2^20] phonemes, got %d", name, Pmax);
    TTTS_REQUIRE(ld_values >= Tmax || (B == 1 && ld_values >= 0), "%s: the value stride must be >= Tmax (ld_values %lld, Tmax %d)", name,
                 (long long)ld_values, Tmax);
    TTTS_REQUIRE(!mask || ld_mask >= Tmax || (B == 1 && ld_mask >= 0), "%s: the mask stride must be >= Tmax (ld_mask %lld, Tmax %d)", name,
                 (long long)ld_mask, Tmax);
    TTTS_REQUIRE(((reinterpret_cast<uintptr_t>(values) | reinterpret_cast<uintptr_t>(mean) | reinterpret_cast<uintptr_t>(counts)) & 3) == 0,
                 "%s: values, mean and counts must be 4-byte aligned", name);
    TTTS_REQUIRE(((reinterpret_cast<uintptr_t>(durations) | reinterpret_cast<uintptr_t>(phoneme_lens) |
                   reinterpret_cast<uintptr_t>(frames)) & 7) == 0,
                 "%s: durations, phoneme_lens and frames must be 8-byte aligned", name);
    hipLaunchKernelGGL(segment_mean_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, values, (long)ld_values, durations,
                       phoneme_lens, frames, mask, (long)ld_mask, Tmax, Pmax, mean, counts);
    TTTS_LAUNCH_CHECK("segment_mean_kernel");
    return TTTS_OK;
}

}  // extern "C"
