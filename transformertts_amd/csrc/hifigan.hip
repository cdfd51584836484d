// The HiFi-GAN generator's layers on ragged (B, Nmax, C) fp32 rows (gfx950).  Inference only.
// pl_b = clamp(lens[b], 0, Nmax); rows at or behind pl_b count as zeros for the taps, are never read, and come back as exact zeros.
//   hg_conv_kernel   z[b, n, co] = sum_j sum_ci w[j, ci, co] f(x[b, n + (j - taps / 2) dil, ci]),  f = leaky_relu(., slope) or the identity
//                    (f(0) = 0: the zero padding commutes with it);  v = z + bias[co] + residual[b, n, co];  y = v;  acc = v scale
//                    (set) or (acc + v) scale (add).  An implicit GEMM on v_mfma_f32_32x32x2_f32.  The weight is re-laid once on the
//                    host to (taps, Cin, Cout): a (tap, 32-channel chunk) slab is 32 rows of contiguous output columns.
//                    A workgroup of four waves owns rows of ONE utterance and up to 256 output columns.  A wave owns 64 rows x 64
//                    columns (four 32 x 32 accumulators; 64 x 32 at Cout 32); the waves lie ncw = 4, 2 or 1 along the columns
//                    (Cout >= 256, >= 128, below) and 4 / ncw along the rows, 64 rows each.  The reduction runs over chunks of 32
//                    input channels and inside a chunk over the taps, both ascending; a chunk of x (its rows and the halo of (taps - 1) dil rows) is staged once for all
//                    taps, the weight slab of the next (chunk, tap) is in flight in registers while one is multiplied out of LDS.
//                    The fma chain is closed after every (chunk, tap): 32 products, then one fp32 add into the running sum, in
//                    ascending order.  A ConvTranspose1d (stride u, taps k, u <= k <= 2 u) runs here as a 3-tap convolution onto
//                    u Cout columns: (B, T, u Cout) row-major is (B, T u, Cout) row-major.
//   hg_post_kernel   y[b, n] = tanh(bias + sum_j sum_ci w[j, ci] leaky_relu(x[b, n + j - taps / 2, ci], slope)): one output per row, a
//                    thread per row on the VALU, the rows of a workgroup staged in LDS per 32-channel chunk; the chain closed per
//                    chunk, the chunks' sums added in ascending order.
// No atomics, no allocation, no host read; the workgroup's tiling depends on the shape alone, so an utterance alone has the bits
// it has in a batch, and every call gives the same bits.
#include "ttts_common.h"

#include <math.h>

namespace ttts {

constexpr int HG_THREADS = 256;
constexpr int HG_WAVES = HG_THREADS / 64;
constexpr int HG_KC = 32;                  // input channels of a chunk
constexpr int HG_XP = 33;                  // odd pitch: the 32 rows an MFMA operand reads fall into 32 banks
constexpr int HG_MAX_TAPS = 11;
constexpr int HG_MAX_DIL = 12;
constexpr int HG_MAX_CIN = 512;
constexpr int HG_MAX_COUT = 2048;          // u Cout of an upsampler
constexpr int HG_MAX_ROWS = 1 << 21;       // 4096 frames x a hop of 512
constexpr int HG_POST_ROWS = 256;

__device__ __forceinline__ int hg_clamp_len(long v, int hi) { return v < 0 ? 0 : v > hi ? hi : (int)v; }
__device__ __forceinline__ float hg_lrelu(float v, float slope) { return v > 0.f ? v : __fmul_rn(v, slope); }

static inline int hg_ncw(int Cout) { return Cout >= 256 ? 4 : Cout >= 128 ? 2 : 1; }
static inline size_t hg_round4(size_t n) { return (n + 3) & ~(size_t)3; }
// the pitch of a weight row in LDS: its two k-rows of an MFMA operand fall into the two halves of the 64 banks
__host__ __device__ static inline int hg_wpitch(int CB) { return (CB + 32) | 32; }
static inline size_t hg_conv_lds_bytes(int ncw, int CB, int taps, int dil) {
    const size_t rows = (size_t)64 * (HG_WAVES / ncw) + (size_t)(taps - 1) * dil;
    return (hg_round4(rows * HG_XP) + (size_t)HG_KC * hg_wpitch(CB)) * sizeof(float);
}

struct HgConvArgs {
    const float* x; const int64_t* lens; const float* w; const float* bias; const float* res;
    float* y; float* acc;
    int Nmax, Cin, Cout, taps, dil, ncw, acc_mode;
    float slope, scale;
};

template <int CT>                                                            // 32-column tiles of a wave: 2, or 1 at Cout 32
__global__ __launch_bounds__(HG_THREADS) void hg_conv_kernel(const HgConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) float hg_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, lr = lane & 31;
    const int ncw = a.ncw, nrg = HG_WAVES / ncw, RB = 64 * nrg, CB = 32 * CT * ncw, WP = hg_wpitch(CB);
    const int cb = wave % ncw, rg = wave / ncw;
    const int Nmax = a.Nmax, Cin = a.Cin, Cout = a.Cout, taps = a.taps, dil = a.dil;
    const int b = blockIdx.y, p0 = blockIdx.x * RB, n0 = blockIdx.z * CB;
    const int pl = hg_clamp_len(a.lens[b], Nmax);
    const int rows = Nmax - p0 < RB ? Nmax - p0 : RB;
    const int ncols = Cout - n0 < CB ? Cout - n0 : CB;                       // a multiple of 32
    const long row0 = (long)b * Nmax + p0;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    if (p0 >= pl) {                                                          // wholly behind the length: zeros, nothing read
        const int n4 = ncols >> 2;
        for (int i = tid; i < rows * n4; i += HG_THREADS) {
            const int rr = i / n4, c4 = i - rr * n4;
            const long at = (row0 + rr) * Cout + n0 + 4 * c4;
            if (a.y) *reinterpret_cast<float4*>(a.y + at) = zero4;
            if (a.acc_mode) *reinterpret_cast<float4*>(a.acc + at) = zero4;
        }
        return;
    }

    const int nxrows = RB + (taps - 1) * dil;
    float* Xs = hg_lds;
    float* Ws = hg_lds + ((nxrows * HG_XP + 3) & ~3);
    const int xrow0 = p0 - (taps >> 1) * dil;
    const float* xb = a.x + (long)b * Nmax * Cin;
    const float slope = a.slope;
    const bool act = slope != 1.f;
    const int c0 = n0 + 32 * CT * cb;                                        // this wave's first column
    const int rbase = rg * 64;
    bool live[2][CT];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) live[rt][ct] = c0 + 32 * ct < Cout && p0 + rbase + rt * 32 < pl;

    f32x16 acc[2][CT], tot[2][CT];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[rt][ct][i] = tot[rt][ct][i] = 0.f;

    const int cb4 = CB >> 2, nwr = CB >> 5;                                  // float4 of a slab a thread holds: 32 CB / 4 / 256
    constexpr int WR = 4 * CT;
    float4 wr[WR];
    auto load_w = [&](int ci0, int j) {                                      // w[j][ci0 .. ci0 + 32)[n0 .. n0 + CB): rows of contiguous columns
#pragma unroll
        for (int u = 0; u < WR; ++u) {
            wr[u] = zero4;
            if (u < nwr) {
                const int i = tid + u * HG_THREADS, k = i / cb4, c4 = i - k * cb4;
                if (ci0 + k < Cin && 4 * c4 < ncols)
                    wr[u] = *reinterpret_cast<const float4*>(a.w + ((long)j * Cin + ci0 + k) * Cout + n0 + 4 * c4);
            }
        }
    };
    auto store_w = [&]() {
#pragma unroll
        for (int u = 0; u < WR; ++u)
            if (u < nwr) {
                const int i = tid + u * HG_THREADS, k = i / cb4, c4 = i - k * cb4;
                *reinterpret_cast<float4*>(Ws + k * WP + 4 * c4) = wr[u];
            }
    };
    auto stage_x = [&](int ci0) {                                            // rows xrow0 .. xrow0 + nxrows of f(x'), channels ci0 .. ci0 + 32
        for (int i = tid; i < nxrows * (HG_KC / 4); i += HG_THREADS) {
            const int rr = i >> 3, c4 = i & 7;
            const int p = xrow0 + rr, ci = ci0 + 4 * c4;
            float4 v = zero4;
            if (p >= 0 && p < pl && ci < Cin) {
                v = *reinterpret_cast<const float4*>(xb + (long)p * Cin + ci);
                if (act) { v.x = hg_lrelu(v.x, slope); v.y = hg_lrelu(v.y, slope); v.z = hg_lrelu(v.z, slope); v.w = hg_lrelu(v.w, slope); }
            }
            float* s = Xs + rr * HG_XP + 4 * c4;
            s[0] = v.x; s[1] = v.y; s[2] = v.z; s[3] = v.w;
        }
    };

    const float* wbp = Ws + half * WP + cb * CT * 32 + lr;
    load_w(0, 0);
    for (int ci0 = 0; ci0 < Cin; ci0 += HG_KC)
        for (int j = 0; j < taps; ++j) {
            __syncthreads();                                                 // the last multiply has left Xs and Ws
            if (j == 0) stage_x(ci0);
            store_w();
            __syncthreads();
            if (j + 1 < taps) load_w(ci0, j + 1);
            else if (ci0 + HG_KC < Cin) load_w(ci0 + HG_KC, 0);
            const float* xa = Xs + (rbase + lr + j * dil) * HG_XP + half;
#pragma unroll
            for (int k = 0; k < HG_KC; k += 2) {
                float av[2], bv[CT];
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) av[rt] = xa[rt * 32 * HG_XP + k];
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) bv[ct] = wbp[k * WP + 32 * ct];
#pragma unroll
                for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct)
                        if (live[rt][ct]) acc[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[rt], bv[ct], acc[rt][ct], 0, 0, 0);
            }
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        tot[rt][ct][i] = __fadd_rn(tot[rt][ct][i], acc[rt][ct][i]);
                        acc[rt][ct][i] = 0.f;
                    }
        }

#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        const int c = c0 + 32 * ct + lr;
        if (c0 + 32 * ct >= Cout) continue;
        const float bias = a.bias ? a.bias[c] : 0.f;
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int rr = rbase + rt * 32 + acc_row(i, half);
                if (rr >= rows) continue;
                const bool valid = p0 + rr < pl;
                const long at = (row0 + rr) * Cout + c;
                float v = 0.f;
                if (valid) {
                    v = __fadd_rn(tot[rt][ct][i], bias);
                    if (a.res) v = __fadd_rn(v, a.res[at]);
                }
                if (a.y) a.y[at] = v;
                if (a.acc_mode == 1) a.acc[at] = valid ? __fmul_rn(v, a.scale) : 0.f;
                else if (a.acc_mode == 2) a.acc[at] = valid ? __fmul_rn(__fadd_rn(a.acc[at], v), a.scale) : 0.f;
            }
    }
}

__global__ __launch_bounds__(HG_POST_ROWS) void hg_post_kernel(const float* __restrict__ x, const int64_t* __restrict__ lens,
                                                               const float* __restrict__ w, const float* __restrict__ bias,
                                                               float* __restrict__ y, int Nmax, int Cin, int taps, float slope) {
    __shared__ float Xs[(HG_POST_ROWS + HG_MAX_TAPS - 1) * HG_XP];
    __shared__ float Wsh[HG_MAX_TAPS * HG_KC];
    const int tid = threadIdx.x, b = blockIdx.y, p0 = blockIdx.x * HG_POST_ROWS, p = p0 + tid;
    const int pl = hg_clamp_len(lens[b], Nmax);
    if (p0 >= pl) {                                                          // wholly behind the length: zeros, nothing read
        if (p < Nmax) y[(long)b * Nmax + p] = 0.f;
        return;
    }
    const int nxrows = HG_POST_ROWS + taps - 1, xrow0 = p0 - (taps >> 1);
    const float* xb = x + (long)b * Nmax * Cin;
    float tot = 0.f;
    for (int ci0 = 0; ci0 < Cin; ci0 += HG_KC) {
        __syncthreads();
        for (int i = tid; i < nxrows * (HG_KC / 4); i += HG_POST_ROWS) {
            const int rr = i >> 3, c4 = i & 7;
            const int q = xrow0 + rr, ci = ci0 + 4 * c4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (q >= 0 && q < pl && ci < Cin) {
                v = *reinterpret_cast<const float4*>(xb + (long)q * Cin + ci);
                v.x = hg_lrelu(v.x, slope); v.y = hg_lrelu(v.y, slope); v.z = hg_lrelu(v.z, slope); v.w = hg_lrelu(v.w, slope);
            }
            float* s = Xs + rr * HG_XP + 4 * c4;
            s[0] = v.x; s[1] = v.y; s[2] = v.z; s[3] = v.w;
        }
        for (int i = tid; i < taps * HG_KC; i += HG_POST_ROWS) {
            const int j = i >> 5, k = i & 31;
            Wsh[i] = ci0 + k < Cin ? w[(long)j * Cin + ci0 + k] : 0.f;
        }
        __syncthreads();
        float acc = 0.f;
        for (int j = 0; j < taps; ++j) {
            const float* xr = Xs + (tid + j) * HG_XP;
#pragma unroll
            for (int k = 0; k < HG_KC; ++k) acc = __fmaf_rn(xr[k], Wsh[j * HG_KC + k], acc);
        }
        tot = __fadd_rn(tot, acc);
    }
    if (p < Nmax) y[(long)b * Nmax + p] = p < pl ? tanhf(__fadd_rn(tot, bias[0])) : 0.f;
}

static inline bool hg_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace ttts

using namespace ttts;

extern "C" {

int ttts_hifigan_max_operand_bytes(void) { return 0x7fffffff; }

int ttts_hifigan_conv(const float* x, const int64_t* lens, const float* w, const float* bias, const float* residual, float* y,
                      float* acc, int B, int Nmax, int Cin, int Cout, int taps, int dilation, float in_slope, int acc_mode,
                      float acc_scale, void* stream) {
    const char* name = "hifigan_conv";
    TTTS_REQUIRE(x && lens && w, "%s: null pointer", name);
    TTTS_REQUIRE(acc_mode >= 0 && acc_mode <= 2, "%s: acc_mode must be 0 (none), 1 (set) or 2 (add), got %d", name, acc_mode);
    TTTS_REQUIRE((acc_mode != 0) == (acc != nullptr), "%s: acc goes with acc_mode 1 or 2 and with nothing else", name);
    TTTS_REQUIRE(y || acc, "%s: null pointer (one of y and acc is needed)", name);
    TTTS_REQUIRE(B >= 1 && B <= 65535, "%s: B must be in [1, 65535] (one grid row per utterance), got %d", name, B);
    TTTS_REQUIRE(Nmax >= 1 && Nmax <= HG_MAX_ROWS, "%s: Nmax must be in [1, %d] rows, got %d", name, HG_MAX_ROWS, Nmax);
    TTTS_REQUIRE((Cin % 32 == 0 && Cin >= 32 && Cin <= HG_MAX_CIN) || (Cin % 4 == 0 && Cin >= 4 && Cin <= 128),
                 "%s: Cin must be a multiple of 32 in [32, %d] or a multiple of 4 in [4, 128], got %d", name, HG_MAX_CIN, Cin);
    TTTS_REQUIRE(Cout % 32 == 0 && Cout >= 32 && Cout <= HG_MAX_COUT, "%s: Cout must be a multiple of 32 in [32, %d], got %d", name,
                 HG_MAX_COUT, Cout);
    TTTS_REQUIRE(taps >= 1 && taps <= HG_MAX_TAPS && (taps & 1), "%s: taps must be odd in [1, %d], got %d", name, HG_MAX_TAPS, taps);
    TTTS_REQUIRE(dilation >= 1 && dilation <= HG_MAX_DIL, "%s: dilation must be in [1, %d], got %d", name, HG_MAX_DIL, dilation);
    TTTS_REQUIRE(in_slope - in_slope == 0.f && acc_scale - acc_scale == 0.f, "%s: in_slope and acc_scale must be finite, got %g and %g",
                 name, (double)in_slope, (double)acc_scale);
    TTTS_REQUIRE((uint64_t)B * Nmax * (Cin > Cout ? Cin : Cout) * sizeof(float) <= (uint64_t)ttts_hifigan_max_operand_bytes(),
                 "%s: an operand may hold up to %d bytes (B %d, Nmax %d, Cin %d, Cout %d): split the batch", name,
                 ttts_hifigan_max_operand_bytes(), B, Nmax, Cin, Cout);
    TTTS_REQUIRE(hg_aligned(x, 16) && hg_aligned(w, 16) && hg_aligned(y, 16) && hg_aligned(acc, 16) && hg_aligned(residual, 16),
                 "%s: x, w, y, acc and residual must be 16-byte aligned", name);
    TTTS_REQUIRE(hg_aligned(bias, 4) && hg_aligned(lens, 8), "%s: bias must be 4-byte and lens 8-byte aligned", name);
    TTTS_REQUIRE(y != x && acc != x, "%s: the output may not be the input (the taps read its neighbours)", name);
    HgConvArgs a;
    a.x = x; a.lens = lens; a.w = w; a.bias = bias; a.res = residual; a.y = y; a.acc = acc;
    a.Nmax = Nmax; a.Cin = Cin; a.Cout = Cout; a.taps = taps; a.dil = dilation; a.ncw = hg_ncw(Cout); a.acc_mode = acc_mode;
    a.slope = in_slope; a.scale = acc_scale;
    const int CT = Cout >= 64 ? 2 : 1, CB = 32 * CT * a.ncw, RB = 64 * (HG_WAVES / a.ncw);
    const dim3 grid((unsigned)cdiv(Nmax, RB), (unsigned)B, (unsigned)cdiv(Cout, CB));
    const size_t lds = hg_conv_lds_bytes(a.ncw, CB, taps, dilation);
    if (CT == 2) hipLaunchKernelGGL(hg_conv_kernel<2>, grid, dim3(HG_THREADS), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(hg_conv_kernel<1>, grid, dim3(HG_THREADS), lds, (hipStream_t)stream, a);
    TTTS_LAUNCH_CHECK("hg_conv_kernel");
    return TTTS_OK;
}

int ttts_hifigan_post(const float* x, const int64_t* lens, const float* w, const float* bias, float* y, int B, int Nmax, int Cin,
                      int taps, float in_slope, void* stream) {
    const char* name = "hifigan_post";
    TTTS_REQUIRE(x && lens && w && bias && y, "%s: null pointer", name);
    TTTS_REQUIRE(B >= 1 && B <= 65535, "%s: B must be in [1, 65535] (one grid row per utterance), got %d", name, B);
    TTTS_REQUIRE(Nmax >= 1 && Nmax <= HG_MAX_ROWS, "%s: Nmax must be in [1, %d] rows, got %d", name, HG_MAX_ROWS, Nmax);
    TTTS_REQUIRE(Cin % 32 == 0 && Cin >= 32 && Cin <= HG_MAX_CIN, "%s: Cin must be a multiple of 32 in [32, %d], got %d", name,
                 HG_MAX_CIN, Cin);
    TTTS_REQUIRE(taps >= 1 && taps <= HG_MAX_TAPS && (taps & 1), "%s: taps must be odd in [1, %d], got %d", name, HG_MAX_TAPS, taps);
    TTTS_REQUIRE(in_slope - in_slope == 0.f, "%s: in_slope must be finite, got %g", name, (double)in_slope);
    TTTS_REQUIRE((uint64_t)B * Nmax * Cin * sizeof(float) <= (uint64_t)ttts_hifigan_max_operand_bytes(),
                 "%s: an operand may hold up to %d bytes (B %d, Nmax %d, Cin %d): split the batch", name,
                 ttts_hifigan_max_operand_bytes(), B, Nmax, Cin);
    TTTS_REQUIRE(hg_aligned(x, 16) && hg_aligned(w, 4) && hg_aligned(bias, 4) && hg_aligned(y, 4) && hg_aligned(lens, 8),
                 "%s: x must be 16-byte, lens 8-byte, w, bias and y 4-byte aligned", name);
    hipLaunchKernelGGL(hg_post_kernel, dim3((unsigned)cdiv(Nmax, HG_POST_ROWS), (unsigned)B), dim3(HG_POST_ROWS), 0, (hipStream_t)stream,
                       x, lens, w, bias, y, Nmax, Cin, taps, in_slope);
    TTTS_LAUNCH_CHECK("hg_post_kernel");
    return TTTS_OK;
}

}  // extern "C"
