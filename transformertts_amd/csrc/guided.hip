// Guided attention loss on the decoder's alignment maps (gfx950): the soft diagonal prior of Transformer-TTS recipes,
//   W_b[t][n] = 1 - exp(-(n / N_b - t / T_b)^2 / (2 sigma^2))   for t < T_b, n < N_b, 0 elsewhere,
//   loss = sum over the selected maps of sum A o W / (n_selected * sum_b T_b N_b),
// with T_b = melspec_lens[b], N_b = phoneme_lens[b] (clamped to the maps' extent).  The normaliser is formed on the device from
// the lengths, the upstream gradient is read from device memory: no host read, so forward and backward capture into a HIP graph.
// Sums: one wave per map row in a fixed lane order and xor tree, then ONE workgroup over the row partials in a fixed order -- no
// atomics, the same bits on every run.
#include "ttts_common.h"

namespace ttts {

__device__ __forceinline__ int guided_len(const int64_t* lens, int b, int cap) {
    long v = lens[b];
    return (int)(v < 0 ? 0 : v > cap ? cap : v);
}
// -expm1f(-x), not 1 - expf(-x): next to the diagonal x is tiny and the weight keeps its relative accuracy
__device__ __forceinline__ float guided_weight(int t, int n, float inv_T, float inv_N, float inv_2s2) {
    const float d = (float)n * inv_N - (float)t * inv_T;
    return -expm1f(-(d * d) * inv_2s2);
}
__device__ __forceinline__ bool guided_head_on(uint64_t head_mask, int h) { return head_mask == 0 || ((head_mask >> h) & 1u); }
// sum_b T_b N_b, by every thread alike (B is a batch size: a short loop over 16 bytes per utterance)
__device__ __forceinline__ float guided_positions(const int64_t* plens, const int64_t* mlens, int B, int Tm, int Tp) {
    long tot = 0;
    for (int b = 0; b < B; ++b) tot += (long)guided_len(mlens, b, Tm) * guided_len(plens, b, Tp);
    return (float)tot;
}

// partials[row] = sum_n A[row][n] W_b[t][n] of one (b, h, t) row; 0 for an unselected head or a row past T_b
__global__ __launch_bounds__(256) void guided_rows_kernel(const float* attn, const int64_t* plens, const int64_t* mlens,
                                                          uint64_t head_mask, float inv_2s2, int H, int Tm, int Tp, long rows,
                                                          float* partials) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int t = (int)(row % Tm), h = (int)((row / Tm) % H), b = (int)(row / ((long)Tm * H));
    const int T = guided_len(mlens, b, Tm), N = guided_len(plens, b, Tp);
    float acc = 0.f;
    if (t < T && guided_head_on(head_mask, h)) {
        const float inv_T = 1.f / (float)T, inv_N = 1.f / (float)N;
        const float* ar = attn + row * Tp;
        for (int n = lane; n < N; n += 64) acc = fmaf(ar[n], guided_weight(t, n, inv_T, inv_N, inv_2s2), acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) partials[row] = acc;
}

// loss = (sum of the n partials, thread j taking j, j + 256, ... and the 256 sums meeting in a fixed tree) / (n_selected sum T N)
__global__ __launch_bounds__(256) void guided_final_kernel(const float* partials, long n, const int64_t* plens, const int64_t* mlens,
                                                           int B, int Tm, int Tp, float n_selected, float* loss) {
    __shared__ float part[256];
    float acc = 0.f;
    for (long i = threadIdx.x; i < n; i += 256) acc += partials[i];
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float norm = n_selected * guided_positions(plens, mlens, B, Tm, Tp);
        *loss = norm > 0.f ? part[0] / norm : 0.f;
    }
}

// d_attn[plane][t][n] = g W_b[t][n] / (n_selected sum T N), exact zeros past the lengths, in the padding columns and in
// unselected heads; planes = B (head_mask 0: one plane serves every head) or B * H
__global__ __launch_bounds__(256) void guided_bwd_kernel(const float* g, const int64_t* plens, const int64_t* mlens, uint64_t head_mask,
                                                         float inv_2s2, float n_selected, int B, int H, int Tm, int Tp, int ld,
                                                         float* d_attn) {
    const long row = blockIdx.x;                       // plane * Tm + t
    const int t = (int)(row % Tm);
    const long plane = row / Tm;
    const int b = head_mask ? (int)(plane / H) : (int)plane, h = head_mask ? (int)(plane % H) : 0;
    const int T = guided_len(mlens, b, Tm), N = guided_len(plens, b, Tp);
    const float norm = n_selected * guided_positions(plens, mlens, B, Tm, Tp);
    const float gs = norm > 0.f ? *g / norm : 0.f;
    const bool on = t < T && guided_head_on(head_mask, h);
    const float inv_T = 1.f / (float)(T > 0 ? T : 1), inv_N = 1.f / (float)(N > 0 ? N : 1);
    for (int n = threadIdx.x; n < ld; n += 256)
        d_attn[row * ld + n] = (on && n < N) ? gs * guided_weight(t, n, inv_T, inv_N, inv_2s2) : 0.f;
}

static int guided_check(const char* name, const void* plens, const void* mlens, uint64_t head_mask, float sigma, int n_selected, int B,
                        int H, int Tm, int Tp) {
    TTTS_REQUIRE(plens && mlens, "%s: null pointer", name);
    TTTS_REQUIRE(B > 0 && H > 0 && Tm > 0 && Tp > 0, "%s: sizes must be positive (B %d, H %d, Tm %d, Tp %d)", name, B, H, Tm, Tp);
    TTTS_REQUIRE(sigma > 0.f, "%s: sigma %g must be positive", name, (double)sigma);
    TTTS_REQUIRE(n_selected > 0, "%s: n_selected %d must be positive", name, n_selected);
    TTTS_REQUIRE(head_mask == 0 || H <= 64, "%s: a head selection takes at most 64 heads (H %d)", name, H);
    TTTS_REQUIRE(head_mask == 0 || H == 64 || (head_mask >> H) == 0, "%s: head_mask %#llx selects a head past H %d", name,
                 (unsigned long long)head_mask, H);
    return TTTS_OK;
}

}  // namespace ttts

using namespace ttts;

extern "C" {

int ttts_guided_attention_fwd(const float* attn, const int64_t* phoneme_lens, const int64_t* melspec_lens, uint64_t head_mask,
                              float sigma, int B, int H, int Tm, int Tp, float* partials, int map_index, int n_maps, int n_selected,
                              float* loss_out, void* stream) {
    TTTS_REQUIRE(attn && partials, "guided_attention_fwd: null pointer");
    int rc = guided_check("guided_attention_fwd", phoneme_lens, melspec_lens, head_mask, sigma, n_selected, B, H, Tm, Tp);
    if (rc) return rc;
    TTTS_REQUIRE(n_maps > 0 && map_index >= 0 && map_index < n_maps, "guided_attention_fwd: map_index %d is outside [0, n_maps %d)",
                 map_index, n_maps);
    const long rows = (long)B * H * Tm;
    TTTS_REQUIRE(rows < (1L << 32), "guided_attention_fwd: grid too large (B*H*Tm %ld)", rows);
    const float inv_2s2 = 1.f / (2.f * sigma * sigma);
    hipLaunchKernelGGL(guided_rows_kernel, dim3((unsigned)cdiv(rows, 4L)), dim3(256), 0, (hipStream_t)stream, attn, phoneme_lens,
                       melspec_lens, head_mask, inv_2s2, H, Tm, Tp, rows, partials + (long)map_index * rows);
    TTTS_LAUNCH_CHECK("guided_rows_kernel");
    if (loss_out) {
        hipLaunchKernelGGL(guided_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, (long)n_maps * rows, phoneme_lens,
                           melspec_lens, B, Tm, Tp, (float)n_selected, loss_out);
        TTTS_LAUNCH_CHECK("guided_final_kernel");
    }
    return TTTS_OK;
}

int ttts_guided_attention_bwd(const float* g_loss, const int64_t* phoneme_lens, const int64_t* melspec_lens, uint64_t head_mask,
                              float sigma, int n_selected, int B, int H, int Tm, int Tp, int ld, float* d_attn, void* stream) {
    TTTS_REQUIRE(g_loss && d_attn, "guided_attention_bwd: null pointer");
    int rc = guided_check("guided_attention_bwd", phoneme_lens, melspec_lens, head_mask, sigma, n_selected, B, H, Tm, Tp);
    if (rc) return rc;
    TTTS_REQUIRE(ld >= Tp && ld % 4 == 0, "guided_attention_bwd: the row stride must be a multiple of 4 floats and >= Tp (ld %d, Tp %d)",
                 ld, Tp);
    const long rows = (long)B * (head_mask ? H : 1) * Tm;
    TTTS_REQUIRE(rows < (1L << 31), "guided_attention_bwd: grid too large (%ld rows)", rows);
    const float inv_2s2 = 1.f / (2.f * sigma * sigma);
    hipLaunchKernelGGL(guided_bwd_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, g_loss, phoneme_lens, melspec_lens,
                       head_mask, inv_2s2, (float)n_selected, B, H, Tm, Tp, ld, d_attn);
    TTTS_LAUNCH_CHECK("guided_bwd_kernel");
    return TTTS_OK;
}

}  // extern "C"
