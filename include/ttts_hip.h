/* ttts_hip.h -- C ABI of libttts_hip.so: hand-written gfx950 (MI355X / CDNA4) HIP kernels for the
 * teacher-forced Transformer-TTS forward/backward hot path.
 *
 * The reference (Orca0917/TransformerTTS, /root/reference) has no FFI of its own: it is pure Python
 * and delegates its arithmetic to stock torch ops.  Each entry point below therefore names the torch
 * call site in the reference that it replaces (file:line relative to /root/reference;
 * "torch/..." = the un-vendored PyTorch the reference runs on).
 *
 * Conventions:
 *   - plain pointers + sizes only; activations are row-major contiguous (B,T,C) fp32, weights keep the
 *     state-dict layouts ((out,in) linear, (Cout,Cin,K) conv, packed (3d,d) in-proj); lengths are int64.
 *   - every function only ENQUEUES work on `stream` (a hipStream_t passed as void*); no device allocation, no
 *     synchronisation, no state that outlives the call: workspaces are owned by the caller, and so is the one host-side
 *     object of the ABI, the deferred-reduction queue (ttts_reduce_queue).  The library reads no environment variables.
 *     Calls are re-entrant from several host threads on different streams (different queues, different workspaces).
 *   - return 0 on success, a negative TTTS_ERR_* otherwise (never throws / exits);
 *     ttts_last_error() returns a thread-local message for the last failure.
 *   - dropout masks are a pure function of (seed, flat element index), so backward entry points
 *     regenerate the forward mask from the same seed; p = 0 disables dropout.
 *   - HIP-graph replay: kernel arguments are frozen when a graph is captured, so everything that changes from step to
 *     step can ALSO be read from a small block of device memory (ttts_step_state): every `seed` argument is
 *     accompanied by `step_seed` (NULL, or a device pointer whose 64-bit word is XORed into the seed when the kernel
 *     runs -- &state->seed), and the optimizer / scheduled-sampling entry points take the state block itself.
 *     The caller refreshes the block with one small host-to-device copy per step, outside the graph.
 */
#ifndef TTTS_HIP_H
#define TTTS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TTTS_OK 0
#define TTTS_ERR_INVALID (-1) /* bad argument (shape, alignment, null pointer) */
#define TTTS_ERR_LAUNCH (-2)  /* hipLaunchKernel reported an error */

/* length of every partial-maxima array (`*_amax`, `*_amax_out`) of this header, in floats */
#define TTTS_AMAX_SLOTS 1024

#define TTTS_ACT_NONE 0
#define TTTS_ACT_RELU 1
#define TTTS_ACT_TANH 2

/* Per-step scalars a captured graph reads from device memory (32 bytes, fields at fixed offsets). */
typedef struct ttts_step_state {
    uint64_t seed;    /*  0: XORed into every dropout / sampling site seed of the step */
    float lr;         /*  8: Adam learning rate of this step (base lr x Noam factor) */
    float p_tf;       /* 12: teacher-forcing ratio of this step (utils/util.py:54-92) */
    int64_t step;     /* 16: 1-based optimizer step count (Adam bias correction) */
    int64_t reserved; /* 24 */
} ttts_step_state;

/* Per-frame scalars of autoregressive decoding (32 bytes, fields at fixed offsets), read by every ttts_decode_* kernel when it
 * runs: one captured graph of a chunk of frames then serves every frame, every max_len up to the buffers' capacity and every
 * threshold.  The caller resets it with one small host-to-device copy per call: t = 1, t_end = max_len (the buffers hold
 * t_end rows of frames), stop_frame = -1.  ttts_decode_frame_out records the first frame at which every row's stop
 * probability reaches the threshold in stop_frame, then advances t.  Every decode kernel returns at once when
 * t >= t_end or stop_frame >= 0.
 * Per-row state (ABI v16): the ttts_decode_*_rows entry points also take `row_end`, B int64 on the device (allocated up to a
 * multiple of 4 entries), reset to -1 by the
 * same copy when it is laid out right behind the state: row_end[b] > 0 is the frame at which utterance b ended, anything else
 * says it is still running.  With TTTS_DECODE_PER_ROW in `flags`, ttts_decode_frame_out_rows latches row_end[b] = t the first
 * time row b reaches the threshold and sets stop_frame at the frame that leaves no row running. */
#define TTTS_DECODE_PER_ROW 1
typedef struct ttts_decode_state {
    int64_t t;            /*  0: the frame being decoded (1-based: frame t is written to ys[:, t], frame 0 is the go frame) */
    int64_t t_end;        /*  8: max_len */
    int64_t stop_frame;   /* 16: first all-stop frame, -1 until one occurs */
    float stop_threshold; /* 24: stop when sigmoid(stop logit) >= threshold for every row */
    int32_t flags;        /* 28: TTTS_DECODE_PER_ROW or 0; read by ttts_decode_frame_out_rows only */
} ttts_decode_state;

/* Attention window of one decoder layer's cross-attention at synthesis (ABI v21; 32 bytes, fields at fixed offsets), read by
 * ttts_decode_attention_window when it runs: which heads are constrained, how far they see and which head moves the window
 * are data, so one captured graph serves every window. */
typedef struct ttts_decode_window {
    int32_t back;         /*  0: keys behind the position a constrained head still sees (>= 0) */
    int32_t ahead;        /*  4: keys ahead of it (>= 0) */
    int32_t guide_head;   /*  8: the head whose largest in-window score becomes the next position; -1: none in this layer */
    int32_t pad;          /* 12 */
    uint64_t head_mask;   /* 16: bit h set: head h is constrained */
    int64_t reserved;     /* 24 */
} ttts_decode_window;

const char* ttts_last_error(void);
int ttts_abi_version(void);

/* ---- deferred second-stage reductions ---------------------------------------------------------------------------
 * The weight-gradient (linear / conv1d / rowdot) and LayerNorm-backward entry points end in a small reduction of
 * their split-K or per-block partials into the parameter gradient -- ~90 launches of a few microseconds each per training
 * step.  They take a `queue` argument: NULL launches the reduction at once; a queue created by the caller makes the
 * entry point append a descriptor to it instead, and ttts_reduce_queue_flush runs everything appended so far in one
 * launch per 48 entries (same summation order as the immediate form, bit for bit).  Until the flush has been enqueued on
 * the same stream the caller must keep every workspace (`ws`) it passed alive and must not read those gradients.
 * The queue is host memory owned by its creator; the library keeps no queue of its own.  Appending (from whichever
 * thread runs the backward node) and flushing are safe against each other; two independent backward passes use two
 * queues.  clear drops what is queued (after a failed pass). */
typedef struct ttts_reduce_queue ttts_reduce_queue;
ttts_reduce_queue* ttts_reduce_queue_create(void);
void ttts_reduce_queue_destroy(ttts_reduce_queue* queue);
int64_t ttts_reduce_queue_pending(ttts_reduce_queue* queue);
int ttts_reduce_queue_flush(ttts_reduce_queue* queue, void* stream);
int ttts_reduce_queue_clear(ttts_reduce_queue* queue);

/* ------------------------------------------------------------------ linear (nn.Linear / LinearNorm)
 * y[M,N] = drop(act(x[M,K] . w[N,K]^T + bias)) + residual          K % 16 == 0
 * Replaces: LinearNorm.forward (model/module.py:52-53); MHA in/out projections
 * (torch/nn/functional.py:6206+ in_proj, out_proj); FFN `_ff_block`
 * (torch/nn/modules/transformer.py:980-982,1197-1199) incl. its ReLU, Dropout and the residual add
 * of model/layers.py:47-50; DecoderPreNet (model/model.py:65-66).
 * row_shift = -1 with T = frames per utterance folds the go-frame shift of model/model.py:278-279
 * into the loader (row (b,t) reads x[b,t-1], zeros at t = 0). */
int ttts_linear_fwd(const float* x, const float* w, const float* bias, const float* residual, float* y, int64_t M,
                    int N, int K, int act, float drop_p, uint64_t seed, const uint64_t* step_seed, int row_shift, int T,
                    void* stream);
/* dx[M,K] = gate * (dy[M,N] . w[N,K]) + residual[M,K]               N % 16 == 0, K % 4 == 0
 * residual may be NULL.  relu_out (NULL or (M,K)): the forward value of the activation dx is the gradient of, when that
 * activation is drop(relu(.)) of a preceding Linear (model/module.py:76-80 prenet, the torch FFN block): gate =
 * relu_out > 0 ? relu_scale : 0 with relu_scale = 1/(1-p) -- the relu / dropout backward mask in the epilogue. */
int ttts_linear_bwd_data(const float* dy, const float* w, const float* residual, float* dx, int64_t M, int N, int K,
                         const float* relu_out, float relu_scale, void* stream);
/* dw[N,K] = dy[M,N]^T . x[M,K] (x rows shifted as in forward); dbias[N] = column sums of dy (optional).
 * Every parameter-gradient output in this header takes `accumulate`: 0 stores, 1 adds to what is there, so that
 * gradients can land directly in slices of one flat, pre-zeroed gradient buffer (the data-parallel bucket).
 * ttts_wgrad_workspace_bytes: the workspace of the problem in every form (fp32, _x6, _h3, _h3_parts; taps > 1: the Conv1d entries
 * with M = B T, N = cout, K = cin) and as a member of any ttts_wgrad_group; 0 for a dimension that is not positive. */
size_t ttts_wgrad_workspace_bytes(int64_t M, int N, int K, int taps);
int ttts_linear_bwd_weight(const float* dy, const float* x, float* dw, float* dbias, float* ws, size_t ws_bytes,
                           int64_t M, int N, int K, int row_shift, int T, int accumulate, ttts_reduce_queue* queue,
                           void* stream);

/* ---- split-precision ("bf16x6") forms of the forward / data-gradient GEMMs.  Same arithmetic contract (fp32 in,
 * fp32 out, fp32 accumulate) with every product formed as six bf16 x bf16 MFMA terms of a 3-way hi/mid/lo split:
 * measured error vs fp64 1.1e-7 (a plain fp32 fma chain: 2.9e-7) at 6/16 of the fp32 MFMA cycles.
 * The weight operand is split once per call by ttts_weight_split into three bf16 planes (hi, mid, lo) of a rows x cols
 * matrix, stored k-tile-major as [cols/16][plane][rows][16] (cols must be a multiple of 16):
 *   mode 0  linear forward     planes of w (N,K)               rows = N,    cols = K
 *   mode 1  linear data-grad   planes of w^T                   rows = K,    cols = N
 *   mode 2  conv forward       [co][tap*cin + ci]              rows = cout, cols = taps*cin,  channels_per_tap = cin
 *   mode 3  conv data-grad     [ci][tap*cout + co]             rows = cin,  cols = taps*cout, channels_per_tap = cout
 *
 * fp16x3 ("h3") form: modes 4-7 of ttts_weight_split are the same four matrices as modes 0-3 written as TWO f16 planes
 * (hi, lo) of w * s, stored [cols/32][plane][rows][32] (cols, and channels_per_tap for the conv modes, must be multiples
 * of 32), followed by a 16-byte tail whose first float is max|w|: s is the power of two that puts max|w| in [2^11, 2^12),
 * measured by the split itself and re-derived from the tail by every kernel that takes the planes.
 * ttts_linear_fwd_h3 / ttts_conv1d_fwd_h3 take such planes and form each product from three f16 x f16 MFMA terms
 * (a_hi*b_hi + a_hi*b_lo + a_lo*b_hi): the same fp32-grade result (error vs fp64 a few 1e-7) for half the matrix-pipe
 * work.  f16 has no bf16-like exponent range, so the ACTIVATION operand is pre-scaled while it is staged, by the power
 * of two that puts ITS measured maximum in [2^11, 2^12): `x_amax` = TTTS_AMAX_SLOTS partial maxima of |x| (their maximum must be
 * >= max|x|; ttts_amax_partials computes them with one read of x, and every kernel of this header that PRODUCES an
 * activation or a gradient can leave them behind itself: the `*_amax_out` arguments).  Every element within 2^-15 of the
 * largest keeps 22 significant bits, smaller ones an absolute error of 2^-37 * max|x| -- no assumption about the operands'
 * magnitudes is left.
 * Every such array has TTTS_AMAX_SLOTS floats.  Arrays named `*_amax_out` are filled with slot-wise atomic maxima and must
 * be zeroed by the caller first (ttts_zero); only ttts_amax_partials writes its array in full. */
size_t ttts_split_bytes(int64_t rows, int64_t cols);
/* bytes of the image ttts_weight_split writes in `mode`.  Modes 4-7 (fp16x3) pad the channels of a tap -- all columns of a
 * linear weight -- with zeros to the next multiple of 32, so that the 32-deep k-tiles of the GEMM never straddle a tap; a
 * channel count that is no multiple of 32 (the 80-channel mel side) therefore needs no other kernel: the loader reads the
 * activation row's neighbour against zero weight columns.  Channel counts must be multiples of 4. */
size_t ttts_split_image_bytes(int64_t rows, int64_t cols, int mode, int channels_per_tap, int taps);
/* tile shape the forward / data-gradient dispatch uses for an M x N output with reduction length K (1: 64x64, 2: 128x128,
 * 3: 64x128, 4: 128x96; fp16x3 only: 6: 256x256 / 8 waves, 7: 256x128 / 8 waves, 8: 256x128 / 4 waves, two workgroups per
 * CU); x6 = 0: fp32-MFMA kernel, 1: bf16x6 kernel, 2: fp16x3 kernel.  A profiling aid (bench.py attributes launches). */
int ttts_gemm_tile_choice(int64_t M, int N, int K, int x6);
int ttts_weight_split(const float* w, void* planes, int rows, int cols, int mode, int channels_per_tap, int taps,
                      void* stream);
/* all weights in one launch: descs (device memory) = n x 8 int64 {w, planes, rows, cols, mode, channels_per_tap, taps,
 * first_block}, first_block = running sum of ttts_weight_split_units(rows, cols, mode, channels_per_tap) over the entries
 * before this one, total_blocks = the final sum.  (A unit is one workgroup: 256 elements of a bf16x6 image; a 32-row x
 * 32-channel tile, all taps of it, of an fp16x3 image -- read in the order the source is contiguous in and written as whole
 * 2 KB runs of the planes.)  A LINEAR fp16x3 entry (modes 4, 5, 8, 9) may be a WINDOW of a STACKED image that several
 * weights share (the fused K/V projection of all decoder layers): channels_per_tap = (image rows << 32) | image columns and
 * taps = (first image row << 32) | first image column of the window (a multiple of 32); `planes` then is the shared image,
 * whose one tail -- one scale -- receives the maximum over every window's weight.  0 / 0: the entry is its own image. */
int64_t ttts_weight_split_units(int64_t rows, int64_t cols, int mode, int channels_per_tap);
int ttts_weight_split_batched(const int64_t* descs, int n, int64_t total_blocks, void* stream);
int ttts_linear_fwd_x6(const float* x, const void* w_planes, const float* bias, const float* residual, float* y,
                       int64_t M, int N, int K, int act, float drop_p, uint64_t seed, const uint64_t* step_seed, int row_shift, int T,
                    void* stream);
/* y_amax_out: NULL, or a caller-zeroed TTTS_AMAX_SLOTS-float array receiving max|y| (y feeds another fp16x3 GEMM / attention) */
int ttts_linear_fwd_h3(const float* x, const void* w_planes, const float* bias, const float* residual, float* y,
                       int64_t M, int N, int K, int act, float drop_p, uint64_t seed, const uint64_t* step_seed, int row_shift,
                       int T, const float* x_amax, float* y_amax_out, void* stream);
/* bn_partials: NULL, or the workspace of ttts_bn_train_stats (ttts_bn_workspace_bytes): the epilogue then leaves BatchNorm's
 * row-chunk partials (count, mean, M2 per output channel and chunk, [nblk][3][cout]) behind and
 * ttts_bn_train_stats_from_partials finishes the statistics without a pass over y.  nblk = ttts_conv1d_fwd_h3_bn_blocks(...);
 * 0 means this shape's tile cannot emit them (pass NULL and use ttts_bn_train_stats). */
int ttts_conv1d_fwd_h3_bn_blocks(int B, int T, int cin, int cout, int taps);
/* rows of (b, t) one partial covers (partial i: rows i * chunk ..; 0: this shape emits none): the statistics of a row range that is
 * a whole number of chunks can be finished from its own partials, bn_partials + first_chunk * 3 * cout (ABI v12) */
int ttts_conv1d_fwd_h3_bn_chunk_rows(int B, int T, int cin, int cout, int taps);
int ttts_conv1d_fwd_h3(const float* x, const void* planes_fwd, const float* bias, float* y, int B, int T, int cin, int cout,
                       int taps, const float* x_amax, float* bn_partials, void* stream);
/* fp16x3 data gradients: as the forward, with the gradient as the activation operand (dy_amax: its partial maxima;
 * 1e-7 .. 1e-5 behind a mean-reduced loss, any magnitude in general).  planes: modes 5 / 7. */
int ttts_amax_partials(const float* x, int64_t n, float* partials /* TTTS_AMAX_SLOTS floats, fully written */, void* stream);
int ttts_linear_bwd_data_h3(const float* dy, const void* wt_planes, const float* residual, float* dx, int64_t M, int N,
                            int K, const float* relu_out, float relu_scale, const float* dy_amax, float* dx_amax_out,
                            void* stream);
/* ---- fp16x3 with an IMAGE activation operand (ABI v10; transformertts_amd/csrc/gemm_h3i.hip).  The kernels above split
 * the fp32 activation while they stage it (registers, 3.5 VALU instructions per MFMA, one k-tile of requests in flight per
 * CU).  Here the producer of the activation writes it already split: an IMAGE is row-major, a row of K values is K/16
 * groups of 64 bytes = {16 f16 "hi", 16 f16 "lo"} of x * 2^e_row (4 bytes per element, as fp32) with a PER-ROW power of two
 * that puts the row's maximum in [2^11, 2^12); row_inv[row] = 2^-e_row.  A row scale of the left operand factors out of the
 * output row, so the GEMM undoes it in its epilogue.  Both operands are then staged by LDS-DMA (no staging registers), on a
 * 128 x 256 tile with two workgroups per CU.  ttts_act_image makes an image from fp32 (K % 16 == 0, K <= 1024);
 * ttts_layernorm_fwd / _bwd emit one next to their fp32 output (their *_image_out arguments).  Replaces the same call
 * sites as ttts_linear_fwd_h3 / ttts_linear_bwd_data_h3 (torch F.linear inside nn.MultiheadAttention / _ff_block,
 * torch/nn/modules/transformer.py:951-982,1158-1199, reached from model/model.py:189-213 and model/layers.py:29-74);
 * no row shift, K % 32 == 0, N % 4 == 0. */
int ttts_act_image(const float* x, void* image, float* row_inv, int64_t M, int K, void* stream);
int ttts_linear_fwd_h3i(const void* x_image, const float* x_row_inv, const void* w_planes, const float* bias,
                        const float* residual, float* y, int64_t M, int N, int K, int act, float drop_p, uint64_t seed,
                        const uint64_t* step_seed, float* y_amax_out, void* stream);
int ttts_linear_bwd_data_h3i(const void* dy_image, const float* dy_row_inv, const void* wt_planes, const float* residual,
                             float* dx, int64_t M, int N, int K, const float* relu_out, float relu_scale,
                             float* dx_amax_out, void* stream);
/* the same kernel on a plain fp32 activation (per-tensor scale from x_amax, as ttts_linear_fwd_h3): the raw k-tile is staged by
 * LDS-DMA and split in place in LDS, so no producer has to write an image; weight planes = modes 8 / 9.  Arguments as
 * ttts_linear_fwd_h3 / ttts_linear_bwd_data_h3 (no row shift; K resp. N a multiple of 32). */
int ttts_linear_fwd_h3d(const float* x, const void* w_planes, const float* bias, const float* residual, float* y,
                        int64_t M, int N, int K, int act, float drop_p, uint64_t seed, const uint64_t* step_seed,
                        const float* x_amax, float* y_amax_out, void* stream);
int ttts_linear_bwd_data_h3d(const float* dy, const void* wt_planes, const float* residual, float* dx, int64_t M, int N,
                             int K, const float* relu_out, float relu_scale, const float* dy_amax, float* dx_amax_out,
                             void* stream);
/* ---- HEAD-IMAGE outputs (ABI v11; gemm_h3i.hip, attention_img.hip).  The output of an attention in-projection (the packed
 * q/k/v of torch `_sa_block` / F.multi_head_attention_forward, torch/nn/functional.py:6206+, or the q and k/v row slices of
 * model/layers.py:54-74) is read by nothing but the attention kernels, which form every product from f16 hi / lo pieces.  So the
 * in-projection writes it in that form INSTEAD of fp32: y_image has the geometry of the fp32 output (M rows of N 4-byte cells),
 * and the 256 bytes of (row, 64-column head) hold {64 f16 hi, 64 f16 lo} of (x W^T + b) * 2^e(row, head) with the power of
 * two that puts the head row's maximum in [2^11, 2^12); y_row_inv[head * M + row] = 2^-e.  The attention kernels stage K / V
 * tiles of it by LDS-DMA (no split arithmetic, two tiles deep).  y_amax_out: NULL, or N / amax_section_cols caller-zeroed
 * TTTS_AMAX_SLOTS-float arrays (one per section of amax_section_cols columns: q / k / v) receiving max|y| of the section
 * (amax_section_cols = 0: one array).  K % 32 == 0, N % 64 == 0, bias-only epilogue; weight planes = mode 8. */
int ttts_linear_fwd_h3d_img(const float* x, const void* w_planes, const float* bias, void* y_image, float* y_row_inv,
                            int64_t M, int N, int K, const float* x_amax, float* y_amax_out, int amax_section_cols,
                            void* stream);
/* the stand-alone conversion: fp32 rows (row stride ld_x floats) -> head image (row stride ld_image cells) + inverse scales
 * [N / 64][M] (tests; operands no GEMM of this library produced) */
int ttts_head_image(const float* x, int64_t ld_x, void* image, int64_t ld_image, float* row_inv, int64_t M, int N, void* stream);
int ttts_conv1d_bwd_data_h3(const float* dy, const void* planes_bwd, float* dx, int B, int T, int cin, int cout, int taps,
                            const float* dy_amax, void* stream);
int ttts_linear_bwd_data_x6(const float* dy, const void* wt_planes, const float* residual, float* dx, int64_t M, int N,
                            int K, const float* relu_out, float relu_scale, void* stream);
int ttts_conv1d_fwd_x6(const float* x, const void* planes_fwd, const float* bias, float* y, int B, int T, int cin, int cout,
                       int taps, void* stream);
int ttts_conv1d_bwd_data_x6(const float* dy, const void* planes_bwd, float* dx, int B, int T, int cin, int cout, int taps,
                            void* stream);
/* Weight gradients in the same split-precision form (both operands are activations, split while they are staged);
 * arguments, workspace (ttts_wgrad_workspace_bytes) and results as ttts_linear_bwd_weight / ttts_conv1d_bwd_weight. */
int ttts_linear_bwd_weight_x6(const float* dy, const float* x, float* dw, float* dbias, float* ws, size_t ws_bytes,
                              int64_t M, int N, int K, int row_shift, int T, int accumulate, ttts_reduce_queue* queue,
                              void* stream);
int ttts_conv1d_bwd_weight_x6(const float* dy, const float* x, float* dw, float* dbias, float* ws, size_t ws_bytes, int B,
                              int T, int cin, int cout, int taps, int accumulate, ttts_reduce_queue* queue, void* stream);
/* fp16x3 weight gradients: both operands are activations, pre-scaled from their partial maxima (dy_amax is shared with the
 * data gradient of the same dy, x_amax with the forward GEMM that read x); shapes the split kernels do not cover fall
 * back to the fp32-MFMA kernel exactly as the _x6 entry points do. */
int ttts_linear_bwd_weight_h3(const float* dy, const float* x, float* dw, float* dbias, float* ws, size_t ws_bytes,
                              int64_t M, int N, int K, int row_shift, int T, int accumulate, const float* dy_amax,
                              const float* x_amax, ttts_reduce_queue* queue, void* stream);
int ttts_conv1d_bwd_weight_h3(const float* dy, const float* x, float* dw, float* dbias, float* ws, size_t ws_bytes, int B,
                              int T, int cin, int cout, int taps, int accumulate, const float* dy_amax, const float* x_amax,
                              ttts_reduce_queue* queue, void* stream);
/* ONE weight-gradient GEMM dy^T x (N x K) whose N rows belong to `nparts` weights (equal row blocks): block i is reduced into
 * dw_parts[i] ((N / nparts) x K floats) and its column sums into dbias_parts[i] (NULL array: no bias gradients); dw_parts /
 * dbias_parts are HOST arrays of device pointers.  The backward of the cross-attention K/V projection of every decoder layer
 * run as one GEMM on the encoder memory they all read (the reference runs it per layer: model/layers.py:54-74, rows d..3d of
 * each layer's multihead_attn.in_proj_weight). */
/* ---- ABI v12 (round 6): grouped weight gradients, the multi-destination weight gradient, stacked weight images
 * (ttts_weight_split_batched).
 * GROUPED weight gradients: n <= 4 independent problems as ONE launch of an fp16x3 weight-gradient kernel -- the weights of a layer,
 * whose operands are all at hand when backward leaves the layer and whose results nobody reads before the optimizer.  Member i
 * with taps_i = 1: dw_i[N_i,K_i] (+)= dy_i[M_i,N_i]^T x_i[M_i,K_i] (ttts_linear_bwd_weight_h3; row_shift_i / T_i as its row_shift /
 * T); taps_i > 1: the weight gradient
 * of a same-padded convolution over utterances of T_i rows, dw_i[N_i = cout, K_i = cin, taps_i], M_i = B T_i
 * (ttts_conv1d_bwd_weight_h3).  dbias_i: column sums of dy_i, or NULL.  Every array argument is a HOST array of n entries; ws_i /
 * ws_bytes_i as ttts_wgrad_workspace_bytes(M_i, N_i, K_i, taps_i), which covers the member in any group (alone too, where an output
 * of one tile is planned more row splits than in a launch of its own).  The row splits are planned for the group, so each member of
 * n writes 1/n of the partial sums of a launch of its own.  ttts_wgrad_group_ok: the CLASS of a problem -- 0: no member of any group; 1: the
 * 4-wave 128 x 128 tile; 2: whole 256 x 256 tiles on the 8-wave LDS-DMA kernel (the FFN, packed in-projection and post-net
 * convolution weights over long row ranges); 3 / 4: the 128 x 96 / 96 x 128 tiles of weights with 80 input / output channels
 * (the mel side) -- the members of one launch share a class.  A convolution member's tap count must be odd, as in the single
 * entries: the launch refuses an even one ("taps=<n>"), although the class query answers for it.  (The autograd of torch.nn.Linear /
 * nn.Conv1d runs these one by one: model/module.py:4-53 and the torch layers of model/model.py:189-213.) */
int ttts_wgrad_group_ok(int64_t M, int N, int K, int taps);
int ttts_wgrad_group(int n, const float* const* dy, const float* const* x, float* const* dw, float* const* dbias,
                     float* const* ws, const size_t* ws_bytes, const int64_t* M, const int* N, const int* K, const int* taps,
                     const int* T, const int* row_shift, int accumulate, const float* const* dy_amax, const float* const* x_amax,
                     ttts_reduce_queue* queue, void* stream);
int ttts_linear_bwd_weight_h3_parts(const float* dy, const float* x, float* const* dw_parts, float* const* dbias_parts, int nparts,
                                    float* ws, size_t ws_bytes, int64_t M, int N, int K, int accumulate, const float* dy_amax,
                                    const float* x_amax, ttts_reduce_queue* queue, void* stream);

/* ------------------------------------------------------------------ Conv1d (k taps, same padding) on (B,T,C)
 * Replaces ConvNormBN's permute -> nn.Conv1d(pad=(k-1)//2) -> permute (model/module.py:28-33) as an
 * implicit GEMM directly on the (B,T,C) layout.  Weights are re-laid once per call by
 * ttts_conv1d_pack_weight: w[co][ci][tap] -> w_fwd[co][tap][ci] and/or w_bwd[ci][tap][co]. */
size_t ttts_conv1d_pack_bytes(int cout, int cin, int taps);
int ttts_conv1d_pack_weight(const float* w, float* w_fwd, float* w_bwd, int cout, int cin, int taps, void* stream);
int ttts_conv1d_fwd(const float* x, const float* w_fwd, const float* bias, float* y, int B, int T, int cin, int cout,
                    int taps, void* stream);
int ttts_conv1d_bwd_data(const float* dy, const float* w_bwd, float* dx, int B, int T, int cin, int cout, int taps,
                         void* stream);
int ttts_conv1d_bwd_weight(const float* dy, const float* x, float* dw, float* dbias, float* ws, size_t ws_bytes, int B,
                           int T, int cin, int cout, int taps, int accumulate, ttts_reduce_queue* queue, void* stream);

/* ------------------------------------------------------------------ BatchNorm1d over (M = B*T rows, C channels)
 * Replaces nn.BatchNorm1d inside ConvNormBN (model/module.py:19,31) plus the Tanh / Dropout entries that
 * follow it in EncoderPreNet / PostNet (model/model.py:29-33,113-126).
 * train: batch statistics over all rows (padding included), running stats updated with momentum and the
 * unbiased variance, num_batches_tracked += 1.  eval: normalise with the running statistics. */
size_t ttts_bn_workspace_bytes(int64_t M, int C);
int ttts_bn_train_stats(const float* x, float* mean, float* invstd, float* running_mean, float* running_var,
                        int64_t* num_batches_tracked, float* ws, size_t ws_bytes, int64_t M, int C, float momentum,
                        float eps, void* stream);
int ttts_bn_train_stats_from_partials(const float* partials, int nblk, float* mean, float* invstd, float* running_mean,
                                      float* running_var, int64_t* num_batches_tracked, int C, float momentum, float eps,
                                      void* stream);
/* as above, merged with n_rows (0 .. 256) rows of the matrix itself (row stride C; `rows` their first) that none of the nblk (>= 0)
 * partials covers: a row range that does not end on a chunk boundary takes its whole chunks from the epilogue's partials and the rest
 * from y (the halves of a twin batch).  (ABI v13) */
int ttts_bn_train_stats_from_partials_rows(const float* partials, int nblk, const float* rows, int n_rows, float* mean,
                                           float* invstd, float* running_mean, float* running_var,
                                           int64_t* num_batches_tracked, int C, float momentum, float eps, void* stream);
/* ttts_bn_train_stats_from_partials_rows for TWO row sets of one matrix in one launch (the halves of a twin batch); the running
 * statistics and the batch counter receive set a's update first, then set b's -- two calls in that order, one launch (ABI v14) */
int ttts_bn_train_stats_twin(const float* partials_a, int nblk_a, const float* rows_a, int n_rows_a, float* mean_a, float* invstd_a,
                             const float* partials_b, int nblk_b, const float* rows_b, int n_rows_b, float* mean_b, float* invstd_b,
                             float* running_mean, float* running_var, int64_t* num_batches_tracked, int C, float momentum,
                             float eps, void* stream);
int ttts_bn_eval_stats(const float* running_mean, const float* running_var, float* mean, float* invstd, int C, float eps,
                       void* stream);
/* z = drop(act((x - mean) * invstd * gamma + beta)); z_amax_out: NULL, or a caller-zeroed TTTS_AMAX_SLOTS-float array receiving max|z| */
int ttts_bn_apply_fwd(const float* x, const float* mean, const float* invstd, const float* gamma, const float* beta,
                      float* z, int64_t M, int C, int act, float drop_p, uint64_t seed, const uint64_t* step_seed,
                      float* z_amax_out, void* stream);
/* backward through drop/act/BN: dx, dgamma, dbeta from dz and the saved x, mean, invstd.  batch_stats = 1: train mode (mean /
 * invstd are the batch statistics of x, whose derivative dx carries); 0: eval mode (running statistics, constants). */
int ttts_bn_bwd(const float* dz, const float* x, const float* mean, const float* invstd, const float* gamma,
                const float* beta, float* dx, float* dgamma, float* dbeta, float* ws, size_t ws_bytes, int64_t M, int C,
                int act, float drop_p, uint64_t seed, const uint64_t* step_seed, int accumulate, float* dx_amax_out,
                int batch_stats, void* stream);

/* ------------------------------------------------------------------ LayerNorm over the last dim (1 <= d <= 1024)
 * Replaces nn.LayerNorm norm1/2/3 of the encoder/decoder layers (torch/nn/modules/transformer.py:951-956,
 * model/layers.py:47-50).  The residual sum is produced by the preceding GEMM's epilogue. */
/* y_image_out / y_row_inv_out (ABI v10): NULL, or the activation image of y and its per-row inverse scales for the GEMMs that read
 * y (ttts_linear_fwd_h3i; M * d * 4 bytes and M floats; d in {256, 512, 1024}): the row is complete in the kernel's registers,
 * so the split costs one extra write and no pass. */
int ttts_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                       int64_t M, int d, float eps, float* y_amax_out /* NULL, or zeroed TTTS_AMAX_SLOTS floats: max|y| */,
                       void* y_image_out, float* y_row_inv_out, void* stream);
size_t ttts_layernorm_bwd_workspace_bytes(int d);
int ttts_layernorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                       float* dx, float* dgamma, float* dbeta, float* ws, size_t ws_bytes, int64_t M, int d,
                       int accumulate, void* dx_image_out /* NULL, or the image of dx (ttts_linear_bwd_data_h3i) */,
                       float* dx_row_inv_out, ttts_reduce_queue* queue, void* stream);
/* the same, and in the same pass dacc = dx * keep(seed, element) / (1 - drop_p): the gradient behind the residual dropout
 * of the sublayer whose output this LayerNorm normalised (ttts_dropout_bwd(dx) without a pass of its own; same mask as
 * the forward epilogue of that sublayer's last Linear).  dacc_amax: NULL, or a caller-zeroed TTTS_AMAX_SLOTS-float array that receives
 * partial maxima of |dacc|.  d in {256, 512, 1024}, operands 16-byte aligned. */
int ttts_layernorm_bwd_drop(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                            float* dx, float* dgamma, float* dbeta, float* ws, size_t ws_bytes, int64_t M, int d,
                            int accumulate, float* dacc, float drop_p, uint64_t seed, const uint64_t* step_seed,
                            float* dacc_amax, void* dacc_image_out /* NULL, or the image of dacc */, float* dacc_row_inv_out,
                            ttts_reduce_queue* queue, void* stream);

/* ------------------------------------------------------------------ attention (64 columns per head)
 * Scaled dot-product attention with masks computed from lengths in-kernel (no mask tensors):
 * key j of batch b is dead when j >= key_lens[b], or (causal) j > i.  q is multiplied by q_scale before q.k^T exactly as
 * torch does (q * sqrt(1 / head_dim), torch/nn/functional.py:6578): 0.125 for head_dim 64.  q/k/v/o are addressed as
 * ptr[(b*T + t)*ld + h*64 + c], so packed in-proj outputs of 64-wide heads are consumed in place; narrower heads
 * (head_dim < 64) are zero-padded to 64 columns by ttts_heads_pad (zeros add nothing to q.k^T and produce zero output
 * columns) and passed with q_scale = sqrt(1 / head_dim).
 * Replaces: encoder self-attention and decoder `_sa_block` (torch/nn/modules/transformer.py:961-978,
 * 1158-1175 -> F.scaled_dot_product_attention, torch/nn/functional.py:6629) and the decoder's
 * `_mha_block` cross-attention with need_weights=True, average_attn_weights=False
 * (model/layers.py:54-74; torch/nn/functional.py:6576-6610).
 * attn (optional) receives the per-head, post-dropout weights (B,H,Tq,Tk); lse (B,H,Tq) is saved for backward. */
/* head_dim < 64: dst (rows, H*64) = the H heads of src (rows x ld_src, head h at column h*head_dim) zero-padded to 64
 * columns each; ttts_heads_unpad writes the first head_dim columns of every 64-wide head of src (rows, H*64) back to
 * dst (rows x ld_dst, head h at column h*head_dim), leaving the other columns of dst untouched. */
int ttts_heads_pad(const float* src, int64_t ld_src, float* dst, int64_t rows, int H, int head_dim, void* stream);
int ttts_heads_unpad(const float* src, float* dst, int64_t ld_dst, int64_t rows, int H, int head_dim, void* stream);
int ttts_attention_fwd(const float* q, const float* k, const float* v, float* o, float* lse, float* attn,
                       const int64_t* key_lens, int B, int H, int Tq, int Tk, int ldq, int ldk, int ldv, int ldo,
                       int causal, float q_scale, float drop_p, uint64_t seed, const uint64_t* step_seed, void* stream);
/* dq, dk, dv from do_ (recomputes the probabilities from q, k and lse); delta (B,H,Tq) is scratch */
int ttts_attention_bwd(const float* q, const float* k, const float* v, const float* o, const float* do_,
                       const float* lse, float* delta, float* dq, float* dk, float* dv, const int64_t* key_lens, int B,
                       int H, int Tq, int Tk, int ldq, int ldk, int ldv, int ldo, int lddq, int lddk, int lddv,
                       int causal, float q_scale, float drop_p, uint64_t seed, const uint64_t* step_seed, void* stream);
/* Split-precision forms of the two entry points above (bf16x6 MFMA products, fp32-grade results; same arguments). */
int ttts_attention_fwd_x6(const float* q, const float* k, const float* v, float* o, float* lse, float* attn,
                          const int64_t* key_lens, int B, int H, int Tq, int Tk, int ldq, int ldk, int ldv, int ldo,
                          int causal, float q_scale, float drop_p, uint64_t seed, const uint64_t* step_seed, void* stream);
/* fp16x3 form of the forward (three f16 MFMA terms; Q/8, K and V pre-scaled from their partial maxima q_amax / k_amax /
 * v_amax -- TTTS_AMAX_SLOTS floats each, the same array three times for a packed projection output -- and probabilities x 2^10);
 * lse in natural units, so either backward form can follow it.  o_amax_out: NULL, or zeroed TTTS_AMAX_SLOTS floats: max|o|.
 * rowstat_out: NULL, or (3, B, H, Tq) floats (ABI v10: a third plane): per query row the subtrahend of the weights' exponents
 * exactly as the kernel used it with the final row maximum (one rounded product, in the kernel's own pre-scaled units), log2
 * of the row sum of those weights -- what ttts_attention_bwd_h3 needs to form the very probabilities the forward formed (it
 * re-creates bit-identical score accumulators and the same exponents, whatever the scores' magnitude; from lse alone the
 * probabilities are only good to ulp(lse), i.e. 6 % at scores of 1e6, where torch -- which keeps the probabilities -- is
 * still accurate) -- and 1.0 / 0.0: the row is ONE-HOT in fp32 (its sum is its largest term).  torch's softmax backward of
 * such a row is exactly zero; a backward that recomputes the probabilities would return the rounding of delta against dP
 * instead, so ttts_attention_bwd_h3 takes the row's score gradient as zero. */
int ttts_attention_fwd_h3(const float* q, const float* k, const float* v, float* o, float* lse, float* attn,
                          const int64_t* key_lens, int B, int H, int Tq, int Tk, int ldq, int ldk, int ldv, int ldo,
                          int causal, float q_scale, float drop_p, uint64_t seed, const uint64_t* step_seed, const float* q_amax,
                          const float* k_amax, const float* v_amax, float* o_amax_out, float* rowstat_out, void* stream);
int ttts_attention_bwd_x6(const float* q, const float* k, const float* v, const float* o, const float* d_o,
                          const float* lse, float* delta, float* dq, float* dk, float* dv, const int64_t* key_lens, int B,
                          int H, int Tq, int Tk, int ldq, int ldk, int ldv, int ldo, int lddq, int lddk, int lddv,
                          int causal, float q_scale, float drop_p, uint64_t seed, const uint64_t* step_seed, void* stream);
/* fp16x3 form of the backward.  d_o is pre-scaled by the power of two that puts max|d_o| in [2^11, 2^12) (do_amax = the
 * TTTS_AMAX_SLOTS partial maxima of ttts_amax_partials(d_o)); dS = P (dP - delta) lives in registers as a lane-local accumulator
 * column and gets a lane-local pre-scale that is lowered on the fly together with its accumulator. */
int ttts_attention_bwd_h3(const float* q, const float* k, const float* v, const float* o, const float* d_o,
                          const float* lse, float* delta, float* dq, float* dk, float* dv, const int64_t* key_lens, int B,
                          int H, int Tq, int Tk, int ldq, int ldk, int ldv, int ldo, int lddq, int lddk, int lddv,
                          int causal, float q_scale, float drop_p, uint64_t seed, const uint64_t* step_seed, const float* do_amax,
                          float* dq_amax_out, float* dkv_amax_out, const float* q_amax, const float* k_amax,
                          const float* v_amax, const float* rowstat /* of the h3 forward, or NULL: use lse */, void* stream);
/* ---- attention for heads of 65 .. 128 columns (ABI v17; attention_wide.hip): the same call sites as ttts_attention_fwd_h3 /
 * ttts_attention_bwd_h3 -- encoder self-attention and decoder `_sa_block` (torch/nn/modules/transformer.py:961-978,1158-1175 ->
 * F.scaled_dot_product_attention, torch/nn/functional.py:6629) and the decoder's `_mha_block` cross-attention with
 * need_weights=True, average_attn_weights=False (model/layers.py:54-74; torch/nn/functional.py:6576-6610) -- in a model whose
 * `nhead` leaves heads wider than 64 columns (the constructor takes any nhead that divides d_model, model/model.py:139-161).
 * Same masks, dropout hash and edge conventions as ttts_attention_fwd; products on fp32 MFMA (exact fp32 products, no operand
 * pre-scales).  q/k/v/o are addressed as ptr[(b*T + t)*ld + h*128 + c], so a packed in-projection output of 128-wide heads is
 * read in place; heads of 65 .. 127 columns are zero-padded to 128 by ttts_heads_pad_w and passed with q_scale =
 * sqrt(1 / head_dim).  rowstat: (2, B, H, Tq) floats, written by the forward and read by the backward: the final row maximum m
 * of the masked, scaled scores (0 for a row without a live key) and the row sum l of exp(s - m).  The backward forms
 * p = exp(s - m) / l as the forward did; a row whose l is exactly 1.0f is one-hot in fp32 and its score gradient is taken as
 * zero (what torch's softmax backward gives; see ttts_attention_fwd_h3).  attn: NULL, or the (B,H,Tq,Tk) post-dropout weights
 * (non-causal form only).  delta (B,H,Tq) is scratch.  A bad argument is refused before any launch with a message that names it
 * (row strides that are no multiple of 4 floats or below H*128, drop_p outside [0, 1), non-positive sizes). */
int ttts_attention_fwd_wide(const float* q, const float* k, const float* v, float* o, float* rowstat, float* attn,
                            const int64_t* key_lens, int B, int H, int Tq, int Tk, int ldq, int ldk, int ldv, int ldo,
                            int causal, float q_scale, float drop_p, uint64_t seed, const uint64_t* step_seed, void* stream);
int ttts_attention_bwd_wide(const float* q, const float* k, const float* v, const float* o, const float* d_o,
                            const float* rowstat, float* delta, float* dq, float* dk, float* dv, const int64_t* key_lens,
                            int B, int H, int Tq, int Tk, int ldq, int ldk, int ldv, int ldo, int lddq, int lddk, int lddv,
                            int causal, float q_scale, float drop_p, uint64_t seed, const uint64_t* step_seed, void* stream);
/* ---- the 128-column attention under masks that are tensors (ABI v18; attention_wide.hip): the call sites above when the layer
 * is given a `src_key_padding_mask` / `tgt_key_padding_mask` / `memory_key_padding_mask` with holes, a `memory_mask`, or a
 * `mask` / `tgt_mask` that is not the causal one (arguments of model/layers.py:29-74 -> `_sa_block` / `_mha_block` ->
 * F.multi_head_attention_forward, which merges them into one float attn_mask, torch/nn/functional.py:6404-6436, and adds it to
 * the scaled scores, torch/nn/functional.py:6578-6586 resp. scaled_dot_product_attention's attn_mask, :6629).  Arguments of the
 * _wide entry points plus:
 *   add_mask   NULL, or fp32: element (b, h, q, key) at add_mask[b*mask_stride_b + h*mask_stride_h + q*ldm + key] (strides in
 *              elements, 0 = broadcast: torch's (Tq, Tk) form is 0 / 0, its (B*H, Tq, Tk) form H*Tq*ldm / Tq*ldm).  A value at
 *              or below half the lowest finite float (-inf, finfo.min) forbids the key; any other value is added to the scaled
 *              score q_scale * q.k.  ldm is a multiple of 4 floats and >= Tk, every slice 16-byte aligned and below 4 GiB.
 *   key_dead   NULL, or (B, ldd) bytes, ldd >= Tk: non-zero = the key is not attended to.
 * A key is alive iff key < key_lens[b] && !dead && !forbidden && (!causal || key <= q); with key_dead the caller may pass
 * key_lens = one past the last live key.  A query row without an alive key gives zeros in o and attn, m = l = 0 in rowstat, a
 * zero dq row and no contribution to dk / dv.  Dropout, the post-dropout weights, rowstat and the one-hot rule are those of
 * the _wide entry points (same hash, same row ids).  Refused before any launch, naming the value: both masks NULL, ldm < Tk or
 * no multiple of 4, a misaligned mask, negative strides, ldd < Tk, weights together with causal. */
int ttts_attention_fwd_wide_masked(const float* q, const float* k, const float* v, float* o, float* rowstat, float* attn,
                                   const int64_t* key_lens, int B, int H, int Tq, int Tk, int ldq, int ldk, int ldv, int ldo,
                                   int causal, float q_scale, float drop_p, uint64_t seed, const uint64_t* step_seed,
                                   const float* add_mask, int64_t ldm, int64_t mask_stride_b, int64_t mask_stride_h,
                                   const uint8_t* key_dead, int64_t ldd, void* stream);
int ttts_attention_bwd_wide_masked(const float* q, const float* k, const float* v, const float* o, const float* d_o,
                                   const float* rowstat, float* delta, float* dq, float* dk, float* dv, const int64_t* key_lens,
                                   int B, int H, int Tq, int Tk, int ldq, int ldk, int ldv, int ldo, int lddq, int lddk, int lddv,
                                   int causal, float q_scale, float drop_p, uint64_t seed, const uint64_t* step_seed,
                                   const float* add_mask, int64_t ldm, int64_t mask_stride_b, int64_t mask_stride_h,
                                   const uint8_t* key_dead, int64_t ldd, void* stream);
/* ---- the 128-column attention backward when the returned weights carry a gradient of their own (ABI v19; attention_wide.hip
 * DATTN forms): the decoder's `_mha_block` hands out the per-head post-dropout weights of nn.MultiheadAttention(need_weights=True,
 * average_attn_weights=False) (model/layers.py:68-74) as ordinary autograd tensors, so a loss written on output['alignments']
 * reaches q, k and v through softmax and dropout (torch/nn/functional.py:6578-6610: baddbmm -> softmax -> dropout -> bmm).
 * Arguments of ttts_attention_bwd_wide_masked -- add_mask and key_dead may BOTH be NULL here -- plus:
 *   attn     the (B,H,Tq,Tk) weights A the forward wrote for these operands, masks, drop_p, seed and step word, contiguous
 *   d_attn   fp32: element (b, h, q, key) at d_attn[b*dattn_stride_b + h*dattn_stride_h + q*ld_dattn + key] (strides in
 *            elements, 0 = broadcast); ld_dattn a multiple of 4 floats and >= Tk, every slice 16-byte aligned and below 4 GiB.
 *            Elements of keys that are not alive are never used.
 * With P the softmax over the alive keys, D the keep mask and A = D o P / (1 - p): dS = P o (D / (1 - p) (d_o . v + d_attn) -
 * delta), delta = d_o . o + sum_n A d_attn (the sum in a fixed order per row); dV is that of the _wide entry points; the
 * one-hot rule stands.  Non-causal only.  Refused before any launch, naming the value: NULL attn or d_attn, causal != 0,
 * ld_dattn < Tk or no multiple of 4, a misaligned slice, negative strides, a slice over 4 GiB, and what the _masked entry point
 * refuses of a mask that is given. */
int ttts_attention_bwd_wide_dattn(const float* q, const float* k, const float* v, const float* o, const float* d_o,
                                  const float* rowstat, float* delta, float* dq, float* dk, float* dv, const int64_t* key_lens,
                                  int B, int H, int Tq, int Tk, int ldq, int ldk, int ldv, int ldo, int lddq, int lddk, int lddv,
                                  int causal, float q_scale, float drop_p, uint64_t seed, const uint64_t* step_seed,
                                  const float* add_mask, int64_t ldm, int64_t mask_stride_b, int64_t mask_stride_h,
                                  const uint8_t* key_dead, int64_t ldd, const float* attn, const float* d_attn, int64_t ld_dattn,
                                  int64_t dattn_stride_b, int64_t dattn_stride_h, void* stream);
/* ---- guided attention loss on the alignment maps (ABI v19; guided.hip): the term Transformer-TTS recipes add on
 * output['alignments'] (the per-head weights of model/layers.py:68-74, a list with one (B,H,Tm,Tp) map per decoder layer,
 * model/model.py) -- in torch, per selected map, `(attn * W[:, None]).sum()` over a host-built (B,Tm,Tp) prior
 *   W_b[t][n] = 1 - exp(-(n / N_b - t / T_b)^2 / (2 sigma^2)) for t < T_b = melspec_lens[b], n < N_b = phoneme_lens[b], else 0,
 * summed over the maps and divided by n_selected * sum_b T_b N_b (n_selected = selected maps x selected heads).  Forward: one call
 * per selected map writes its B*H*Tm row sums to partials[map_index] (partials: (n_maps, B*H*Tm) floats; head_mask: 0 = every
 * head, else bit h = head h counts, H <= 64); the call with loss_out != NULL (the last one) also sums all n_maps * B*H*Tm partials
 * in a fixed order and writes the scalar.  Backward: reads the upstream gradient *g_loss from device memory and writes
 * d_attn[plane][t][n] = g W_b[t][n] / (n_selected sum T N) with row stride ld (a multiple of 4 floats, >= Tp) and exact zeros in
 * padding rows and columns: (B, Tm, ld) when head_mask is 0 -- one tensor that serves every selected map and, through a head
 * stride of 0, every head (ttts_attention_bwd_wide_dattn) -- else (B, H, Tm, ld) with zero planes for unselected heads.  The
 * normaliser is formed on the device; nothing is read back, no atomics: both calls capture into a HIP graph and repeat bit for
 * bit.  Refused, naming the value: sigma <= 0, non-positive sizes or n_selected, a head_mask bit past H, a bad ld or map_index. */
int ttts_guided_attention_fwd(const float* attn, const int64_t* phoneme_lens, const int64_t* melspec_lens, uint64_t head_mask,
                              float sigma, int B, int H, int Tm, int Tp, float* partials, int map_index, int n_maps, int n_selected,
                              float* loss_out, void* stream);
int ttts_guided_attention_bwd(const float* g_loss, const int64_t* phoneme_lens, const int64_t* melspec_lens, uint64_t head_mask,
                              float sigma, int n_selected, int B, int H, int Tm, int Tp, int ld, float* d_attn, void* stream);
/* ---- phoneme durations from the alignment maps (ABI v20; alignment.hip): what a Transformer-TTS teacher hands a
 * non-autoregressive student (FastSpeech: focus rate, most diagonal head, frames per phoneme; Glow-TTS: monotonic alignment
 * search).  In torch, over output['alignments'] (the per-head weights of model/layers.py:68-74, one (B,H,Tm,Tp) map per decoder
 * layer): `attn.max(-1)`, `.argmax(-1)`, a host read to pick the head, `torch.bincount` per utterance -- three ATen passes over
 * every map -- and a Python loop for the search.  Here: one pass over each map, one small kernel each for the choice, the
 * counts and the search, every data-dependent decision on the device, nothing read back, no atomics on global memory, fixed
 * summation orders (lane order, then the xor tree): the calls capture into a HIP graph and repeat bit for bit.
 * Element (b, h, t, n) of a map is attn[b * ld_batch + h * ld_head + t * ld_row + n] (strides in floats, unit column stride, no
 * alignment asked); T_b = melspec_lens[b] clamped to [0, Tm], N_b = phoneme_lens[b] clamped to [0, Tp] (int64, device).  Nothing at
 * t >= T_b or n >= N_b is ever loaded.
 *   rowstats   for map `layer` of L: argmax[layer][b][h][t] = the FIRST n < N_b with A[t][n] = max_n A[t][n] (torch.argmax's tie
 *              rule; 0 for t >= T_b or N_b = 0), argmax being (L,B,H,Tm) int32; rowmax is (B,H,Tm) floats of scratch that the next
 *              call may reuse; focus[layer][b][h] = (1 / T_b) sum_{t < T_b} max_n A[t][n], 0 when T_b = 0 or N_b = 0, focus being
 *              (L,B,H) floats.
 *   select     choice[b] = layer * H + head (int64, (B,)); choice_pairs, if not NULL, (B,2) = (layer, head).  Modes:
 *              UTTERANCE  per b the largest focus[layer][b][head], ties to the lowest layer * H + head;
 *              BATCH      one pair for every b, the largest sum_b focus over the rows with T_b, N_b > 0 (summed in b order), same ties;
 *              FIXED      the given (layer, head).
 *   durations_argmax   durations[b][n] = #{t < T_b : argmax[choice[b]][b][t] = n}, int64 (B,Tp), exact zeros at n >= N_b; a row
 *              sums to T_b when N_b > 0.  valid (may be NULL): valid[b] = T_b > 0 and N_b > 0.
 *   mas        on plane choice[b] of utterance b, with s[t][n] = logf(fmaxf(A[t][n], 1e-30f)): Q[0][0] = s[0][0],
 *              Q[t][n] = s[t][n] + max(Q[t-1][n], Q[t-1][n-1]) over the cells with n <= t and N_b-1-n <= T_b-1-t (those from which
 *              the end is still reachable); the path runs from (0, 0) to (T_b-1, N_b-1) and on a tie STAYS on its phoneme
 *              (Q[t-1][n] >= Q[t-1][n-1]).  durations[b][n] = frames the path spends on n: >= 1 for n < N_b, summing to T_b, zeros
 *              from N_b on.  valid[b] = 0 (uint8) and an all-zero row when T_b < N_b or a length is 0 -- no monotonic path visits
 *              every phoneme.  The chosen plane lives in the map choice[b] names, so `maps` is a HOST array of L device pointers
 *              that travels to the kernel by value (no device pointer table); all L maps share the strides.  ws: the stay / advance
 *              bits, one per cell, 8-byte aligned, ttts_alignment_mas_workspace_bytes(B, Tm, Tp) bytes (0 for a non-positive size).
 * Refused before any launch, naming the value: null pointers (a NULL entry of `maps` included), non-positive sizes, ld_row < Tp,
 * negative ld_head / ld_batch, L > 16, a layer outside [0, L), B*H*Tm >= 2^31, an unknown mode, a FIXED (layer, head) outside
 * (L, H), L*H > 1024 (select), Tp > 4096 (durations_argmax), Tp > 1024 (mas), a workspace that is misaligned or too small. */
#define TTTS_ALIGN_MAX_MAPS 16
#define TTTS_ALIGN_SELECT_UTTERANCE 0
#define TTTS_ALIGN_SELECT_BATCH 1
#define TTTS_ALIGN_SELECT_FIXED 2
int ttts_alignment_rowstats(const float* attn, int64_t ld_row, int64_t ld_head, int64_t ld_batch, const int64_t* phoneme_lens,
                            const int64_t* melspec_lens, int B, int H, int Tm, int Tp, int layer, int L, int32_t* argmax,
                            float* rowmax, float* focus, void* stream);
int ttts_alignment_select(const float* focus, const int64_t* phoneme_lens, const int64_t* melspec_lens, int L, int B, int H, int mode,
                          int layer, int head, int64_t* choice, int64_t* choice_pairs, void* stream);
int ttts_alignment_durations_argmax(const int32_t* argmax, const int64_t* choice, const int64_t* phoneme_lens,
                                    const int64_t* melspec_lens, int L, int B, int H, int Tm, int Tp, int64_t* durations, uint8_t* valid,
                                    void* stream);
size_t ttts_alignment_mas_workspace_bytes(int B, int Tm, int Tp);
int ttts_alignment_mas(const float* const* maps, int L, int64_t ld_row, int64_t ld_head, int64_t ld_batch, const int64_t* choice,
                       const int64_t* phoneme_lens, const int64_t* melspec_lens, int B, int H, int Tm, int Tp, void* ws,
                       size_t ws_bytes, int64_t* durations, uint8_t* valid, void* stream);
/* ---- dynamic time warping between two ragged batches of feature sequences (ABI v22; dtw.hip): the number that compares a
 * synthesised mel with its recording, whose lengths never agree -- mel-DTW on log-mels, MCD-DTW on mel-cepstra.  In torch:
 * `torch.cdist(x, y, p=1)` (or p=2) for the cells, then a Python loop over the Tx + Ty - 1 anti-diagonals of
 * `torch.minimum(torch.minimum(D[i-1, j-1], D[i-1, j]), D[i, j-1])` with host control and a host loop for the path: thousands of
 * launches a batch, not capturable.  Here: two launches, every decision on the device, nothing read back, no atomics, fp32
 * throughout, fixed summation order: the call captures into a HIP graph and repeats bit for bit, and row b's result depends on
 * neither the other rows nor Tx / Ty beyond its own lengths.
 * Element (b, i, k) of x is x[b * ldx_batch + i * ldx_row + k] (strides in floats, unit channel stride, dword loads, no alignment
 * asked), y alike; n_b = x_lens[b] clamped to [0, Tx], m_b = y_lens[b] clamped to [0, Ty] (int64, device).  Nothing at row >= n_b
 * of x or row >= m_b of y is ever loaded.
 *   cell cost   TTTS_DTW_L1: c[i][j] = sum_k |x[i][k] - y[j][k]|
 *               TTTS_DTW_L2: c[i][j] = sqrtf(sum_k (x[i][k] - y[j][k])^2)
 *               the sum runs over k = 0 .. C-1 in that order, whatever B, the padding or the strides
 *   recurrence  D[0][0] = c[0][0],  D[i][j] = c[i][j] + min(D[i-1][j-1], D[i-1][j], D[i][j-1]),  a predecessor that does not exist
 *               counting as +inf
 *   tie rule    the FIRST minimum wins in the order diagonal (i-1, j-1), then (i-1, j), then (i, j-1)
 *   cost        (B,) fp32: D[n_b-1][m_b-1]
 *   path_len    (B,) int64: cells on the path backtracked from (n_b-1, m_b-1) to (0, 0) by the tie rule
 *   distance    (B,) fp32: cost / (path_len * C) for L1, cost / path_len for L2
 *   valid       (B,) uint8: n_b > 0 && m_b > 0; an invalid row has cost, distance and path_len 0 and an all -1 path row
 *   path        NULL, or (B, Tx + Ty - 1, 2) int32: the cells (i, j) in order from (0, 0), -1 behind path_len
 * ws: 4-byte aligned, ttts_dtw_workspace_bytes(B, Tx, Ty) bytes =
 *   B * 4 * (Tx * Ty + S * (Tx + 63) * 64 + S * Tx + 2 * (Tx + Ty)),  K = the least of 1, 2, 4, 8, 16 with 64 * K >= Ty (16 beyond),
 *   S = ceil(Ty / (64 * K))
 * -- the staged cell costs, one 32-bit word of 2-bit directions per lane and step (2 bits a cell once Ty >= 1024), the last
 * column of each strip of 64 * K columns, and the path in backtrack order; 0 for a size that is not positive or above 4096.  A
 * caller with many utterances runs them in groups to bound it (transformertts_amd.metrics.dtw_distance does).
 * Refused before any launch, naming the value: null pointers (path may be NULL), non-positive sizes, a row stride < C, negative
 * batch strides, an unknown metric, Tx or Ty > 4096, B > 65535 (the grid), a workspace that is misaligned or too small. */
#define TTTS_DTW_L1 0
#define TTTS_DTW_L2 1
size_t ttts_dtw_workspace_bytes(int B, int Tx, int Ty);
int ttts_dtw(const float* x, int64_t ldx_row, int64_t ldx_batch, const int64_t* x_lens, const float* y, int64_t ldy_row,
             int64_t ldy_batch, const int64_t* y_lens, int B, int Tx, int Ty, int C, int metric, void* ws, size_t ws_bytes, float* cost,
             int64_t* path_len, float* distance, uint8_t* valid, int32_t* path, void* stream);
/* ---- log-mel front end: a ragged batch of waveforms to model-ready mel batches (ABI v23; audio.hip, fft_lds.h): what
 * librosa.stft(center=True, pad_mode='reflect', window='hann') -> abs -> librosa.filters.mel(norm='slaney') -> log(clip) computes,
 * in one launch, with no padded copy of the signal and no spectrogram in HBM.
 *   wave        (B, Nmax) fp32, utterance b at wave + b * ld_batch; len_b = wave_lens[b] (int64, device) clamped to [0, Nmax].
 *               Samples at or beyond len_b are never read.
 *   framing     frame t covers samples g = t * hop - n_fft/2 + n, n = 0 .. n_fft - 1
 *   reflection  g < 0 reads sample -g; g >= len reads sample 2 * (len - 1) - g (the edge sample is not repeated)
 *   frames      frames = 1 + len / hop, written to mel_lens[b] (int64); Tmax = 1 + Nmax / hop rows per utterance in `out`.
 *               len <= n_fft/2 cannot be reflected: mel_lens[b] = 0 and zero rows, nothing of the utterance is read
 *   window      periodic Hann, 0.5 - 0.5 cos(2 pi n / win_length), zero-padded to n_fft, left pad (n_fft - win_length) / 2
 *   transform   X[k] = sum_n w[n] x[n] exp(-2 pi i k n / n_fft), k = 0 .. n_fft/2, fp32, in LDS; n_fft in {256, 512, 1024, 2048}
 *   mel         filter f = sum_i weights[offset_f + i] * |X[first_f + i]|, i = 0 .. count_f - 1 in this order
 *   value       TTTS_AUDIO_LOGMEL: log(max(mel, clip_val)) -- a mel <= clip_val gives exactly (float)log((double)clip_val) --
 *               then, mean_std != NULL, (x - mean) / (std + 1e-8) with mean = mean_std[0], std = mean_std[1] read on the device;
 *               out is (B, Tmax, n_mels).  TTTS_AUDIO_MAGNITUDE: |X[k]|, out is (B, Tmax, n_fft/2 + 1), mean_std is not read.
 *               Rows at or beyond mel_lens[b] are written as zeros in both modes.
 * `tables` is one device buffer of 4-byte words that the caller fills (transformertts_amd.audio builds it in fp64 and rounds):
 *   8 header words (0x4C454D54, n_fft, win_length, n_mels, nnz, 0, 0, 0) | window (n_fft floats) | cos, -sin of 2 pi k / (n_fft/2),
 *   k < n_fft/2 (n_fft/2 floats each) | cos, -sin of 2 pi k / n_fft, k <= n_fft/4 (n_fft/4 + 1 floats each) | first_f, count_f,
 *   offset_f (n_mels int32 each) | weights (nnz floats).  ttts_audio_tables_bytes gives its size (0 for an n_fft outside the set
 *   or a size < 1); ttts_audio_tables_check reads a HOST copy before it is uploaded and refuses an n_fft outside the set,
 *   win_length > n_fft or < 1, a size or header that does not match, a filter that leaves the n_fft/2 + 1 bins, offsets that
 *   are not the running sum of the counts.  The kernel clamps what it reads from the table, so no table makes it load out of bounds.
 * ttts_logmel_stats: sums[b] = (sum x, sum x^2) in double over the rows < mel_lens[b] (clamped to [0, Tmax]) of mel
 *   (B, Tmax, n_mels) contiguous, one workgroup per utterance, a fixed order, no atomics: two calls agree bit for bit.  The data
 *   set's mean = S / count, std = sqrt(Q / count - mean^2 + 1e-8) over the utterances' sums (preprocess.py:45-72).
 * No host read, no allocation, capturable into a HIP graph.  Refused before any launch, naming the value: null pointers
 * (mean_std may be NULL), B < 1 or a size < 1, n_fft not in the supported set, hop < 1 or hop > n_fft, an unknown mode, a batch
 * stride < Nmax, Nmax > 2^30, n_mels > 512 or nnz > 4096 (the filters are staged in LDS), clip_val <= 0, misaligned pointers (4 bytes;
 * 8 for wave_lens, mel_lens and sums), B > 65535 (the grid). */
#define TTTS_AUDIO_LOGMEL 0
#define TTTS_AUDIO_MAGNITUDE 1
size_t ttts_audio_tables_bytes(int n_fft, int n_mels, int nnz);
int ttts_audio_tables_check(const void* host_tables, size_t bytes, int n_fft, int win_length, int n_mels, int nnz);
int ttts_logmel(const float* wave, int64_t ld_batch, const int64_t* wave_lens, int B, int Nmax, int n_fft, int hop, int n_mels,
                int nnz, const void* tables, float clip_val, const float* mean_std, float* out, int64_t* mel_lens, int mode,
                void* stream);
int ttts_logmel_stats(const float* mel, const int64_t* mel_lens, int B, int Tmax, int n_mels, double* sums, void* stream);
/* ---- Griffin-Lim vocoder: a ragged batch of (normalised) log-mels back to waveforms (ABI v24; vocoder.hip, audio_common.h,
 * fft_lds.h): librosa.feature.inverse.mel_to_audio's fast Griffin-Lim with a pseudo-inverse mel basis, restated from the
 * documented definitions on the front end's tables and conventions.  bins = n_fft/2 + 1.
 *   magnitude   ttts_mel_to_magnitude: x = mel[b, t, :] (row t of utterance b at mel + b * ld_batch + t * ld_row, n_mels floats);
 *               mean_std != NULL: x * (std + 1e-8) + mean, read on the device from the front end's two floats; m[f] = expf(x[f]);
 *               mag[k] = max(sum_f pinv[k, f] * m[f], floor), f ascending; pinv is (bins, n_mels) fp32 row-major (the caller forms
 *               numpy.linalg.pinv of the mel basis in fp64 and rounds once).  frames_b = melspec_lens[b] clamped to [0, Tmax].  A
 *               row is vocodable iff (frames_b - 1) * hop > n_fft/2 -- anything shorter the front end could not reflect -- and
 *               keeps its frames; otherwise its effective frames are 0.  The effective frames are written to `frames` (int64);
 *               the two transforms read that array, never melspec_lens.  mag is (B, Tmax, bins); rows at or beyond the effective
 *               frames are zeros, nothing at or beyond a length is read.
 *   inverse     ttts_istft: spec is (B, Tmax, bins, 2) fp32 (re, im); x_t = irfft(spec[b, t], n_fft), the imaginary parts of bin 0
 *               and bin n_fft/2 ignored, the 1/n_fft applied here; with g' = t * hop + n over the frames t < frames_b in ascending
 *               t: y[g'] = sum_t w[n] x_t[n], env[g'] = sum_t w[n]^2; wave[b, g] = env > 1.17549435e-38f ? y / env : y at
 *               g' = g + n_fft/2 for g < wave_lens[b] = frames_b > 0 ? (frames_b - 1) * hop : 0 (written, int64); samples from
 *               there to Nmax = (Tmax - 1) * hop are zeros; wave is (B, Nmax).  Any frames_b >= 1 is taken (clamped to [0, Tmax]).
 *               A gather: a workgroup owns 2 * n_fft consecutive samples and adds the frames that touch them in ascending t, so a
 *               sample's bits do not depend on the grid, the batch or the call.
 *   forward     ttts_stft_project: reb = STFT(wave) exactly as ttts_logmel frames, reflects, windows and transforms; wave is
 *               (B, Nmax) at stride ld_batch, Tmax = 1 + Nmax / hop.  Give wave_lens (then frames = 1 + len / hop by the front
 *               end's rule, 0 for len <= n_fft/2) or frames (then len = (frames - 1) * hop, and frames whose len <= n_fft/2 count
 *               as 0): one of them.  frames_out != NULL receives the frames used.  mag == NULL: spec = reb, rows beyond the frames
 *               zeros -- the complex STFT.  mag given ((B, Tmax, bins)): t = reb - (momentum / (1 + momentum)) * prev;
 *               prev <- reb in place ((B, Tmax, bins, 2)); a2 = |t|^2; spec = mag * (a2 > 1e-30f ? t * rsqrt(a2) : (1, 0)); rows
 *               beyond the frames are not touched.  momentum in [0, 1); momentum = 0 needs no prev.
 *   Griffin-Lim spec = mag * init (unit phases); prev = 0; n_iter times { wave = istft(spec); project }; wave = istft(spec):
 *               n_iter + 1 inverse and n_iter forward launches (transformertts_amd.audio.Vocoder).
 * `tables` is the front end's table buffer (window, roots, w^k; the filter sections are not read).  ttts_vocoder_pinv_check reads a
 * HOST copy of pinv before it is uploaded: the size and finite values.  No host read, no allocation, no atomics, the same bits
 * on every call, capturable into a HIP graph.  Refused before any launch, with a message: null pointers (mean_std, mag, prev,
 * frames_out and one of wave_lens / frames may be NULL), B < 1 or a size < 1, n_fft not in {256, 512, 1024, 2048}, hop < 1 or
 * hop > n_fft, Tmax < 2, more than 2^30 samples, n_mels > 512, strides that do not cover a row, floor <= 0, momentum outside
 * [0, 1), momentum > 0 without prev, prev or momentum without mag, misaligned pointers (4 bytes; 8 for spec, prev and the int64
 * arrays), B > 65535 (the grid). */
int ttts_vocoder_pinv_check(const void* host_pinv, size_t bytes, int n_fft, int n_mels);
int ttts_mel_to_magnitude(const float* mel, int64_t ld_row, int64_t ld_batch, const int64_t* melspec_lens, int B, int Tmax, int n_fft,
                          int hop, int n_mels, const float* pinv, const float* mean_std, float floor, float* mag, int64_t* frames,
                          void* stream);
int ttts_istft(const float* spec, const int64_t* frames, int B, int Tmax, int n_fft, int hop, const void* tables, float* wave,
               int64_t* wave_lens, void* stream);
int ttts_stft_project(const float* wave, int64_t ld_batch, const int64_t* wave_lens, const int64_t* frames, int B, int Nmax, int n_fft,
                      int hop, const void* tables, const float* mag, float* prev, float momentum, float* spec, int64_t* frames_out,
                      void* stream);
/* ---- Band-limited resampler: a ragged batch of waveforms from one rate to another (resample.hip; additive, the ABI version
 * stays 24): windowed-sinc (Kaiser) interpolation in polyphase form, the family of resampy's kaiser_best and torchaudio's
 * sinc_interp_kaiser, restated from the definition.
 *   rates       g = gcd(orig, new), L = new / g, M = orig / g, L != M; cutoff s = rolloff * min(1, L / M)
 *   kernel      k(u) = sinc(u) * w(u / zeros), sinc(u) = sin(pi u) / (pi u), w(v) = I0(beta sqrt(1 - v^2)) / I0(beta) for |v| < 1,
 *               else 0; W = ceil(zeros / s), K = 2 W + 2 taps
 *   table       h[r][k] = s * k(s * ((W - k) + p_r / L)), p_r = (r M) mod L, built by the caller in fp64 and rounded to fp32 once,
 *               tap-major: table[k * L + r], L * K floats.  ttts_resample_table_check reads a HOST copy: the size, finite values,
 *               K even and at least 4, gcd(L, M) == 1.
 *   sum         output j of utterance b sits at input time j M / L: q = floor(j M / L) (formed in 64 bits), r = j mod L,
 *               y[b, j] = sum_{k = 0 .. K-1} table[k * L + r] * x[b, q - W + k], ascending k, fp32 fused multiply-adds from 0;
 *               x[b, i] counts as 0 for i < 0 or i >= len_b and such a sample is never loaded
 *   lengths     len_b = wave_lens[b] clamped to [0, Nmax]; out_lens[b] = ceil(len_b L / M) (int64, written); out is (B, Nout) at
 *               stride ld_out with Nout = ceil(Nmax L / M); samples from out_lens[b] to Nout are zeros
 * One launch, grid (ceil(Nout / tile), B) with tile = ttts_resample_tile outputs per workgroup; a workgroup wholly behind
 * out_lens[b] only writes its zeros.  No host read, no allocation, no atomics, the same bits whatever the grid, the batch or the
 * call, capturable into a HIP graph.  Refused before any launch, with a message that names the value: null pointers, B < 1 or
 * B > 65535 (the grid), Nmax < 1 or Nmax > 2^30, L < 1 or M < 1, L == M, L > 1024 (the table), max(L / M, M / L) > 8 and K > 1280
 * (the input span a workgroup stages: at most 1023 * 8 + 2 + 1280 floats of LDS), K odd or K < 4, strides that do not cover a
 * row, misaligned pointers (4 bytes; 8 for the int64 arrays). */
size_t ttts_resample_table_bytes(int L, int K);
int ttts_resample_table_check(const void* host_table, size_t bytes, int L, int M, int K);
int ttts_resample_tile(void);
int ttts_resample(const float* wave, int64_t ld_batch, const int64_t* wave_lens, int B, int Nmax, int L, int M, int K,
                  const float* table, float* out, int64_t ld_out, int64_t* out_lens, void* stream);
/* ---- Frame pitch and energy: YIN F0, voicing, aperiodicity and the STFT frame energy of a ragged batch of waveforms, and the
 * phoneme-level means of such frame values (pitch.hip; additive, the ABI version stays 24).  YIN restated from its definition.
 *   framing     the front end's: pitch frame t of utterance b holds x_n = wave[g], g = t * hop - F/2 + n, n < F = frame_length;
 *               g < 0 reads -g, g >= len_b reads 2 (len_b - 1) - g.  len_b = wave_lens[b] clamped to [0, Nmax]; frames_b =
 *               1 + len_b / hop, or 0 when len_b <= max(F, n_fft) / 2 (written to `frames`, int64); the outputs are (B, Tmax) with
 *               Tmax = 1 + Nmax / hop, rows at or beyond frames_b zeros.  Samples at or beyond len_b are never read.
 *   difference  d(tau) = sum_{j < W} (x_j - x_{j+tau})^2 for tau = 1 .. tau_max, W = window, differences squared in fp32 -- never
 *               e(0) + e(tau) - 2 acf(tau).  Summed over blocks of BL samples (ascending j, fused multiply-adds from 0 inside a
 *               block), the block partials added in ascending order; BL = ttts_pitch_block(...): hop when hop divides W, W / hop <= 8
 *               and the shared partials fit the workgroup's LDS, else W.
 *   normalised  d'(tau) = d(tau) * tau / sum_{k <= tau} d(k); 1 where that running sum is 0 (a silent frame)
 *   lag         tau_0 = the first tau in [tau_min, tau_max] with d'(tau) < threshold.  With one the frame is voiced and tau* is
 *               reached from tau_0 by stepping up while tau + 1 <= tau_max and d'(tau + 1) < d'(tau); without one it is unvoiced
 *               and tau* is the first argmin of d' over [tau_min, tau_max].
 *   outputs     voiced (uint8, 0 / 1); aperiodicity = d'(tau*); f0 = sample_rate / (tau* + s) when voiced, exactly 0 otherwise;
 *               s = clamp(0.5 (a - c) / (a - 2 b + c), -0.5, 0.5) with a, b, c = d'(tau* - 1), d'(tau*), d'(tau* + 1) when
 *               tau_min < tau* < tau_max and a - 2 b + c > 0, else 0
 *   energy      sqrt(sum_{k = 0 .. n_fft/2} |X[k]|^2) with X the front end's STFT of the n_fft samples centred at t * hop, from
 *               y_n = hann[n] * x_n as (n_fft * sum y^2 + (sum y)^2 + (sum (-1)^n y)^2) / 2; `hann` is the front end's window:
 *               n_fft floats, the periodic Hann of win_length zero-padded and centred
 *   means       ttts_segment_mean: phoneme p < phoneme_lens[b] of utterance b covers frames [c_p, c_p + dur_p), c the exclusive
 *               prefix sum of durations[b, :] ((B, Pmax) int64, negative counts as 0), clipped to frames[b] (clamped to [0, Tmax]);
 *               mean[b, p] = the fp32 sum of values[b, t] over those frames (those with mask[b, t] != 0 when a mask is given) in
 *               ascending t, divided by their number counts[b, p] (int32); 0 when none counts; phonemes at or beyond
 *               phoneme_lens[b] get 0 and 0.  values is (B, Tmax) fp32 at stride ld_values, mask (B, Tmax) uint8 at ld_mask.
 * ttts_pitch_energy is one launch over the ragged batch, a workgroup per ttts_pitch_frames(...) consecutive frames of an
 * utterance, ttts_pitch_block(...) the block length BL of its sums (both 0 for a shape the entry refuses); ttts_pitch_lags is the number of neighbouring lags a thread carries (a build constant, for the benchmark's
 * label).  ttts_segment_mean is one launch, a wave per utterance.  No host read, no allocation, no atomics, the same bits
 * whatever the grid, the batch or the call, capturable into a HIP graph.  Refused before any launch, with a message that names
 * the value: null pointers (mask may be NULL), B < 1 or B > 65535 (the grid), Nmax < 1 or Nmax > 2^30, n_fft not in {256, 512,
 * 1024, 2048}, win_length outside [1, n_fft], frame_length odd, < 2 or > 4096, hop < 1 or hop > frame_length, window < 1,
 * tau_min < 2, tau_min >= tau_max, window + tau_max > frame_length, threshold outside (0, 1), sample_rate <= 0, Tmax or Pmax
 * < 1, strides that do not cover a row, misaligned pointers (4 bytes; 8 for the int64 arrays). */
int ttts_pitch_lags(void);
int ttts_pitch_frames(int n_fft, int hop, int frame_length, int window, int tau_max);
int ttts_pitch_block(int n_fft, int hop, int frame_length, int window, int tau_max);
int ttts_pitch_energy(const float* wave, int64_t ld_batch, const int64_t* wave_lens, int B, int Nmax, int n_fft, int win_length, int hop,
                      int frame_length, int window, int tau_min, int tau_max, float sample_rate, float threshold, const float* hann,
                      float* f0, uint8_t* voiced, float* aperiodicity, float* energy, int64_t* frames, void* stream);
int ttts_segment_mean(const float* values, int64_t ld_values, const int64_t* durations, const int64_t* phoneme_lens,
                      const int64_t* frames, const uint8_t* mask, int64_t ld_mask, int B, int Tmax, int Pmax, float* mean,
                      int32_t* counts, void* stream);
/* ---- Variance adaptor of a FastSpeech-2-style student: length regulator and its transpose, durations from predicted
 * log-durations, quantised pitch / energy embeddings, three masked regression losses (variance.hip; additive, the ABI version
 * stays 24).  Throughout pl_b = phoneme_lens[b] clamped to [0, Pmax]; dur'_p = max(durations[b, p], 0) for p < pl_b, else 0;
 * c the exclusive prefix sum of dur'; frames_b = min(sum dur', Tmax).
 *   regulator   ttts_length_regulate_fwd: y[b, t, :] = x[b, p(t), :] for t < frames_b, where c_p <= t < c_p + dur'_p; exact zeros
 *               from frames_b on.  x is (B, Pmax, D) fp32 at row stride ld_row and batch stride ld_batch (floats), y (B, Tmax, D)
 *               packed; mel_lens[b] = frames_b (int64); index[b, t] = p(t), -1 from frames_b on (int32).  One launch, a
 *               workgroup per ttts_length_regulate_frames frames of an utterance.
 *   transpose   ttts_length_regulate_bwd: dx[b, p, :] = the fp32 sum of dy[b, t, :] over t in [c_p, min(c_p + dur'_p, frames_b))
 *               in ascending t, one plain add per frame from 0.f -- bit for bit a sequential fp32 loop; exact zeros for a phoneme
 *               without a frame and for p >= pl_b.  dy (B, Tmax, D) and dx (B, Pmax, D) packed; accumulate != 0: dx += that sum.
 *   durations   ttts_durations_from_log: d = rint((exp(log_d) - 1) alpha) evaluated in fp64 from the fp32 input, halves to even,
 *               clamped to [0, 2^31 - 1]; 0 for a NaN or infinite log_d; then max(d, min_duration) for p < pl_b; 0 for p >= pl_b.
 *   embedding   ttts_variance_embed_fwd: i = the number of pitch_bins (n_pitch - 1 ascending fp32 boundaries) strictly below
 *               pitch[b, p] -- torch.bucketize with right=False; a NaN value gives 0 -- and j alike for the energy; y = (x +
 *               pitch_table[i]) + energy_table[j] in that order for p < pl_b, y = x behind it; pitch_ids / energy_ids (B, Pmax)
 *               int64 hold i / j, -1 behind it.  A NULL table skips that feature: its other pointers are not touched.  The
 *               backward needs no kernel of its own: dx = dy, and the table gradients are ttts_embedding_bwd on the saved ids (it
 *               compares ids for equality with a table row, so -1 contributes nowhere and is never an index).
 *   loss        ttts_variance_loss_fwd: out[0 .. 2] = the means over the n = sum_b pl_b valid phonemes of (log_d_pred -
 *               fp32(log_fp64(dur' + 1)))^2, (pitch_pred - pitch_target)^2, (energy_pred - energy_target)^2, all (B, Pmax) packed;
 *               out[3] = (w_d out[0] + w_p out[1]) + w_e out[2]; exactly 0 when n = 0.  One workgroup of 1024 threads: thread i
 *               adds the squares of the flat elements i, i + 1024, ... in ascending order (plain multiply, plain add, from 0.f,
 *               elements behind a length skipped); the 64 lanes of a wave meet in a butterfly (lane l adds lane l ^ 32, then
 *               l ^ 16, ... l ^ 1); the 16 wave sums are added in ascending order from 0.f; then one division by (float)n.
 *               ttts_variance_loss_bwd: with gout the gradient of the four outputs, s_k = (2 / (float)n) * (gout[k] + w_k *
 *               gout[3]) and d_pred_k = s_k * (pred_k - target_k) for p < pl_b, exact 0 behind it and everywhere when n = 0;
 *               every product, sum and quotient rounded on its own.  One launch writes the three gradients.
 * No host read, no allocation, no atomics, the same bits whatever the grid, the batch or the call, capturable into a HIP graph;
 * nothing at or behind a length is read (the embedding passes x rows through).  Refused before any launch, with a message that
 * names the value: null pointers, B outside [1, 65535], Pmax outside [1, 4096], Tmax outside [1, 2^20], D outside [4, 4096] or
 * no multiple of 4, n_pitch / n_energy outside [2, 4096], strides that do not cover a row or are no multiple of 4, alpha not
 * positive and finite, min_duration < 0, weights not finite, misaligned pointers (16 bytes for the float rows, 8 for int64, 4
 * for the other arrays). */
int ttts_length_regulate_frames(void);
int ttts_length_regulate_fwd(const float* x, int64_t ld_row, int64_t ld_batch, const int64_t* durations, const int64_t* phoneme_lens,
                             int B, int Pmax, int Tmax, int D, float* y, int64_t* mel_lens, int32_t* index, void* stream);
int ttts_length_regulate_bwd(const float* dy, const int64_t* durations, const int64_t* phoneme_lens, int B, int Pmax, int Tmax, int D,
                             float* dx, int accumulate, void* stream);
int ttts_durations_from_log(const float* log_d, const int64_t* phoneme_lens, int B, int Pmax, float alpha, int64_t min_duration,
                            int64_t* durations, void* stream);
int ttts_variance_embed_fwd(const float* x, int64_t ld_row, int64_t ld_batch, const float* pitch, const float* energy,
                            const float* pitch_bins, int n_pitch, const float* energy_bins, int n_energy, const float* pitch_table,
                            const float* energy_table, const int64_t* phoneme_lens, int B, int Pmax, int D, float* y,
                            int64_t* pitch_ids, int64_t* energy_ids, void* stream);
int ttts_variance_loss_fwd(const float* log_d_pred, const int64_t* durations, const float* pitch_pred, const float* pitch_target,
                           const float* energy_pred, const float* energy_target, const int64_t* phoneme_lens, int B, int Pmax, float w_d,
                           float w_p, float w_e, float* out, void* stream);
int ttts_variance_loss_bwd(const float* log_d_pred, const int64_t* durations, const float* pitch_pred, const float* pitch_target,
                           const float* energy_pred, const float* energy_target, const int64_t* phoneme_lens, int B, int Pmax, float w_d,
                           float w_p, float w_e, const float* gout, float* d_log_d, float* d_pitch, float* d_energy, void* stream);
/* ---- mel loss of the student (csrc/student_loss.hip; additive, the ABI version stays 24) --------------------------------
 * The masked mean absolute and mean squared error between two ragged mel batches.  pred is (B, T, M) fp32 read through
 * (ld_row_pred, ld_batch_pred), target (B, Tt, M) through its own pair -- the float4-row rule of the variance entries: rows of
 * M floats a multiple of 4 floats apart, utterances a multiple of 4 floats apart that cover T resp. Tt rows, 16-byte aligned
 * bases.  pred_lens, target_lens: (B,) int64 on the device.
 *   n_b = clamp(min(pred_lens[b], target_lens[b]), 0, min(T, Tt)); N = sum_b n_b; den = (float)(N M)
 *   out[0] mae = sum |pred - target| / den, out[1] mse = sum (pred - target)^2 / den over b, t < n_b, m; both exactly 0 when N = 0
 *   out[2] mel = w_mae mae + w_mse mse; out[3] total = mel + extra[0] (extra NULL: mel itself); frames[0] = N
 * ttts_mel_loss_fwd is two launches: partial sums per workgroup into `workspace` (ttts_mel_loss_workspace_bytes; utterances are
 * cut into chunks of ttts_mel_loss_rows() frames, min(B ceil(min(T, Tt) / rows), ttts_mel_loss_max_workgroups()) workgroups
 * stride over the chunks -- the grid follows from the shapes alone), then one workgroup of ttts_mel_loss_sweep() threads that
 * adds the partials in ascending order and takes N as an integer sum.  The order of every sum is stated at the top of the
 * source file.  ttts_mel_loss_bwd is one element-wise launch: with the upstream gradients of the four outputs as device scalars
 * (NULL counts as 0), G = g_total + g_mel, dpred[b, t, m] = sign(d) ((G w_mae + g_mae) / den) + ((2 (G w_mse + g_mse)) / den) d
 * for t < n_b with d = pred - target and sign(0) = 0; dpred is (B, T, M) contiguous and holds exact zeros at and behind n_b,
 * and everywhere when N = 0.  The gradient of extra is g_total (the caller's).
 * No atomics, no allocation, no host read, the same bits on every call, capturable; nothing at or behind n_b is read in either
 * operand.  Refused before any launch, with a message that names the value: null required pointers, B outside [1, 65535], T or Tt
 * outside [1, 2^20], M outside [4, 4096] or no multiple of 4, strides that do not cover a row or are no multiple of 4,
 * misaligned pointers, a workspace that is too small, weights that are not finite.  ttts_mel_loss_workspace_bytes returns 0 for
 * a shape the entries refuse. */
int ttts_mel_loss_rows(void);
int ttts_mel_loss_sweep(void);
int ttts_mel_loss_max_workgroups(void);
size_t ttts_mel_loss_workspace_bytes(int B, int T, int Tt, int M);
int ttts_mel_loss_fwd(const float* pred, int64_t ld_row_pred, int64_t ld_batch_pred, const float* target, int64_t ld_row_target,
                      int64_t ld_batch_target, const int64_t* pred_lens, const int64_t* target_lens, int B, int T, int Tt, int M,
                      float w_mae, float w_mse, const float* extra, float* out, int64_t* frames, void* workspace,
                      size_t workspace_bytes, void* stream);
int ttts_mel_loss_bwd(const float* pred, int64_t ld_row_pred, int64_t ld_batch_pred, const float* target, int64_t ld_row_target,
                      int64_t ld_batch_target, const int64_t* pred_lens, const int64_t* target_lens, int B, int T, int Tt, int M,
                      float w_mae, float w_mse, const float* g_mae, const float* g_mse, const float* g_mel, const float* g_total,
                      float* dpred, void* stream);
/* ttts_heads_pad / ttts_heads_unpad with the padded width as an argument (ABI v17): width 64 (head_dim 1 .. 64) or 128
 * (head_dim 1 .. 128); dst resp. src is (rows, H*width).  The operands of the attention call sites above when head_dim is not
 * the kernels' own width. */
int ttts_heads_pad_w(const float* src, int64_t ld_src, float* dst, int64_t rows, int H, int head_dim, int width, void* stream);
int ttts_heads_unpad_w(const float* src, float* dst, int64_t ld_dst, int64_t rows, int H, int head_dim, int width, void* stream);
/* ---- attention on head-image operands (ABI v11; attention_img.hip): the same call sites as ttts_attention_fwd_h3 /
 * ttts_attention_bwd_h3 (encoder self-attention and decoder `_sa_block`, torch/nn/modules/transformer.py:961-978,1158-1175 ->
 * torch/nn/functional.py:6629; the decoder's `_mha_block`, model/layers.py:54-74), head_dim 64.  q / k / v point at head 0 of
 * their section inside a head image (row strides ld* in 4-byte cells; a packed q/k/v image is passed as three pointers d cells
 * apart), *_inv at the [head][rows] inverse scales of that section (B * Tq rows per head plane on the q side, B * Tk on the key
 * side), v_amax at the TTTS_AMAX_SLOTS partial maxima of |v| (the section array ttts_linear_fwd_h3d_img filled).  o, lse, attn,
 * o_amax_out as ttts_attention_fwd_h3.  rowstat_out: (5, B, H, Tq) floats -- the three planes of ttts_attention_fwd_h3 plus
 * the query row's exponent multiplier 2^-e_q * q_scale * log2(e) and score multiplier 2^-e_q * q_scale; the backward
 * requires it (it forms the forward's own probabilities from bit-identical accumulators).  q_inv_rows / k_inv_rows / stat_plane (ABI v12): rows per head plane of the inverse scales and
 * floats per plane of the row statistics -- 0: B * Tq, B * Tk, B * H * Tq; larger when the batch is the FIRST part of a bigger
 * image (the encoder of both forwards of a training step run as one batch: ops.twin). */
int ttts_attention_fwd_img(const void* q, const void* k, const void* v, const float* q_inv, const float* k_inv,
                           const float* v_inv, float* o, float* lse, float* attn, const int64_t* key_lens, int B, int H, int Tq,
                           int Tk, int ldq, int ldk, int ldv, int ldo, int causal, float q_scale, float drop_p, uint64_t seed,
                           const uint64_t* step_seed, const float* v_amax, float* o_amax_out, float* rowstat_out, int64_t q_inv_rows, int64_t k_inv_rows, int64_t stat_plane,
                           void* stream);
/* dq, dk, dv in fp32 (strides ldd*) from d_o; o / d_o fp32; do_amax = partial maxima of |d_o|; delta (B,H,Tq) is scratch.
 * q_splits > 1 (dk / dv the two halves of one packed (B, Tk, 2 H 64) gradient; causal too since round 6): the dK / dV kernel splits the query
 * range over q_splits workgroups per key block, partial sums in dkv_partials, one fixed-order reduction at the end. */
int ttts_attention_bwd_img(const void* q, const void* k, const void* v, const float* q_inv, const float* k_inv,
                           const float* v_inv, const float* o, const float* d_o, const float* rowstat, float* delta, float* dq,
                           float* dk, float* dv, const int64_t* key_lens, int B, int H, int Tq, int Tk, int ldq, int ldk, int ldv,
                           int ldo, int lddq, int lddk, int lddv, int causal, float q_scale, float drop_p, uint64_t seed,
                           const uint64_t* step_seed, const float* do_amax, float* dq_amax_out, float* dkv_amax_out,
                           float* dkv_partials /* NULL, or q_splits x B x Tk x lddk floats */, int q_splits /* 1: no split */,
                           int64_t q_inv_rows, int64_t k_inv_rows, int64_t stat_plane, void* stream);

/* ------------------------------------------------------------------ small row / element-wise pieces
 * nn.Embedding gather / scatter-add (model/model.py:168,288; no padding_idx) */
int ttts_embedding_fwd(const int64_t* ids, const float* table, float* out, int64_t n, int vocab, int d,
                       float* out_amax_out /* NULL, or zeroed TTTS_AMAX_SLOTS floats: max|out| */, void* stream);
int ttts_embedding_bwd(const int64_t* ids, const float* dout, float* dtable, int64_t n, int vocab, int d, int accumulate,
                       void* stream);
/* PositionalEncoding.forward (model/model.py:91-97): y = drop(x + alpha * pe[t]) */
int ttts_posenc_fwd(const float* x, const float* pe, const float* alpha, float* y, int B, int T, int d, float drop_p,
                    uint64_t seed, const uint64_t* step_seed, float* y_amax_out /* NULL, or zeroed TTTS_AMAX_SLOTS floats */, void* stream);
size_t ttts_posenc_bwd_workspace_bytes(void);
int ttts_posenc_bwd(const float* dy, const float* pe, float* dx, float* dalpha, float* ws, size_t ws_bytes, int B, int T,
                    int d, float drop_p, uint64_t seed, const uint64_t* step_seed, int accumulate, void* stream);
/* dx = dy * 1[out > 0] / (1-p): backward of drop(relu(.)) given the forward output.  dx_amax_out (NULL, or zeroed
 * TTTS_AMAX_SLOTS floats): also leave the partial maxima of |dx| behind -- the dynamic pre-scale input of
 * the fp16x3 gradient GEMMs that consume dx -- without a second pass over it. */
int ttts_relu_dropout_bwd(const float* dy, const float* out, float* dx, int64_t n, float drop_p, float* dx_amax_out,
                          void* stream);
/* dx = dy * keep(seed, i) / (1-p); dx_amax_out as above */
int ttts_dropout_bwd(const float* dy, float* dx, int64_t n, float drop_p, uint64_t seed, const uint64_t* step_seed,
                     float* dx_amax_out, void* stream);
/* p[0 .. nbytes) = 0 by a fill kernel on the stream (the flat gradient bucket and the partial-maxima arrays at the start of
 * a step; p and nbytes multiples of 4).  Deliberately not hipMemsetAsync: see csrc/elementwise.hip. */
int ttts_zero(void* p, size_t nbytes, void* stream);
/* z = x + y */
int ttts_add(const float* x, const float* y, float* z, int64_t n, void* stream);
/* z = (x + y) + w: the gradient of a tensor with three consumers in one pass (autograd's own accumulation is one add per
 * extra consumer); n % 4 == 0 */
int ttts_add3(const float* x, const float* y, const float* w, float* z, int64_t n, void* stream);
/* ---- input side: device-side padding of a ragged batch --------------------------------------
 * Replaces the host loop of collate_fn (dataset.py:76-91) and the per-sample transpose of __getitem__
 * (dataset.py:64).  `ragged` holds the B utterances back to back, each in its on-disk (n_mels, len_b) row-major
 * layout (preprocess.py:36-42); frame_offsets (B+1, int64, device) are prefix sums of the lengths in frames.
 * out (B, Tmax, n_mels) fp32 is fully written (frames >= len_b are zero).  1 <= n_mels <= 128. */
int ttts_collate_melspec(const float* ragged, const int64_t* frame_offsets, float* out, int B, int Tmax, int n_mels,
                         void* stream);
/* phoneme ids: ragged int64 ids back to back, offsets (B+1); out (B, Pmax) int64, padded with 0 (dataset.py:79,88) */
int ttts_collate_phoneme(const int64_t* ragged, const int64_t* offsets, int64_t* out, int B, int Pmax, void* stream);

/* stop-token head, LinearNorm(d_model, 1) (model/model.py:226,313): y[m] = x[m,:].w + b, and its backward */
int ttts_rowdot_fwd(const float* x, const float* w, const float* b, float* y, int64_t M, int d, void* stream);
size_t ttts_rowdot_bwd_workspace_bytes(int d);
int ttts_rowdot_bwd(const float* dy, const float* x, const float* w, float* dx_accum, float* dw, float* db, float* ws,
                    size_t ws_bytes, int64_t M, int d, int accumulate, ttts_reduce_queue* queue, void* stream);

/* ------------------------------------------------------------------ loss and scheduled-sampling mix
 * TransformerTTSLoss.forward (loss.py:15-55): out4 = [total, pred_mel, post_mel, stop]; masked MSE over frames
 * t < lens[b] (x2, post weighted 0.5 in the total) + BCE-with-logits on the stop gate (1 at t = lens[b]-1) with
 * pos_weight, mean over valid frames.  ws keeps the normalisers for ttts_loss_bwd, which takes the upstream gradients
 * of the four outputs as device scalars (NULL = no gradient for that output) and writes the gradients of pred / post /
 * stop. */
size_t ttts_loss_workspace_bytes(void);
int ttts_loss_fwd(const float* pred, const float* post, const float* stop, const float* mel, const int64_t* lens,
                  float* out4, float* ws, size_t ws_bytes, int B, int T, int C, float pos_weight, void* stream);
int ttts_loss_bwd(const float* pred, const float* post, const float* stop, const float* mel, const int64_t* lens,
                  const float* ws, const float* g_total, const float* g_pred_mel, const float* g_post_mel, const float* g_stop,
                  float* dpred, float* dpost, float* dstop, int B, int T, int C, float pos_weight, void* stream);
/* block_mask + apply_teacher_forcing (utils/util.py:103-120): u is the (B,T) uniform draw; frame t takes the model's
 * prediction when any u[t-l_bar/2 .. t-l_bar/2+l_bar-1] < 1-p_tf (max_pool1d(k=l_bar, s=1, pad=l_bar/2)[:T]), the
 * ground truth otherwise, and zero beyond lens[b].  u == NULL: the draw (torch.rand of utils/util.py:108) is generated
 * in the kernel from `seed` (a counter-based uniform per frame).  st != NULL: p_tf and the seed word of the step are
 * read from device memory when the kernel runs (p_tf by value is ignored).
 * out_amax_out: NULL, or a caller-zeroed TTTS_AMAX_SLOTS-float array receiving max|out|. */
int ttts_sched_sampling_mix(const float* pred, const float* mel, const float* u, const int64_t* lens, float* out, int B,
                            int T, int C, float p_tf, int l_bar, uint64_t seed, const ttts_step_state* st,
                            float* out_amax_out, void* stream);

/* ------------------------------------------------------------------ optimizer over flat buffers
 * Global L2 norm of the flat gradient bucket (clip_grad_norm_, train.py:41) and one torch.optim.Adam step
 * (lightning_module.py:160-163: betas (0.9, 0.98), eps 1e-9, lr = Noam factor set by the host) on flat parameter /
 * gradient / moment buffers; the clip factor min(1, max_grad_norm / (norm + 1e-6)) is applied inside the step.
 * st != NULL: lr and step are read from the device-side step state when the kernel runs (graph replay). */
size_t ttts_grad_norm_workspace_bytes(void);
int ttts_grad_norm(const float* g, float* norm_out, float* ws, size_t ws_bytes, int64_t n, void* stream);
int ttts_adam_step(float* p, const float* g, float* exp_avg, float* exp_avg_sq, const float* grad_norm, int64_t n, float lr,
                   float beta1, float beta2, float eps, int64_t step, float max_grad_norm, const ttts_step_state* st,
                   void* stream);

/* ------------------------------------------------------------------ autoregressive decoding (one frame, M = B rows)
 * The K/V-cache loop of TransformerTTS.inference (transformertts_amd/model/model.py:310-338; the reference's loop is
 * model/model.py:354-384) as weight-streaming fp32 kernels whose frame index, length, threshold and stop
 * state come from `st` (ttts_decode_state above).  Plain fp32 FMA arithmetic, fixed summation orders that depend on neither
 * the row count nor the capacities (bitwise reproducible), no atomics.  Row strides are in floats; "(t - 1) * tstride" terms
 * use the t read from `st`.
 *
 * y = act(x . w^T + bias) (+ residual): the decoder's in / out projections, FFN linears and the cross-attention q projection
 * (torch/nn/functional.py in_proj / out_proj, torch/nn/modules/transformer.py _ff_block, model/layers.py:47-50 residuals).
 * Row m of x is x + m * ldx + (t - 1) * x_tstride; w is (N, K) in its state-dict layout (row slices of a packed in-projection
 * included); output column n < n_split goes to y + m * ldy + (t - 1) * y_tstride + n, column n >= n_split to
 * y2 + m * ldy2 + (t - 1) * y2_tstride + (n - n_split) -- the K/V columns of a self-attention in-projection written straight
 * into row t - 1 of that layer's cache.  K % 4 == 0, K <= 4096, x and w 16-byte aligned, ldx and x_tstride multiples of 4;
 * act NONE or RELU; bias, residual may be NULL; y2 may be NULL when n_split == N. */
int ttts_decode_linear(const float* x, int64_t ldx, int64_t x_tstride, const float* w, const float* bias, const float* residual,
                       int64_t ldr, float* y, int64_t ldy, int64_t y_tstride, float* y2, int64_t ldy2, int64_t y2_tstride,
                       int n_split, int M, int N, int K, int act, const ttts_decode_state* st, void* stream);
/* Frame in: out[B,d] = relu(relu(ys[:, t-1] . w1^T + b1) . w2^T + b2) + alpha[0] * pe[t - 1]: the decoder pre-net in eval mode
 * and the positional encoding of the newest frame (model/model.py:356-357 DecoderPreNet + PositionalEncoding, eval: no
 * dropout).  ys is (B, t_end, n_mels) with batch stride ld_ys; pe is the (rows, d) table; tmp is B x d floats of scratch
 * (16-byte aligned).  d and n_mels multiples of 4. */
int ttts_decode_frame_in(const float* ys, int64_t ld_ys, int n_mels, const float* w1, const float* b1, const float* w2,
                         const float* b2, const float* pe, const float* alpha, float* tmp, float* out, int B, int d,
                         const ttts_decode_state* st, void* stream);
/* Frame out: the heads (model/model.py:372-373 linear1 / linear2 on the last frame): ys[:, t] = x . w_mel^T + b_mel,
 * stop[b * ld_stop + t - 1] = x . w_stop + b_stop; then, when every row has 1 / (1 + expf(-stop)) >= st->stop_threshold
 * (torch.sigmoid(stop) >= threshold, model/model.py:379-380), st->stop_frame = t; finally st->t = t + 1. */
int ttts_decode_frame_out(const float* x, const float* w_mel, const float* b_mel, const float* w_stop, const float* b_stop,
                          float* ys, int64_t ld_ys, float* stop, int64_t ld_stop, int B, int d, int n_mels,
                          ttts_decode_state* st, void* stream);
/* y[M,d] = LayerNorm(x) (norm1 / norm2 / norm3 of the post-norm decoder layer, model/layers.py:46-50); d <= 1024 */
int ttts_decode_layernorm(const float* x, const float* gamma, const float* beta, float* y, int M, int d, float eps,
                          const ttts_decode_state* st, void* stream);
/* One query row per (utterance b, head h) against key rows 0 .. len - 1 (scaled dot-product attention of torch's MHA,
 * torch/nn/functional.py multi_head_attention_forward, q scaled by 1 / sqrt(head_dim)):
 *   q row b at q + b * ldq, head h at column h * head_dim; key / value row j of utterance b at k / v + b * ld_batch + j * ld_row
 *   (+ h * head_dim); len = lens[b] (int64, device; the memory key-padding mask of cross-attention) or, lens == NULL, the t of
 *   `st` (self-attention over the cache rows written so far); len is clamped to max_keys.  Keys at or past len are never read.
 *   out row b at out + b * ldo.  head_dim a multiple of 16 up to 128.
 * Keys are split in blocks of 64 whose partials go to the caller's workspace (ttts_decode_attention_workspace_bytes) and are
 * combined in block order by a second launch. */
size_t ttts_decode_attention_workspace_bytes(int B, int H, int head_dim, int max_keys);
int ttts_decode_attention(const float* q, int64_t ldq, const float* k, const float* v, int64_t ld_row, int64_t ld_batch,
                          const int64_t* lens, float* out, int64_t ldo, float* ws, size_t ws_bytes, int B, int H, int head_dim,
                          int max_keys, const ttts_decode_state* st, void* stream);

/* ---- ABI v16: per-utterance ends and alignment rows (decode.hip) ------------------------------------------------------
 * The same kernels with per-row state: `row_end` (B int64, device, required; see ttts_decode_state) names the rows that have
 * ended.  An ended row is neither read nor written -- its activation rows, its K/V cache row, ys, stop and map rows keep what
 * they held -- and its attention workgroups, combine and LayerNorm waves return before their first load; a row still running
 * gets bit for bit what the entry point without `row_end` gives it.  Row m of every (M, ...) operand belongs to row_end[m].
 * The GEMV and stop kernels read the end frames of four rows at once: `row_end` must be readable up to M rounded up to a
 * multiple of 4 entries (the entries behind M are read, never acted on and never written).
 * Everything else as ttts_decode_linear / _frame_in / _layernorm. */
int ttts_decode_linear_rows(const float* x, int64_t ldx, int64_t x_tstride, const float* w, const float* bias,
                            const float* residual, int64_t ldr, float* y, int64_t ldy, int64_t y_tstride, float* y2, int64_t ldy2,
                            int64_t y2_tstride, int n_split, int M, int N, int K, int act, const int64_t* row_end,
                            const ttts_decode_state* st, void* stream);
int ttts_decode_frame_in_rows(const float* ys, int64_t ld_ys, int n_mels, const float* w1, const float* b1, const float* w2,
                              const float* b2, const float* pe, const float* alpha, float* tmp, float* out, int B, int d,
                              const int64_t* row_end, const ttts_decode_state* st, void* stream);
int ttts_decode_layernorm_rows(const float* x, const float* gamma, const float* beta, float* y, int M, int d, float eps,
                               const int64_t* row_end, const ttts_decode_state* st, void* stream);
/* Frame out with per-row ends: heads and stop logits of the running rows as ttts_decode_frame_out.  st->flags without
 * TTTS_DECODE_PER_ROW: the decision of ttts_decode_frame_out (every running row at or above the threshold at this frame), row_end
 * is only read.  With it: a running row with 1 / (1 + expf(-stop)) >= st->stop_threshold gets row_end[b] = t (the first
 * crossing: the row is skipped afterwards), and st->stop_frame = t once no row is left running; st->t = t + 1 either way. */
int ttts_decode_frame_out_rows(const float* x, const float* w_mel, const float* b_mel, const float* w_stop, const float* b_stop,
                               float* ys, int64_t ld_ys, float* stop, int64_t ld_stop, int B, int d, int n_mels, int64_t* row_end,
                               ttts_decode_state* st, void* stream);
/* ttts_decode_attention with per-row ends and, map != NULL, the attention weights of this frame (the cross-attention maps the
 * training forward returns as `alignments`, model/layers.py:54-74 need_weights=True, average_attn_weights=False): row t - 1 of
 * plane (b, h) at map + (b * H + h) * map_ld_head + (t - 1) * map_ld_row receives softmax(q k^T / sqrt(head_dim)) over the keys
 * below len and zeros from there to max_keys.  The key blocks write their unnormalised weights and the combine launch rescales
 * them, block by block, with the factors it applies to the context vector.  map_rows: frames a plane holds (nothing is written
 * when t - 1 >= map_rows); map_ld_row >= max_keys, map_ld_head >= map_rows * map_ld_row.  map == NULL: no map code runs. */
int ttts_decode_attention_rows(const float* q, int64_t ldq, const float* k, const float* v, int64_t ld_row, int64_t ld_batch,
                               const int64_t* lens, float* out, int64_t ldo, float* ws, size_t ws_bytes, int B, int H, int head_dim,
                               int max_keys, const int64_t* row_end, float* map, int64_t map_ld_head, int64_t map_ld_row,
                               int map_rows, const ttts_decode_state* st, void* stream);
/* ---- ABI v21: an attention window on the cross-attention of batched synthesis (decode.hip) ---------------------------------
 * ttts_decode_attention_rows with, per utterance, a position that a guide head moves from frame to frame and a window around
 * it that the constrained heads cannot see out of: the windowed inference of attention TTS toolkits.  The reference has no
 * such mode (its `inference`, model/model.py:323-394, attends to every phoneme below the length at every frame); what this
 * restates is torch's MHA softmax (torch/nn/functional.py multi_head_attention_forward) under an additive -inf mask on the keys
 * outside  max(0, c - back) <= j <= min(len - 1, c + ahead)  (both ends inclusive) for the heads in win->head_mask.
 *   win: this layer's window struct, on the device, 8-byte aligned.  pos: int32 positions, row b at pos + b * ld_pos; it must hold
 *   t_end - 1 entries per row.  The centre c of frame t is pos[b, t - 2], and 0 at t = 1 (whatever pos holds then); a centre
 *   outside [0, len) is clamped into it, so a window always holds a key; a struct with a negative back or ahead makes the
 *   launch do nothing.  After the softmax the head win->guide_head (-1: none)
 *   writes pos[b, t - 1] = the key with its largest score among those it sees, the lowest one on equal scores: every layer of
 *   a frame reads the entry of the frame before, so there is no read-write race within a frame and pos needs no reset.
 * Key blocks that do not meet a constrained head's window return before any K/V load; keys outside it are not loaded; with a
 * map its row is exactly 0 outside the window up to max_keys.  A head that is not constrained, and every head under a window
 * that covers all keys, gets bit for bit what ttts_decode_attention_rows gives; an ended row writes neither out, map nor pos.
 * lens, row_end, win and pos are required; H <= 64.  The workspace is that of ttts_decode_attention_workspace_bytes (the
 * blocks' first-maximum keys use a slot it already has). */
int ttts_decode_attention_window(const float* q, int64_t ldq, const float* k, const float* v, int64_t ld_row, int64_t ld_batch,
                                 const int64_t* lens, float* out, int64_t ldo, float* ws, size_t ws_bytes, int B, int H,
                                 int head_dim, int max_keys, const int64_t* row_end, float* map, int64_t map_ld_head,
                                 int64_t map_ld_row, int map_rows, const ttts_decode_window* win, int32_t* pos, int64_t ld_pos,
                                 const ttts_decode_state* st, void* stream);
/* x (outer, T, C) contiguous: rows t >= lens[o / group] of slice o := 0 (lens int64 on the device, clamped to [0, T]; group
 * slices share one length: the heads of an attention map).  The frames behind each utterance's end in the outputs of a batched
 * synthesis, and in the post-net's input and every layer's output (a convolution over a zero-padded batch does not keep them
 * zero by itself).  16-byte stores when C % 4 == 0 and x is 16-byte aligned.  outer <= 65535. */
int ttts_mask_rows(float* x, const int64_t* lens, int64_t outer, int group, int64_t T, int64_t C, void* stream);

/* ---- additive (ABI 24): a length-masked Conv1d -> ReLU -> LayerNorm -> Dropout stage (predictor.hip) ------------------------
 * The building block of FastSpeech 2's variance predictors and FFT blocks, on (B, Pmax, C) fp32 rows of ragged utterances.
 * x is addressed through (ld_row, ld_batch) as the variance entries address it; pl_b = clamp(lens[b], 0, Pmax); w (Cout, Cin, taps)
 * and bias as nn.Conv1d holds them, gamma / beta as nn.LayerNorm.
 *   x'[b, p] = x[b, p] for p < pl_b, exact zeros elsewhere (memory at or behind a length is never read)
 *   z = bias + sum_j sum_ci w[co, ci, j] x'[b, p + j - taps / 2, ci];  r = max(z, 0);  mean, rstd = 1 / sqrt(var + eps) over co (biased)
 *   y = ((r - mean) rstd) gamma + beta, times keep_elem(seed ^ *step_seed, flat index in (B, Pmax, Cout)) / (1 - drop_p) when drop_p > 0
 * y (B, Pmax, Cout) is fully written: exact zeros for p >= pl_b.  r (B, Pmax, Cout), mean and rstd (B, Pmax): all three or none (NULL:
 * inference); zeros behind the lengths.  x_masked: NULL, or (B, Pmax, Cin) contiguous receiving x' (the weight gradient's operand).
 * One launch, an implicit GEMM on the fp32-input MFMA; a workgroup owns 32 rows of one utterance and all Cout columns, so no
 * utterance's result depends on another row of the batch.  Every sum has a fixed order.
 * 1 <= B <= 65535, 1 <= Pmax <= 4096, Cin a multiple of 4 in [4, 1024], Cout a multiple of 32 in [32, 256], taps odd in [1, 9]. */
int ttts_ragged_conv_norm_fwd(const float* x, int64_t ld_row, int64_t ld_batch, const int64_t* lens, const float* w, const float* bias,
                              const float* gamma, const float* beta, int B, int Pmax, int Cin, int Cout, int taps, float eps,
                              float drop_p, uint64_t seed, const uint64_t* step_seed, float* y, float* r, float* mean, float* rstd,
                              float* x_masked /* may be NULL */, void* stream);
/* Backward of the stage from dy (B, Pmax, Cout) contiguous (nothing behind a length is read): g = dy keep / (1 - drop_p); dgamma =
 * sum g x_hat, dbeta = sum g; dr = LayerNorm's backward; dz = dr [r > 0]; dbias = sum dz; dw[co, ci, j] = sum dz[b, p, co] x'[b, p + j
 * - taps / 2, ci] (ttts_conv1d_bwd_weight on dz and x_masked); dx[b, p, ci] = sum_j sum_co dz[b, p - j + taps / 2, co] w[co, ci, j] for
 * p < pl_b, exact zeros behind it ((B, Pmax, Cin) contiguous).  dx: NULL = not wanted.  dw: NULL = not wanted (x_masked is then
 * not read).  dw, dbias, dgamma, dbeta take `accumulate`.  ws: ttts_ragged_conv_norm_workspace_bytes(B, Pmax, Cin, Cout, taps). */
size_t ttts_ragged_conv_norm_workspace_bytes(int B, int Pmax, int Cin, int Cout, int taps);
int ttts_ragged_conv_norm_bwd(const float* dy, const float* r, const float* mean, const float* rstd, const float* x_masked,
                              const int64_t* lens, const float* w, const float* gamma, int B, int Pmax, int Cin, int Cout, int taps,
                              float drop_p, uint64_t seed, const uint64_t* step_seed, float* dx, float* dw, float* dbias,
                              float* dgamma, float* dbeta, float* ws, size_t ws_bytes, int accumulate, void* stream);

/* ---- additive (ABI 24): the conv feed-forward sublayer of an FFT block on ragged rows (predictor.hip) ---------
 * FastSpeech's position-wise feed-forward: two Conv1d layers, dropout on the branch, residual, LayerNorm.  x (B, Pmax, D) through
 * (ld_row, ld_batch); pl_b and x' as above; w1 (Chid, D, k1), b1, w2 (D, Chid, k2), b2 as nn.Conv1d holds them.
 *   h = max(conv_k1(x') + b1, 0)   (B, Pmax, Chid), exact zeros behind pl_b; required (the second launch reads it)
 *   z = conv_k2(h) + b2;  s = x' + z keep_elem(seed ^ *step_seed, flat index in (B, Pmax, D)) / (1 - drop_p)  (no multiply at drop_p 0)
 *   y = ((s - mean) rstd) gamma + beta over D (biased variance, two passes), exact zeros behind pl_b
 * Two launches of the stage's implicit GEMM: bias + ReLU in column blocks of 256, then bias + dropout + residual + LayerNorm with a
 * workgroup owning whole rows (the residual is read in the epilogue through x's strides, below the length only).  s (B, Pmax, D),
 * mean and rstd (B, Pmax): all three or none (NULL: inference).  x_masked: NULL, or (B, Pmax, D) contiguous receiving x'.
 * D a multiple of 32 in [32, 256], Chid a multiple of 32 in [32, 1024], k1 and k2 odd in [1, 9], Pmax <= 4096, B <= 65535. */
int ttts_ragged_conv_ffn_fwd(const float* x, int64_t ld_row, int64_t ld_batch, const int64_t* lens, const float* w1, const float* b1,
                             const float* w2, const float* b2, const float* gamma, const float* beta, int B, int Pmax, int D, int Chid,
                             int k1, int k2, float eps, float drop_p, uint64_t seed, const uint64_t* step_seed, float* h, float* y,
                             float* s, float* mean, float* rstd, float* x_masked /* may be NULL */, void* stream);
/* Backward of the sublayer from dy (B, Pmax, D) contiguous (nothing behind a length is read): ds = LayerNorm's backward (also the
 * residual's share of dx), dgamma = sum dy x_hat, dbeta = sum dy; dz2 = ds keep / (1 - drop_p); dz1 = conv(dz2, flipped w2) [h > 0];
 * dx = conv(dz1, flipped w1) + ds, exact zeros behind the lengths; dw2, db2 = ttts_conv1d_bwd_weight(dz2, h); dw1, db1 =
 * ttts_conv1d_bwd_weight(dz1, x_masked).  dx: NULL = not wanted.  dw1, db1, dw2, db2: all four or none (NULL: not wanted; x_masked is
 * then not read).  The six parameter gradients take `accumulate`.  ws: ttts_ragged_conv_ffn_workspace_bytes(B, Pmax, D, Chid, k1, k2). */
size_t ttts_ragged_conv_ffn_workspace_bytes(int B, int Pmax, int D, int Chid, int k1, int k2);
int ttts_ragged_conv_ffn_bwd(const float* dy, const float* s, const float* mean, const float* rstd, const float* h, const float* x_masked,
                             const int64_t* lens, const float* w1, const float* w2, const float* gamma, int B, int Pmax, int D, int Chid,
                             int k1, int k2, float drop_p, uint64_t seed, const uint64_t* step_seed, float* dx, float* dw1, float* db1,
                             float* dw2, float* db2, float* dgamma, float* dbeta, float* ws, size_t ws_bytes, int accumulate,
                             void* stream);

/* ---- additive (ABI 24): the layers of a HiFi-GAN generator on ragged rows, inference only (hifigan.hip) ---------
 * Activations are (B, Nmax, C) fp32, contiguous; pl_b = clamp(lens[b], 0, Nmax); rows at or behind pl_b count as zeros for the taps,
 * are never read (a NaN there does not leak) and come back as exact zeros, so every utterance is convolved as if it were alone,
 * zero-padded at its own ends.  Every sum has a fixed order; no atomics, no allocation, no host read.
 * The dilated convolution, an implicit GEMM on the fp32-input MFMA:
 *   z[b, n, co] = sum_j sum_ci w[j, ci, co] f(x[b, n + (j - taps / 2) dilation, ci]);  f = leaky_relu(., in_slope), in_slope = 1: none
 *   v = z + bias[co] + residual[b, n, co]   (bias, residual: NULL = absent; residual (B, Nmax, Cout), read below the length only)
 *   y = v (NULL: not wanted);  acc_mode 1: acc = v acc_scale;  acc_mode 2: acc = (acc + v) acc_scale;  acc_mode 0: acc must be NULL
 * w is the convolution's weight re-laid to (taps, Cin, Cout).  A ConvTranspose1d with stride u and u <= k <= 2 u taps is this entry
 * with 3 taps onto u Cout columns: (B, T, u Cout) row-major is (B, T u, Cout) row-major.  The reduction runs over chunks of 32 input
 * channels, inside a chunk over the taps; the fma chain is closed after every (chunk, tap) and the sums are added in that order.
 * Cin a multiple of 32 in [32, 512] or a multiple of 4 in [4, 128]; Cout a multiple of 32 in [32, 2048]; taps odd in [1, 11];
 * dilation in [1, 12]; Nmax <= 2^21; B <= 65535; every operand at most the bytes the query below returns. */
int ttts_hifigan_max_operand_bytes(void);
int ttts_hifigan_conv(const float* x, const int64_t* lens, const float* w, const float* bias, const float* residual, float* y,
                      float* acc, int B, int Nmax, int Cin, int Cout, int taps, int dilation, float in_slope, int acc_mode,
                      float acc_scale, void* stream);
/* y[b, n] = tanh(bias[0] + sum_j sum_ci w[j, ci] leaky_relu(x[b, n + j - taps / 2, ci], in_slope)) for n < pl_b, exact zeros behind
 * it: a generator's last layer, one output per row on the VALU.  w (taps, Cin); y (B, Nmax).  Cin a multiple of 32 in [32, 512]. */
int ttts_hifigan_post(const float* x, const int64_t* lens, const float* w, const float* bias, float* y, int B, int Nmax, int Cin,
                      int taps, float in_slope, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TTTS_HIP_H */
