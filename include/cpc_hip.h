/* cpc_hip.h -- C ABI of libcpc_hip.so, the MI355X (gfx950) implementation of the
 * CPC-audio train-step hot path.
 *
 * The reference (facebookresearch/CPC_audio) has no FFI: its hot path is a set of
 * torch.nn.Module classes.  This ABI is what those modules' forward/backward bind to
 * in the drop-in package (cpc_audio_amd/model.py, criterion.py via ctypes); each entry
 * point cites the reference code it replaces.  INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 (or int32 where stated), owned by the
 *     caller (torch's caching allocator); nothing is allocated or retained here;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no syncs;
 *   - activations are channels-last: (B, L, C) with C = 256 contiguous;
 *   - return value 0 = ok, CPC_ERR_* = argument error, 1000+e = hipError_t e.
 */
#ifndef CPC_HIP_H
#define CPC_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define CPC_OK 0
#define CPC_ERR_SHAPE 1        /* unsupported / inconsistent sizes */
#define CPC_ERR_ARG 2          /* null pointer or bad flag */

/* ABI version, bumped on any signature change. */
int cpc_abi_version(void);
/* The two-stream entry points (*_streams) keep a small pool of hipEvents per (device, caller stream), created on first use and
 * reused for the life of the process -- right for long-lived streams.  A caller that creates and destroys streams hands each
 * one back before destroying it (no *_streams call of this library may be in flight on it). */
int cpc_release_stream(void* stream);
/* *overlap = 1 if a kernel on stream_b completes while stream_a is busy, 0 if the two execute in submission order: the runtime
 * maps hipStreams onto a few hardware queues (4 per priority level) in creation order, and two streams on one queue serialise
 * whatever their events allow.  Launches a 3 ms one-wavefront wait kernel on stream_a and blocks the calling thread until both
 * streams drain: a start-up probe, used by the host side to choose the side streams of cpc_train_step. */
int cpc_streams_overlap(void* stream_a, void* stream_b, int* overlap);

/* Arithmetic of the NT GEMMs (conv forward/dgrad, projections, heads):
 *   1 bf16 matrix pipe, fp32 operands split by truncation into three bf16 pieces, six
 *     bf16 MFMAs per product, fp32 accumulate: error <= 2^-23 per product (fp32 level), 2.67x the rate;
 *   0 exact-f32 MFMA (v_mfma_f32_32x32x2_f32);
 *   2 fp16 matrix pipe for the 128-row conv tiles, operands scaled by a power of two (from a bound on their max|.|) and split into two
 *     fp16 pieces, three fp16 MFMAs per product (hh + hl + lh), fp32 accumulate: error <= 2^-21 per product,
 *     half the MFMAs of mode 1.  Applies to the conv layers (forward, dgrad, wgrad), whose operand bounds
 *     come for free (ChannelNorm affine; max|gradient| accumulated by the producing kernel); the small generic
 *     GEMMs (projections, heads, weight gradients of the AR / criterion) run as in mode 1 unless their operand bounds are
 *     known (cpc_set_gemm_split);
 *   3 (default) as 2, and the encoder (cpc_encoder_forward / _backward) keeps the output of layer 0 -- at B >= ~100 also
 *     of layer 1 -- in H2 storage (below): conv1 (conv2), 70 % (87 %) of the conv stack's FLOPs, read both GEMM operands
 *     global -> LDS by DMA (csrc/conv_dma.hip, 256- / 128-row tiles); their weight gradients read the pieces as stored.  The
 *     per-layer entry points (cpc_conv_layer_*, cpc_conv_gemm_forward, cpc_norm_backward) behave as in mode 2. */
int cpc_set_mfma_mode(int mode);
int cpc_get_mfma_mode(void);

/* Device-side error flags of the current device, accumulated since they were last cleared (clear != 0 clears them):
 *   CPC_DEVERR_GRU_POLL_TIMEOUT  a workgroup of the persistent recurrence (cpc_gru_forward / _backward) gave up
 *                                waiting for another one; its outputs carry NaN from that step on
 *   CPC_DEVERR_NEGATIVE_INDEX    cpc_nce_prepare was handed a draw outside batchIdx in [0,B) / seqIdx in [0,S)
 *                                (criterion.py:181-189 draws [0,B) and [1,S)); the index was clamped
 *   CPC_DEVERR_CONV_EXCHANGE     a workgroup of the N-split conv forward (cpc_set_fwd_nsplit) gave up waiting for its partner's
 *                                ChannelNorm statistics; its rows carry NaN
 *   CPC_DEVERR_LSTM_POLL_TIMEOUT a workgroup of the persistent LSTM recurrence (cpc_lstm_forward / _backward) gave up
 *                                waiting for another one; its outputs carry NaN from that step on
 *   CPC_DEVERR_LABEL_RANGE       a supervised criterion (cpc_classifier_forward, cpc_ctc_forward) met a label outside [0, C)
 *                                (CTC: [0, C-1)); it was clamped for addressing and the loss is NaN.  cpc_ctc_seq_forward: a
 *                                target outside [0, C) or equal to the blank; that sequence's loss is NaN
 *   CPC_DEVERR_ABX_INDEX         an ABX entry point (cpc_abx_*) met a segment id outside [0, n_seg), a segment outside the frames
 *                                or a size outside [1, S]; it was clamped for addressing and that group's score (pair's distance) is NaN
 *   CPC_DEVERR_DECODE_RANGE      a PER entry point (cpc_ctc_beam_search, cpc_nw_align_score) met a sequence length outside
 *                                [1, T_max] (alignment: [0, L]) or a blank outside [0, P); that sequence's score is NaN
 *   CPC_DEVERR_LENGTH_RANGE      cpc_ctc_seq_forward met an input length outside [0, T] or a target length outside [0, Lmax],
 *                                or cpc_seqnorm_forward / _backward a length outside [0, S];
 *                                it was clamped for addressing and that sequence's loss is NaN
 * The reference raises Python exceptions for such things; kernels cannot, so the wrapper (ops.check_device_errors) turns
 * the mask into a RuntimeError.  The call synchronises with the device: logging points and tests, not the step path.
 * Returns the mask (>= 0) or a negative number if the flags cannot be read. */
#define CPC_DEVERR_GRU_POLL_TIMEOUT 1
#define CPC_DEVERR_NEGATIVE_INDEX 2
#define CPC_DEVERR_CONV_EXCHANGE 4
#define CPC_DEVERR_LSTM_POLL_TIMEOUT 8
#define CPC_DEVERR_LABEL_RANGE 16
#define CPC_DEVERR_ABX_INDEX 32
#define CPC_DEVERR_DECODE_RANGE 64
#define CPC_DEVERR_LENGTH_RANGE 128
/*   CPC_DEVERR_RNN_POLL_TIMEOUT  a workgroup of a persistent Elman recurrence (cpc_rnn_forward / _backward) gave up waiting for
 *                                another one; its outputs carry NaN from that step on */
#define CPC_DEVERR_RNN_POLL_TIMEOUT 256
int cpc_device_error_flags(int clear);

/* ---------------------------------------------------------------- encoder ----
 * CPCEncoder.forward, cpc/model.py:99-105:  5 x relu(ChannelNorm(conv_i(x))).
 * ChannelNorm: cpc/model.py:50-58 (mean / UNBIASED variance over channels, eps 1e-5).
 */

/* Layer 0 (conv0 1->256 k10 s5 p3, model.py:83,100) fused with norm + ReLU.
 * wave (B,L); w (256,1,10); bias,nw,nb (256); y (B,L0,256); mean,rstd (B*L0). */
int cpc_conv0_forward(const float* wave, const float* w, const float* bias, const float* nw,
                      const float* nb, float* y, float* mean, float* rstd, int B, int L,
                      void* stream);
/* "H2" activation storage (csrc/cpc_common.h): an fp32 tensor of 256-channel rows kept as two fp16 pieces per element,
 * x * s = h + l with s = the power of two that maps a bound *amax >= max|x| into fp16's range -- exactly the two operand
 * pieces of the 3-product fp16 GEMM tiles -- laid out per 8 channels as [h x 8 | l x 8] (32 bytes; 1 KB per row, as fp32).
 * In mode 3 (cpc_set_mfma_mode) the encoder keeps the outputs of layers 0 and 1 in this form: conv1 / conv2 then read both
 * GEMM operands global -> LDS by DMA.  The entry points below expose the pieces (tests, benchmarks, other callers). */
/* conv0 writing y in H2 storage scaled by scale(*y_amax) (y_amax == NULL: plain fp32, = cpc_conv0_forward) */
int cpc_conv0_forward_h2(const float* wave, const float* w, const float* bias, const float* nw, const float* nb,
                         void* y, float* mean, float* rstd, const float* y_amax, int B, int L, void* stream);
/* fp32 (n_rows,256) <-> H2 with the scale of *amax */
int cpc_h2_encode(const float* src, void* dst, long n_rows, const float* amax, void* stream);
int cpc_h2_decode(const void* src, float* dst, long n_rows, const float* amax, void* stream);
/* conv weight (256,256,k) -> the DMA kernel's K-tile-major H2 rows; wq: 256*k*256 + 64 floats (max|w| behind the tiles) */
int cpc_conv_weight_relayout_h2(const float* w, float* wq, int k, void* stream);
/* One conv layer (k = 2s) + bias + ChannelNorm + ReLU on the DMA kernel (conv_dma.hip, one launch): x in H2 storage scaled
 * by scale(*x_amax); y in H2 storage scaled by scale(*y_amax) (which must bound |y|), or fp32 when y_amax == NULL; xhat,
 * rstd fp32.  zeros: 32 floats of zeros (padding rows).  bm: rows per workgroup, 128 / 256 (0: by problem size). */
int cpc_conv_gemm_forward_h2(const void* x_h2, const float* wq, const float* bias, const float* nw, const float* nb,
                             void* y, float* xhat, float* rstd, const float* x_amax, const float* y_amax,
                             const float* zeros, int B, int Lin, int k, int s, int p, int bm, void* stream);
/* tuning knobs of the DMA kernel inside the composite encoder: rows per workgroup (0 / 128 / 256) and the K-walk
 * rotation step between neighbouring workgroups (0: lockstep) */
int cpc_set_conv0_tuning(int groups, int nontemporal);   /* layer-0 forward kernel: 16-step groups per wave (1..8, default 4); 1 / 0 (default):
                                                          * activation rows as non-temporal / plain stores */
int cpc_set_dma_tile(int bm);
int cpc_set_h2_layers(int n);            /* mode 3, which layers read their input (and write their gradient) in H2 storage: 1 = conv1, 2 = conv1 and
                                            conv2, both on the DMA kernels; 4 = all four -- conv1 (conv2 from B ~ 100 on) on the DMA kernels, the
                                            short layers on the register-staged tiles, which stage H2 rows as they lie, and every weight
                                            gradient on the DMA + transposing-read kernel with one batched reduction; 0 = by problem size */
int cpc_set_dma_layer2(int on);          /* 1: layer 2 (forward and data gradient) on the DMA-fed kernels whatever the batch size; 0 (default): from B ~ 100 on */
int cpc_set_conv_small_tile(int bm);     /* rows per workgroup of the register-staged conv tiles below 32000 rows: 32 (default) or 64 */
int cpc_set_dgrad_nsplit(int min_wgs);    /* > 0: the H2-fed data gradient of layers below the 128-row regime runs on 128 x 128 tiles (two workgroups
                                            per row tile, 128 input channels each) where that still gives min_wgs workgroups; 0: 32-row tiles */
int cpc_set_conv_small_pipe(int on);     /* 1 (default): the 32- / 64-row tiles of the H2-fed register-staged conv kernels (cpc_set_h2_layers(4)) run the software-
                                            pipelined 16-k schedule of the 128-row tiles (four chunks of global loads in flight); 0: one 32-k stage */
int cpc_set_wgrad_dma_groups(int wgs);  /* workgroups the DMA weight gradient aims at (row splits = wgs / taps); 64..512 */
int cpc_set_wgrad_dma_stages(int n);     /* its LDS pipeline: 2 stages of 32 contraction rows (one in flight) or 4 (default) of 16 (three in flight) */
int cpc_set_wgrad_dma_min_rows(int rows); /* ... and the fewest rows one of its splits walks (default 512; 128..8192, a multiple of 64) */
int cpc_set_wgrad1_early(int on);        /* two-stream encoder backward: 0 (default) layer 1's weight gradient behind its data gradient, 1 beside it */
int cpc_set_h2_dx(int on);               /* mode 3: 1 (default) keeps the gradient dx of every layer whose input is in H2 storage in H2 storage
                                            too (layer 1; layer 2 where conv2 reads H2 input): data gradient on the DMA kernel, weight
                                            gradient on DMA + transposing LDS reads; 2: the same with the weight gradient on the
                                            register-staged tile (A/B); 0: fp32 dx */
int cpc_set_gemm_split(int on);          /* 1 (default): plain GEMMs with known operand bounds (the criterion's, see cpc_nce_forward) run on two
                                            fp16 pieces in mode >= 2, wide products on the 128 x 256 pipelined tile; 0: three bf16 pieces always;
                                            2: two pieces but never the wide tile; 3: the wide tile whatever the grid size (tests) */
int cpc_set_gemm_fuse(int on);           /* 1 (default): the transformer layer's feed-forward ReLU (forward, dropout 0) and ReLU derivative
                                            (backward) as epilogues of their GEMMs on the wide fp16-piece tile; 0: elementwise kernels
                                            behind the GEMMs (same bits) */
int cpc_set_dma_rotation(int step);
int cpc_set_dma_pipeline(int variant);   /* main-loop schedule of the forward DMA kernel on 256-row tiles (tuning / measurement switch; results
                                          * agree to rounding order).  2 (default): tap-pair walk -- an input row reaches LDS once for both
                                          * taps that read it -- where k == 2*stride and Lout % 256 == 0, variant 1 elsewhere; 1: two 32-k
                                          * LDS stages; 0: four 16-k stages, three in flight; 3, 4, 5: ping-pong slots (one wave of a SIMD
                                          * multiplies while its partner loads) with 0 / 2 / 4 DMA pieces issued among the MFMAs; 6: skewed
                                          * slots.  What each measured: DESIGN.md section 4.10 */
long cpc_conv0_backward_scratch_floats(int B, int L);
/* Backward of layer 0 (no dgrad: the waveform needs no gradient, train.py:81-87).
 * dy = gradient w.r.t. y.  Outputs dW0 (256,1,10), dB0, dNW0, dNB0 (256) are overwritten. */
int cpc_conv0_backward(const float* wave, const float* w, const float* bias, const float* nw,
                       const float* nb, const float* mean, const float* rstd, const float* dy,
                       float* scratch, float* dW0, float* dB0, float* dNW0, float* dNB0, int B,
                       int L, void* stream);

/* Layers 1..4 (256->256, k = 2s; model.py:85-92,101-104): x (B,Lin,256) ->
 * y = relu(norm(conv)) and xhat (pre-affine normalised), both (B,Lout,256); rstd (B*Lout).
 * w is PyTorch (O,I,W); wp is 256*k*256*3/2 floats of scratch (re-laid-out weight, see below). */
int cpc_conv_layer_forward(const float* x, const float* w, const float* bias, const float* nw,
                           const float* nb, float* wp, float* y, float* xhat, float* rstd, int B,
                           int Lin, int k, int s, int p, void* stream);
/* Weight re-layout (O,I,W) -> K-major rows wp[co][kk*256+ci]; three bf16 planes in the default
 * split-bf16 mode.  wp: 256*k*256*3/2 floats. */
int cpc_conv_weight_relayout(const float* w, float* wp, int k, void* stream);
/* The forward GEMM kernel alone on a weight prepared by cpc_conv_weight_relayout (one launch). */
/* x_amax: device float holding an upper bound of max|x| (cpc_absmax, or the bound of the producing ChannelNorm);
 * read in mode 2 only, may be NULL otherwise. */
int cpc_conv_gemm_forward(const float* x, const float* wp, const float* bias, const float* nw,
                          const float* nb, float* y, float* xhat, float* rstd, const float* x_amax, int B,
                          int Lin, int k, int s, int p, void* stream);
/* *out = max(*out, max_i |x_i|), exact and order-independent (*out must be initialised, e.g. 0). */
int cpc_absmax(const float* x, long n, float* out, void* stream);
/* ReLU' + ChannelNorm backward over M rows; small3 = [d norm.w | d norm.b | d conv.bias]. */
/* dx_amax (may be NULL): device float that receives max(*dx_amax, max|dx|) (initialise to 0); it is the operand
 * bound the mode-2 dgrad / wgrad of this layer read. */
int cpc_norm_backward(const float* dy, const float* xhat, const float* y, const float* rstd,
                      const float* nw, float* dx, float* colpart, float* tmp, float* small3,
                      float* dx_amax, int M, void* stream);
/* wd: 256*k*256*3/2 floats of scratch (per-phase re-laid-out weight). */
/* dx_amax: device float bounding max|dx| (mode 2; NULL = computed with an extra pass over dx);
 * dprev_amax (fuse only, may be NULL): receives max(*dprev_amax, max|dprev|). */
int cpc_conv_layer_dgrad(const float* dx, const float* w, float* wd, int fuse,
                         const float* xhat_prev, const float* y_prev, const float* rstd_prev,
                         const float* nw_prev, float* dprev, float* colpart, float* tmp,
                         float* small3, const float* dx_amax, float* dprev_amax, int B, int Lin, int k,
                         int s, int p, void* stream);
/* dx_amax, x_amax: device floats bounding max|dx| and max|x| (read in mode 2 only). */
int cpc_conv_layer_wgrad(const float* dx, const float* x, float* part, float* dW, const float* dx_amax,
                         const float* x_amax, int B, int Lin, int k, int s, int p, int splits,
                         int rows_per_split, void* stream);

/* 0: one launch per time step; 1: the two-layer recurrence runs as one persistent launch whenever all of its
 * workgroups can be resident at once (gru.hip) -- bit-identical with 0; 2 (default): as 1, with the forward's
 * recurrent products on the fp16 matrix pipe (operands split into two fp16 pieces, three MFMAs per product, fp32
 * accumulate: differences at the 1e-7 level; exact-f32 products whenever the caller supplies h0). */
int cpc_set_gru_mode(int mode);
/* Persistent recurrence: 1 places the 32 workgroups of each 16-sequence batch tile on one XCD (grid of 256 * ceil(tiles / 8)
 * workgroups, workgroup b on XCD b % 8), so that the step-to-step hand-over stays inside one L2; 0 (default, measured
 * faster) interleaves the tiles over the XCDs (grid of 32 * tiles); 2 forces the packed numbering whatever the device
 * reports (tests). */
int cpc_set_gru_xcd_pack(int on);
/* Hand-over of the persistent recurrence through one XCD's L2 (gru.hip): bit 0 the forward with one batch tile (32 workgroups) per
 * XCD, bit 1 the backward with one (tile, layer) group of 16 workgroups per half XCD, each checked for its placement at the
 * start of the launch, in launches with one batch tile per workgroup; bits 2 / 3 the same in any launch.  Default 3. */
int cpc_set_gru_xcd_local(int mask);
int cpc_set_gru_poll_plain(int mask);   /* first looks of the persistent recurrence through the XCD's L2 (gru.hip); default 15 */
/* Persistent recurrence: cap on the 16-sequence batch tiles of one launch (0 = whatever fits the device, the default); a
 * larger batch runs as several launches one after the other (B = 256 on 256 CUs: two launches of 8 tiles). */
int cpc_set_gru_chunk_tiles(int tiles);
/* Batch tiles a workgroup of the persistent recurrence may own: 2 (default) = a batch that does not fit the device in one launch
 * (B = 256 per GPU, BASELINE configs[2], on 256 CUs) runs as ONE launch, each workgroup interleaving its two tiles step by step
 * (cpc/model.py:193's nn.GRU over the whole batch); 1 = serial launches over chunks of tiles.  Same bits either way. */
int cpc_set_gru_tiles_per_wg(int n);
/* Persistent recurrence: the wait before a step's first look at the hand-over buffers (forward / backward kernel), in
 * units of 64 clocks; < 0 (default): every wave steers its own so that looks that cannot succeed yet are not issued
 * (they load the L2s the hand-over itself goes through). */
int cpc_set_gru_poll_pacing(int first_fwd, int first_bwd);
/* Polling budget of one wave of the persistent recurrence (re-reads over the whole launch) before it gives up and
 * flags CPC_DEVERR_GRU_POLL_TIMEOUT; limit < 0 restores the default (2^20).  Tests use 0 to drive the error path. */
int cpc_set_gru_spin_limit(int limit);

/* Tuning / test knob: rows per block of the conv GEMM tiles (0 = auto, 32, 64, 128). */
int cpc_set_conv_tile(int bm);

/* Whole encoder.  params / grads: 20 pointers in the reference's state-dict order
 * (conv{i}.weight, conv{i}.bias, batchNorm{i}.weight, batchNorm{i}.bias, i = 0..4).
 * cpc_encoder_layout fills sizes[0..21]: [0] saved floats, [1] fwd scratch floats,
 * [2] bwd scratch floats, [3..7] L0..L4, then offsets into `saved` (see enc_conv.hip). */
int cpc_encoder_layout(int B, int L, long* sizes);
/* fp32 copy of the saved output of layer `layer` (0..3) of a cpc_encoder_forward, whatever its storage: dst (B,L_layer,256).
 * Tests / debugging; call it in the mode the forward ran in. */
int cpc_encoder_saved_activation(const float* saved, int layer, float* dst, int B, int L, void* stream);
/* Offsets (in floats, into the backward scratch) of the tensors that survive a cpc_encoder_backward: offs[0..3] = dx1..dx4, the
 * gradients w.r.t. the conv outputs of layers 1..4 (B,L_i,256), offs[4] = dy0, the gradient w.r.t. layer 0's output (B,L0,256);
 * stored as the mode says (mode 4: bf16 elements).  Tests / debugging; call it in the mode the backward ran in. */
int cpc_encoder_backward_offsets(int B, int L, long* offs);
/* Tests / debugging, mode 4 only: the data gradients of layers 2..4 share one temporary, which the next layer's overwrites.  With a
 * device buffer set here, cpc_encoder_backward copies each out before its norm backward reads it: dy1, dy2, dy3 (the gradients
 * w.r.t. y1, y2, y3; bf16 (B,L_i,256)) back to back, B*(L1+L2+L3)*256 bf16 elements.  NULL (default): no copies.  Process-wide. */
int cpc_encoder_keep_data_gradients(void* buf);
int cpc_encoder_forward(const float* wave, const float* const* params, float* saved,
                        float* scratch, float* z, int B, int L, void* stream);
/* The weight-only preparation cpc_encoder_forward starts with (GEMM layouts and max|w| of conv1..4, bounds of the layers'
 * inputs from the ChannelNorm affines; what cpc/model.py:83-92's nn.Conv1d does inside MIOpen, hoisted), alone, for a caller
 * that runs it ahead of the forward: mask bit i (1..4) = layer i, bit 0 = the four bounds.  Used by cpc_train_step_tail. */
int cpc_encoder_prepare_weights(const float* const* params, float* saved, float* scratch, int B, int L, int mask, void* stream);
int cpc_encoder_backward(const float* wave, const float* const* params, const float* saved,
                         const float* z, const float* dz, float* scratch, float* const* grads,
                         int B, int L, void* stream);

/* The same with the four conv weight-gradient GEMMs on `wgrad_stream` (they are not on the dx chain); ordering
 * between the two streams is internal (hip events, no host synchronisation) and `stream` waits for `wgrad_stream`
 * before the call returns control of the outputs.  wgrad_stream == stream: identical to cpc_encoder_backward. */
int cpc_encoder_backward_streams(const float* wave, const float* const* params, const float* saved,
                                 const float* z, const float* dz, float* scratch, float* const* grads, int B,
                                 int L, void* stream, void* wgrad_stream);

/* The encoder at C channels, 2 <= C <= 512 (csrc/enc_wide.hip): params / grads are the 20 pointers in state-dict order at the
 * reference's shapes -- conv0.weight (C,1,10), conv{i}.weight (C,C,k), biases (C,), batchNorm{i}.weight / .bias (1,C,1) -- wave
 * (B,1,L), z and dz (B,L4,C); every gradient is fully overwritten.  cpc_encoder_layout_c fills the same 22 slots as
 * cpc_encoder_layout; inside `saved` the activations have a row pitch of 64 ceil(C / 64) floats with zero pad columns.
 * Exact-f32 MFMAs whatever cpc_set_mfma_mode says; no atomics: two calls give the same bits.  C == 256 forwards to the entry
 * points above (their kernels, layouts and bits).  C < 2 (one channel has no unbiased variance), C > 512 or a shape the index
 * arithmetic does not cover (B (L + 16) >= 2^30, a window shorter than the five convolutions need): CPC_ERR_SHAPE, checked first and
 * before any launch; a NULL pointer or a workspace that is not 16-byte aligned: CPC_ERR_ARG. */
int cpc_encoder_layout_c(int B, int L, int C, long* sizes);
int cpc_encoder_forward_c(const float* wave, const float* const* params, float* saved, float* scratch, float* z,
                          int B, int L, int C, void* stream);
int cpc_encoder_backward_c(const float* wave, const float* const* params, const float* saved, const float* z,
                           const float* dz, float* scratch, float* const* grads, int B, int L, int C, void* stream);
/* dst (B,L_layer,C), the true width: the saved output of layer `layer` (0..3) of a cpc_encoder_forward_c.  Tests / debugging. */
int cpc_encoder_saved_activation_c(const float* saved, int layer, float* dst, int B, int L, int C, void* stream);

/* The encoder at C channels under any of the reference's normModes (csrc/enc_wide.hip).  norm: 0 layerNorm (forwards
 * to the _c entries above: their kernels, launches and bits), 1 batchNorm (nn.BatchNorm1d), 2 instanceNorm (nn.InstanceNorm1d with
 * affine parameters, the same in train and eval), 3 ID (relu(conv + bias)); any other value: CPC_ERR_ARG.  2 <= C <= 512, 256
 * included (the other modes run it on the padded storage).  params / grads keep 20 slots in state-dict order; norm weight and
 * bias are read as C contiguous floats (the (C,) of the torch modules; ChannelNorm's (1,C,1) under layerNorm); under ID the norm
 * slots may be NULL and are not touched.  running: 10 pointers, running_mean and running_var of layers 0..4 in that order --
 * required under batchNorm (CPC_ERR_ARG when NULL), read in eval mode, and in training updated in place once per forward call:
 * mean with `momentum`, var with the unbiased batch variance.  instanceNorm needs L_4 >= 2 and B <= 65535, batchNorm in training B L_4 >= 2:
 * CPC_ERR_SHAPE otherwise, as for a shape the _c entries refuse.  cpc_encoder_layout_n fills 32 slots: under layerNorm the 22 of
 * cpc_encoder_layout_c; otherwise 0..2 the float counts of saved / forward scratch / backward scratch, 3..7 L_0..L_4, 8..11 the
 * offsets of y0..y3 in `saved`, 12..15 xhat1..4, 16..20 mean per layer, 21..25 rstd per layer ((groups, pitch) each; -1 under
 * ID, which keeps y0..y3 only), 26 the row pitch 64 ceil(C / 64), 27 the statistic groups (B under instanceNorm, else 1).
 * `training` must be the same in the three calls.  The statistics use centred partials combined in index order (no atomics, no
 * E[x^2] - E[x]^2): two calls give the same bits.  Every gradient, z and every saved tensor the backward reads are fully overwritten. */
int cpc_encoder_layout_n(int B, int L, int C, int norm, int training, long* sizes);
int cpc_encoder_forward_n(const float* wave, const float* const* params, float* const* running, float* saved, float* scratch,
                          float* z, int B, int L, int C, int norm, int training, float momentum, float eps, void* stream);
int cpc_encoder_backward_n(const float* wave, const float* const* params, const float* saved, const float* z, const float* dz,
                           float* scratch, float* const* grads, int B, int L, int C, int norm, int training, void* stream);
/* dst (B,L_layer,C): the saved output of layer `layer` (0..3) of a cpc_encoder_forward_n.  Tests / debugging. */
int cpc_encoder_saved_activation_n(const float* saved, int layer, float* dst, int B, int L, int C, int norm, void* stream);

/* ------------------------------------------------------------ plain GEMMs ----
 * C[M,N] = A[M,K] . B[N,K]^T + bias[N]   (N % 128 == 0, K % 16 == 0; bias may be NULL).
 * This is torch.nn.Linear's arithmetic (criterion.py:90-91,108; the GRU projections). */
int cpc_gemm_nt(const float* A, int lda, const float* B, int ldb, const float* bias, float* C,
                int ldc, int M, int N, int K, void* stream);
/* C[N1,N2] (+)= A[M,N1]^T . B[M,N2]   (N1, N2 % 128 == 0): every weight gradient. */
long cpc_gemm_tn_scratch_floats(int M, int N1, int N2);
int cpc_gemm_tn(const float* A, int lda, const float* B, int ldb, float* part, float* C, int M,
                int N1, int N2, int accumulate, void* stream);

/* ------------------------------------------------------------ autoregressor ----
 * CPCAR.forward, cpc/model.py:185-204: nn.GRU(256, 256, num_layers=nl, batch_first=True)
 * (model.py:175-176) with optional initial state h0 (the carried `self.hidden`, :193-198).
 * params / grads: weight_ih_l, weight_hh_l, bias_ih_l, bias_hh_l for l = 0..nl-1
 * (torch state-dict order, gate rows r,z,n).  x, y, dy, dx: (B,S,256); h0, hN: (nl,B,256).
 * cpc_gru_layout fills sizes[0..2] = saved / forward-scratch / backward-scratch floats. */
int cpc_gru_layout(int B, int S, int nl, long* sizes);
int cpc_gru_forward(const float* x, const float* h0, const float* const* params, float* saved,
                    float* scratch, float* y, float* hN, int B, int S, int nl, void* stream);
int cpc_gru_backward(const float* x, const float* h0, const float* const* params,
                     const float* saved, const float* y, const float* dy, float* scratch, float* dx,
                     float* const* grads, int B, int S, int nl, void* stream);

/* The part of the two-layer backward that depends on the forward pass only (per-step gate-derivative coefficients
 * and the pre-filled hand-over buffers of the persistent launch: cpc_gru_coef_floats(B,S,nl) floats; 0 unless
 * nl == 2; one buffer serves one backward call).  cpc_gru_backward_coef may run any time after the forward
 * on any stream; cpc_gru_backward_with_coef(coef != NULL) then skips that work (coef == NULL: same as
 * cpc_gru_backward). */
long cpc_gru_coef_floats(int B, int S, int nl);
int cpc_gru_backward_coef(const float* h0, const float* const* params, const float* saved, const float* y, float* coef,
                          int coef_done, int B, int S, int nl, void* stream);
/* cpc_gru_forward that also fills the coefficient arrays of `coef` (cpc_gru_coef_floats floats) on the way: the persistent
 * forward's gate threads hold every input of those coefficients in registers.  Follow with cpc_gru_backward_coef(coef_done = 1),
 * which then only prepares the hand-over buffers and the transposed weights. */
int cpc_gru_forward_coef(const float* x, const float* h0, const float* const* params, float* saved, float* scratch, float* y,
                         float* hN, float* coef, int B, int S, int nl, void* stream);
int cpc_gru_backward_with_coef(const float* x, const float* h0, const float* const* params, const float* saved,
                               const float* y, const float* dy, const float* coef, float* scratch, float* dx,
                               float* const* grads, int B, int S, int nl, void* stream);

/* cpc_gru_forward_coef split for callers that keep launches off their critical stream: cpc_gru_forward_prepare fills the
 * persistent recurrence's hand-over buffers in `scratch` (the forward's only activation-independent launch) on any stream;
 * cpc_gru_forward_coef_prepared, on a stream that has waited for it, skips that fill.  nl == 2. */
int cpc_gru_forward_prepare(float* scratch, int B, int S, int nl, void* stream);
int cpc_gru_forward_coef_prepared(const float* x, const float* h0, const float* const* params, float* saved, float* scratch,
                                  float* y, float* hN, float* coef, int B, int S, int nl, void* stream);

/* As cpc_gru_backward_with_coef, with the weight and bias gradients (what only the optimiser reads) on
 * `wgrad_stream`, released by an event behind the recurrence; dx stays on `stream`.  There is NO join: the caller
 * orders every consumer of `grads` after `wgrad_stream` and keeps `scratch` alive until then.  (nl == 2; other depths
 * run on `stream` alone.) */
int cpc_gru_backward_streams(const float* x, const float* h0, const float* const* params, const float* saved,
                             const float* y, const float* dy, const float* coef, float* scratch, float* dx,
                             float* const* grads, int B, int S, int nl, void* stream, void* wgrad_stream);

/* The two-layer recurrence over the first T of S steps (1 <= T <= S, else CPC_ERR_ARG; nl == 2): for a loss that reads y[:, :T] only.
 * S stays the stride of every tensor and the M of every GEMM; T only bounds the time loops, each of which costs a hand-over
 * round trip between workgroups.  T == S is exactly the entry without the suffix.
 *   cpc_gru_forward_prepare_steps: cpc_gru_forward_prepare, plus zeros in rows t >= T of y and of layer 0's output in `saved`
 *     (what the shortened forward leaves unwritten and the backward's GEMMs read over all S steps); any stream.
 *   cpc_gru_forward_coef_prepared_steps: runs steps t < T; y[:, :T], the saved values and the coefficients of those steps are the
 *     full run's bits.  hN is written only when T == S.  Only a backward with the same T (or a smaller one) may follow.
 *   cpc_gru_backward_streams_steps: the caller promises dy[:, T:] == 0.  Starts at t = T - 1 with an incoming dh of zero -- what
 *     the full run has there -- and writes the gate gradients of the steps behind as zeros: dx (dx[:, T:] == 0) and the eight
 *     gradients equal cpc_gru_backward_streams' on the same inputs. */
int cpc_gru_forward_prepare_steps(float* scratch, float* saved, float* y, int B, int S, int T, int nl, void* stream);
int cpc_gru_forward_coef_prepared_steps(const float* x, const float* h0, const float* const* params, float* saved, float* scratch,
                                        float* y, float* hN, float* coef, int B, int S, int T, int nl, void* stream);
int cpc_gru_backward_streams_steps(const float* x, const float* h0, const float* const* params, const float* saved,
                                   const float* y, const float* dy, const float* coef, float* scratch, float* dx,
                                   float* const* grads, int B, int S, int T, int nl, void* stream, void* wgrad_stream);

/* ------------------------------------------------------------ LSTM autoregressor ----
 * CPCAR with mode "LSTM" (cpc/model.py:167-169, the reference's default --arMode): nn.LSTM(256, 256, num_layers=nl,
 * batch_first=True), 1 <= nl <= 8, fp32, optional carried state (h0, c0) -- both or neither.
 * params / grads: weight_ih_l (4H,H), weight_hh_l (4H,H), bias_ih_l, bias_hh_l (4H) for l = 0..nl-1 (torch state-dict order,
 * gate rows i,f,g,o); grads are OVERWRITTEN.  x, y, dy, dx: (B,S,256); h0, c0, hN, cN: (nl,B,256).
 * cpc_lstm_layout fills sizes[0..2] = saved / forward-scratch / backward-scratch floats (B * S <= 2^21).
 * The forward writes `saved` (what the backward reads); y and hN / cN are outputs.  The backward differentiates x and the
 * parameters; h0 and c0 receive no gradient (the reference detaches the carried state, cpc/model.py:194-198).
 * flags: CPC_LSTM_PER_STEP runs the per-step kernels (one launch per time step) instead of the persistent recurrence, which is
 * otherwise taken whenever its grid can be resident at once; both give the same bits.  Arguments are checked before any launch. */
#define CPC_LSTM_PER_STEP 1
int cpc_lstm_layout(int B, int S, int nl, long* sizes);
int cpc_lstm_forward(const float* x, const float* h0, const float* c0, const float* const* params, float* saved,
                     float* scratch, float* y, float* hN, float* cN, int B, int S, int nl, int flags, void* stream);
int cpc_lstm_backward(const float* x, const float* h0, const float* c0, const float* const* params, const float* saved,
                      const float* y, const float* dy, float* scratch, float* dx, float* const* grads, int B, int S, int nl,
                      int flags, void* stream);

/* G LSTM heads side by side (the criterion's --rnnMode LSTM: K nn.LSTM(256, 256, batch_first=True) reading the same context,
 * cpc/criterion/criterion.py:66-68): one layer, no carried state, 1 <= G <= 64, B * S * G <= 2^21, fp32.
 * x, dx: (B,S,256), shared by the heads (dx is summed over them); y, dy: (B,S,G*256), head g at columns g*256.. -- the layout the
 * score kernels read.  The heads' parameters one behind the other: w_ih (G*1024,256), w_hh (G,1024,256), b_ih, b_hh (G*1024), gate
 * rows i,f,g,o; the gradients have the same layouts and are OVERWRITTEN.
 * cpc_lstm_group_layout fills sizes[0..2] = saved / forward-scratch / backward-scratch floats.
 * The input projection of all heads is one GEMM; the recurrences of as many whole heads as can be resident together (counted as
 * CUs * max(1, min(occupancy query - 1, 4)) workgroups) share one persistent launch, the launches follow one another; where not
 * even one head fits, and with CPC_LSTM_PER_STEP, one launch per time step runs all heads.  Same bits either way.  A polling
 * time-out raises CPC_DEVERR_LSTM_POLL_TIMEOUT.  Arguments are checked before any launch. */
int cpc_lstm_group_layout(int B, int S, int G, long* sizes);
int cpc_lstm_group_forward(const float* x, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                           float* saved, float* scratch, float* y, int B, int S, int G, int flags, void* stream);
int cpc_lstm_group_backward(const float* x, const float* w_ih, const float* w_hh, const float* saved, const float* y,
                            const float* dy, float* scratch, float* dx, float* dw_ih, float* dw_hh, float* db_ih, float* db_hh,
                            int B, int S, int G, int flags, void* stream);

/* ------------------------------------------------------------ Elman RNN ----
 * torch.nn.RNN(256, 256) with tanh: h_t = tanh(W_ih x_t + b_ih + W_hh h_{t-1} + b_hh), over T time steps of R independent rows,
 * G heads side by side and nl stacked layers, fp32; T * R * G <= 2^21, 1 <= G <= 64, 1 <= nl <= 8, and G > 1 only with nl == 1
 * and without h0 / hN (CPC_ERR_SHAPE / CPC_ERR_ARG otherwise).
 * flags: CPC_RNN_TIME_MAJOR: x, dx are (T,R,256) and y, dy (T,R,G*256) -- the criterion's --rnnMode RNN predictors, whose nn.RNN
 *   is built without batch_first and so walks the batch axis of the (B,W,256) context: T = B, R = W, G = K
 *   (cpc/criterion/criterion.py:62-64); without it they are (R,T,256) / (R,T,G*256) -- CPCAR with mode "RNN"
 *   (cpc/model.py:177-180: nn.RNN(256, 256, nl, batch_first=True)), R = B, T = S, G = 1.
 *   CPC_RNN_PER_STEP: one launch per time step instead of the persistent recurrence (otherwise taken for as many whole heads per
 *   launch as can be resident together, as cpc_lstm_group_forward); same bits.
 * params / grads: for l = 0..nl-1 weight_ih_l (G*256,256), weight_hh_l (G,256,256), bias_ih_l, bias_hh_l (G*256): the heads' tensors
 *   one behind the other; grads are OVERWRITTEN.  h0 (or NULL), hN (or NULL): (nl,R,256); h0 receives no gradient.
 * cpc_rnn_layout fills sizes[0..2] = saved / forward-scratch / backward-scratch floats.  The backward needs y and `saved` (the
 * lower layers' outputs) only.  A polling time-out raises CPC_DEVERR_RNN_POLL_TIMEOUT.  Arguments are checked before any launch. */
#define CPC_RNN_PER_STEP 1
#define CPC_RNN_TIME_MAJOR 2
int cpc_rnn_layout(int T, int R, int G, int nl, long* sizes);
int cpc_rnn_forward(const float* x, const float* h0, const float* const* params, float* saved, float* scratch, float* y, float* hN,
                    int T, int R, int G, int nl, int flags, void* stream);
int cpc_rnn_backward(const float* x, const float* h0, const float* const* params, const float* saved, const float* y,
                     const float* dy, float* scratch, float* dx, float* const* grads, int T, int R, int G, int nl, int flags,
                     void* stream);

/* ------------------------------------------------------------ autoregressors at any input width ----
 * The three cells above with an encoder width D in 1..512 in front of the 256-wide context (MFCC at 13 / 40 / 80 coefficients,
 * the learned filter bank at 64, CPCEncoder(512) ...): x, dx are (B,S,D) -- for the RNN (R,T,D), or (T,R,D) with CPC_RNN_TIME_MAJOR, one head --
 * and weight_ih_l0 and its gradient (3H | 4H | H, D); everything else is as in cpc_gru_* / cpc_lstm_* / cpc_rnn_* (same
 * params / grads order, saved buffers, flags, carried state, error words).  Only layer 0's input projection and its two backward
 * products depend on D; they run in csrc/in_proj.hip, the recurrences and the layers above are the 256-wide ones.  With D == 256
 * the *_in entries ARE the plain entries: same launches, same bits, same layout sizes.  The GRU takes no prepared coefficients
 * and no second stream here (cpc_gru_forward_coef / cpc_gru_backward_streams stay 256-wide).
 * cpc_*_layout_in fill sizes[0..2] = saved / forward-scratch / backward-scratch floats.  D outside 1..512: CPC_ERR_SHAPE; a NULL
 * pointer: CPC_ERR_ARG; both before any launch. */
int cpc_gru_layout_in(int B, int S, int nl, int D, long* sizes);
int cpc_gru_forward_in(const float* x, const float* h0, const float* const* params, float* saved, float* scratch, float* y,
                       float* hN, int B, int S, int nl, int D, void* stream);
int cpc_gru_backward_in(const float* x, const float* h0, const float* const* params, const float* saved, const float* y,
                        const float* dy, float* scratch, float* dx, float* const* grads, int B, int S, int nl, int D, void* stream);
int cpc_lstm_layout_in(int B, int S, int nl, int D, long* sizes);
int cpc_lstm_forward_in(const float* x, const float* h0, const float* c0, const float* const* params, float* saved, float* scratch,
                        float* y, float* hN, float* cN, int B, int S, int nl, int D, int flags, void* stream);
int cpc_lstm_backward_in(const float* x, const float* h0, const float* c0, const float* const* params, const float* saved,
                         const float* y, const float* dy, float* scratch, float* dx, float* const* grads, int B, int S, int nl,
                         int D, int flags, void* stream);
int cpc_rnn_layout_in(int T, int R, int nl, int D, long* sizes);
int cpc_rnn_forward_in(const float* x, const float* h0, const float* const* params, float* saved, float* scratch, float* y,
                       float* hN, int T, int R, int nl, int D, int flags, void* stream);
int cpc_rnn_backward_in(const float* x, const float* h0, const float* const* params, const float* saved, const float* y,
                        const float* dy, float* scratch, float* dx, float* const* grads, int T, int R, int nl, int D, int flags,
                        void* stream);

/* ------------------------------------------------------------ the LSTM at any hidden width ----
 * torch.nn.LSTM(D, H, nl, batch_first=True) with 1 <= D <= 512 and 1 <= H <= 512: x, dx (B,S,D); y, dy (B,S,H); h0, c0 (both or
 * neither), hN, cN (nl,B,H); params / grads in state-dict order at their TRUE shapes -- weight_ih_l0 (4H,D), weight_ih_l{k>0}
 * (4H,H), weight_hh (4H,H), biases (4H) -- every gradient fully overwritten.  Inside, the recurrence runs at the padded width
 * Hp = 128 ceil(H/128) on zero-padded parameter copies (csrc/lstm.hip; a padded unit stays exactly zero), persistent or, for a
 * grid that cannot be co-resident or with CPC_LSTM_PER_STEP, one launch per step (bit-identical).  `saved` keeps every layer's
 * padded output, so the backward does not read y (it must still be non-NULL).  A polling time-out raises
 * CPC_DEVERR_LSTM_POLL_TIMEOUT.  1 <= nl <= 8, B*S <= 2^21 and B*S*4Hp <= 2^31 (so B*S <= 2^20 above H = 384); anything else:
 * CPC_ERR_SHAPE from all three; a NULL pointer, h0 without c0 or an unknown flag bit: CPC_ERR_ARG; both before any launch.
 * With H == 256 the *_h entries ARE cpc_lstm_*_in: same launches, same bits, same layout sizes. */
int cpc_lstm_layout_h(int B, int S, int nl, int D, int H, long* sizes);
/* Which recurrence kernels the cpc_lstm_forward_h / _backward_h calls of this process (H != 256) have launched since the last
 * cpc_lstm_paths_h(1): bit 0 a persistent launch, bit 1 per-step launches.  Host-side bookkeeping, no device access. */
int cpc_lstm_paths_h(int clear);
int cpc_lstm_forward_h(const float* x, const float* h0, const float* c0, const float* const* params, float* saved, float* scratch,
                       float* y, float* hN, float* cN, int B, int S, int nl, int D, int H, int flags, void* stream);
int cpc_lstm_backward_h(const float* x, const float* h0, const float* c0, const float* const* params, const float* saved,
                        const float* y, const float* dy, float* scratch, float* dx, float* const* grads, int B, int S, int nl,
                        int D, int H, int flags, void* stream);

/* ------------------------------------------------------------ the GRU at any hidden width ----
 * torch.nn.GRU(D, H, nl, batch_first=True) with 1 <= D <= 512, 1 <= H <= 512 and 1 <= nl <= 8: x, dx (B,S,D); y, dy (B,S,H);
 * h0 (or NULL), hN (nl,B,H); params / grads in state-dict order at their TRUE shapes -- weight_ih_l0 (3H,D), weight_ih_l{k>0}
 * (3H,H), weight_hh (3H,H), biases (3H) -- every gradient fully overwritten; the carried state gets no gradient.  Inside, the
 * recurrence runs at the padded width Hp = 128 ceil(H/128) on zero-padded parameter copies (csrc/gru.hip).  A padded unit has
 * r = z = 1/2 and n = 0, so h' = h_prev / 2: it stays exactly zero because the carried h0 is padded with WRITTEN zeros.  One
 * persistent launch per layer and direction or, for a grid that cannot be co-resident or with CPC_GRU_PER_STEP, one launch
 * per step (bit-identical); exact-f32 MFMAs, no atomics on floats.  `saved` keeps every layer's padded output, so the backward
 * does not read y (it must still be non-NULL).  A polling time-out raises CPC_DEVERR_GRU_POLL_TIMEOUT and the budget is
 * cpc_set_gru_spin_limit's.
 * Shapes: the GEMM row maps index B*S rows with 21 bits, and row offsets into the (B,S,3Hp) arrays are 32-bit: B*S <= 2^21 and
 * B*S*3Hp <= 2^31 (the second binds above H = 256: B*S <= 1864135 at Hp = 384, <= 1398101 at Hp = 512).  Anything else:
 * CPC_ERR_SHAPE from all three; a NULL pointer or an unknown flag bit: CPC_ERR_ARG; both before any launch.
 * With H == 256 the *_h entries ARE cpc_gru_*_in: same launches, same bits, same layout sizes; CPC_GRU_PER_STEP is refused there
 * with CPC_ERR_ARG (that path's choice belongs to cpc_set_gru_mode). */
#define CPC_GRU_PER_STEP 1
int cpc_gru_layout_h(int B, int S, int nl, int D, int H, long* sizes);      /* sizes[0..2]: saved / forward / backward scratch */
/* Which recurrence kernels the cpc_gru_forward_h / _backward_h calls of this process (H != 256) have launched since the last
 * cpc_gru_paths_h(1): bit 0 a persistent launch, bit 1 per-step launches.  Host-side bookkeeping, no device access. */
int cpc_gru_paths_h(int clear);
int cpc_gru_forward_h(const float* x, const float* h0, const float* const* params, float* saved, float* scratch, float* y,
                      float* hN, int B, int S, int nl, int D, int H, int flags, void* stream);
int cpc_gru_backward_h(const float* x, const float* h0, const float* const* params, const float* saved, const float* y,
                       const float* dy, float* scratch, float* dx, float* const* grads, int B, int S, int nl, int D, int H,
                       int flags, void* stream);

/* The projection on its own (csrc/in_proj.hip; exact-f32 MFMAs, so nothing is assumed about the size of x):
 *   cpc_in_proj_forward   out[M,N] = x[M,D] . w[N,D]^T + bias            (bias may be NULL)
 *   cpc_in_proj_backward  dx[M,D] = dg[M,N] . w[N,D]   and   dw[N,D] = dg[M,N]^T . x[M,D]   (both OVERWRITTEN; dx or dw may be
 *                         NULL -- that product is skipped -- but not both)
 * 1 <= M <= 2^24, N a multiple of 128 (<= 65536), 1 <= D <= 512 (CPC_ERR_SHAPE otherwise).  Row m of x and of dx starts at
 * + m * ldx floats, ldx >= D, at any 4-byte alignment: nothing is read or written outside the D columns of the M rows.  w is
 * contiguous; out, dg (N floats per row) and scratch must be 16-byte aligned (CPC_ERR_ARG otherwise, as for a NULL pointer).
 * scratch: cpc_in_proj_scratch_floats(M, N, D) floats (0 for a shape outside the limits) -- a zero-padded copy of w and the row
 * splits of dw, which are summed in a fixed order: no atomics, the same bits every run. */
long cpc_in_proj_scratch_floats(int M, int N, int D);
int cpc_in_proj_forward(const float* x, long ldx, const float* w, const float* bias, float* scratch, float* out, int M, int N,
                        int D, void* stream);
int cpc_in_proj_backward(const float* x, long ldx, const float* w, const float* dg, float* scratch, float* dx, float* dw, int M,
                         int N, int D, void* stream);

/* ------------------------------------------------------------ supervised criteria ----
 * SpeakerCriterion / PhoneCriterion (cpc/criterion/criterion.py:182-246): nn.Linear(256, C) + nn.CrossEntropyLoss() (mean)
 * and (argmax == label).double().mean(); CTCPhoneCriterion (criterion.py:249-283): the same linear layer, log_softmax and
 * nn.CTCLoss(blank = C-1, zero_infinity = True, reduction mean) with every input length S and the frame labels collapsed
 * on the device (collapseLabelChain, cpc/criterion/seq_alignment.py:64-86: no host round trip) into the targets of the loss
 * that cpc_ctc_seq_forward / _backward run as well.  fp32, 2 <= C <= 8192.
 * cpc_supervised_layout(B, S, C, ctc, sizes): R = B * S rows (the speaker criterion: B rows, S = 1), R * C < 2^31, CTC with
 *   1 <= S <= 512.  sizes[0] = saved floats (what the forward writes for the backward: the R * C logits first; then per-row
 *   log-sum-exp, loss and hit, or with ctc the collapsed int64 targets, their lengths and what the CTC loss saves),
 *   sizes[1] = scratch floats of cpc_classifier_backward (dlogits and per-slab dW / db partials), sizes[2] = dlogits floats of
 *   cpc_ctc_backward (R * C; 0 without ctc).
 * x: R rows of 256 floats, row r at x + r * ldx (ldx >= 256: cFeature[:, -1, :] read in place); W (C,256), b (C);
 * labels: int64, (R) / (B,S).  A label out of range is clamped for addressing, raises CPC_DEVERR_LABEL_RANGE and makes the
 * loss NaN.  loss: one float; acc: one double.  Arguments are checked before any launch; nothing is allocated and nothing
 * waits for the device.
 * cpc_classifier_backward: dW, db overwritten; dX (R,256 dense) only when non-NULL.  dlogits NULL: g (softmax - onehot) / R
 * from the saved forward (labels, saved and dloss -- one device float, the loss's gradient -- required); non-NULL: the
 * caller's (R,C) dlogits (the CTC path; labels, saved and dloss ignored).  dW / db are summed over row slabs in a fixed order
 * (no float atomics: the same bits on every run).
 * cpc_ctc_backward: dlogits (B*S, C) of the loss w.r.t. the logits, scaled by *dloss (zero for a sequence whose loss was
 * infinite); W, b and x then receive their gradients through cpc_classifier_backward(dlogits = ...). */
int cpc_supervised_layout(int B, int S, int C, int ctc, long* sizes);
int cpc_classifier_forward(const float* x, long ldx, const float* W, const float* b, const long long* labels, float* saved,
                           float* loss, double* acc, int R, int C, void* stream);
int cpc_classifier_backward(const float* x, long ldx, const float* W, const long long* labels, const float* saved,
                            const float* dloss, const float* dlogits, float* scratch, float* dW, float* db, float* dX, int R,
                            int C, void* stream);
int cpc_ctc_forward(const float* x, const float* W, const float* b, const long long* labels, float* saved, float* loss, int B,
                    int S, int C, void* stream);
int cpc_ctc_backward(const float* saved, const float* dloss, float* dlogits, int B, int S, int C, void* stream);
/* The same criteria on D features per row, 1 <= D <= 512 (CPC_ERR_SHAPE beyond; checked first): x rows of D floats at
 * x + r * ldx (ldx >= D, else CPC_ERR_ARG; the CTC call: dense), W (C,D), dW (C,D) and dX (R,D) dense at pitch D; everything else
 * as above.  The same host code and kernels as the 256 entry points, which pass 256: D = 256 gives their bits.
 * cpc_ctc_backward serves every width: the logits and the loss's block lie in ``saved`` where they do at 256. */
int cpc_supervised_layout_d(int B, int S, int C, int D, int ctc, long* sizes);
int cpc_classifier_forward_d(const float* x, long ldx, const float* W, const float* b, const long long* labels, float* saved,
                             float* loss, double* acc, int R, int C, int D, void* stream);
int cpc_classifier_backward_d(const float* x, long ldx, const float* W, const long long* labels, const float* saved,
                              const float* dloss, const float* dlogits, float* scratch, float* dW, float* db, float* dX, int R,
                              int C, int D, void* stream);
int cpc_ctc_forward_d(const float* x, const float* W, const float* b, const long long* labels, float* saved, float* loss, int B,
                      int S, int C, int D, void* stream);

/* ------------------------------------------------------- PER phone classifier ----
 * CTCphone_criterion of cpc/eval/common_voices_eval.py: nn.Conv1d(256, C, 8, stride 4) on the features, log_softmax and
 * nn.CTCLoss(blank, reduction, zero_infinity = True) with per-utterance input lengths and padded targets (csrc/phone_head.hip).
 * fp32 storage, exact-f32 FMA products, CTC recursions in float64 in log space, no float atomics and fixed summation orders:
 * identical calls give identical bits, and a sequence's results do not depend on the batch around it.  Arguments are checked
 * before any launch; nothing is allocated and nothing waits for the device.
 * cpc_phone_head_layout(B, S, C, Lmax, sizes): B >= 1 utterances of S >= 8 frames, T = (S - 8) / 4 + 1 <= 2048 windows,
 *   2 <= C <= 256 classes, 0 <= Lmax <= 512 target columns, B * T * C < 2^28 (CPC_ERR_SHAPE beyond).  sizes[0] = T,
 *   sizes[1] = floats of wr (C * 2048), sizes[2] = scratch floats of the head's forward and backward, sizes[3] = floats of
 *   logits / dlogits (B * T * C), sizes[4] = saved floats of cpc_ctc_seq_forward.
 * x: (B, S, 256) contiguous, channels-last (cFeature before its permute); W (C, 256, 8) and dW in torch's Conv1d layout; b (C).
 * cpc_phone_head_forward: logits[b, t, o] = b[o] + sum_{j<8} sum_{c<256} x[b, 4t + j, c] W[o, c, j], (B, T, C) dense.  wr receives
 *   the weight in the order of a window's 2048 floats, wr[o][j * 256 + c]: the backward's dX reads it.
 * cpc_phone_head_backward: dlogits (B, T, C) -> dW, db overwritten, summed over row slabs in slab order; dX (B, S, 256) only
 *   when non-NULL, in gather form (each frame sums its at most two windows; frames no window covers get exactly 0).
 * cpc_ctc_seq_forward: logits (B, T, C); in_len (B) int64 in [0, T]; targets int64, row b at targets + b * tgt_stride
 *   (tgt_stride >= Lmax; may be NULL when Lmax = 0); tgt_len (B) int64 in [0, Lmax]; 0 <= blank < C; reduction 0 none (loss: B
 *   floats), 1 mean (the mean over b of loss_b / max(tgt_len_b, 1)), 2 sum.  A sequence whose loss is infinite (its target does
 *   not fit into in_len, in_len = 0 with a target) counts 0; in_len = 0 with an empty target is loss 0.  A target outside
 *   [0, C) or equal to the blank raises CPC_DEVERR_LABEL_RANGE, a length out of range CPC_DEVERR_LENGTH_RANGE; either is clamped
 *   for addressing and makes that sequence's loss NaN.
 * cpc_ctc_seq_backward: dlogits (B, T, C) of the reduced loss, scaled by dloss (one float; B floats for reduction none):
 *   exactly 0 for t >= in_len[b] and for a sequence whose loss was infinite.  Same logits, saved and sizes as the forward. */
int cpc_phone_head_layout(int B, int S, int C, int Lmax, long* sizes);
int cpc_phone_head_forward(const float* x, const float* W, const float* b, float* wr, float* scratch, float* logits, int B,
                           int S, int C, void* stream);
int cpc_phone_head_backward(const float* x, const float* wr, const float* dlogits, float* scratch, float* dW, float* db,
                            float* dX, int B, int S, int C, void* stream);
/* The head at D input features, Conv1d(D, C, 8, stride 4), 1 <= D <= 512 (CPC_ERR_SHAPE beyond; checked first): x (B, S, D),
 * W (C, D, 8), wr[o][j * D + c] (C * 8 * D floats), dX (B, S, D); every other limit, order and guarantee as above, and D = 256
 * gives the bits and the sizes of the calls above.  The CTC calls do not depend on D. */
int cpc_phone_head_layout_d(int B, int S, int C, int Lmax, int D, long* sizes);
int cpc_phone_head_forward_d(const float* x, const float* W, const float* b, float* wr, float* scratch, float* logits, int B,
                             int S, int C, int D, void* stream);
int cpc_phone_head_backward_d(const float* x, const float* wr, const float* dlogits, float* scratch, float* dW, float* db,
                              float* dX, int B, int S, int C, int D, void* stream);
int cpc_ctc_seq_forward(const float* logits, const long long* in_len, const long long* targets, long tgt_stride,
                        const long long* tgt_len, float* saved, float* loss, int B, int T, int C, int Lmax, int blank,
                        int reduction, void* stream);
int cpc_ctc_seq_backward(const float* logits, const float* saved, const float* dloss, float* dlogits, int B, int T, int C,
                         int Lmax, int blank, int reduction, void* stream);

/* ------------------------------------------------------- PER phone classifier: seqNorm and dropout ----
 * What CTCphone_criterion.getPrediction does in front of its head with --seqNorm and --dropout (csrc/seqnorm.hip): per
 * utterance b and channel c, over the n = lengths[b] valid frames,
 *   m = mean_{t<n} x[b,t,c],  v = the unbiased variance over the same frames (two-pass),  r = 1 / sqrt(v + 1e-8)
 *   y[b,t,c] = (x[b,t,c] - m) * r * scale[b,c]   for every t < S (the padding is normalised with the valid frames' statistics)
 * x, y, dy, dx: (B, S, 256) contiguous fp32; lengths: (B) int64 on the device, NULL = every utterance has S frames; scale:
 * (B, 256) or NULL = 1 (nn.Dropout2d's per-(utterance, channel) factor); stats: (B, 2, 256) receives m and r for the backward,
 * NULL when no gradient will be asked for.  normalise = 0: y = x * scale, dx = dy * scale (lengths, stats and the backward's x
 * are not read).  B >= 1, S >= 1, B * S * 256 < 2^31 (CPC_ERR_SHAPE beyond).  y / dx must not alias an input.
 * cpc_seqnorm_backward: g = dy * scale, xh = (x - m) * r, G1 = sum_{t<S} g, G2 = sum_{t<S} g * xh:
 *   dx[b,t,c] = r * (g - [t < n] * (G1 / n + xh * G2 / (n - 1)))
 * One launch per call; exact fp32, no float atomics; the summation order of one (b, c) depends on S and n only, so an utterance
 * gives the same bits alone and inside a batch, on the 16-byte path and on the scalar path (taken when a tensor pointer is not
 * 16-byte aligned).  A length outside [0, S] raises CPC_DEVERR_LENGTH_RANGE and is clamped; n < 2 is no error: that
 * utterance's outputs are NaN, as torch.var's are.  Arguments are checked before any launch; nothing is allocated and
 * nothing waits for the device. */
int cpc_seqnorm_forward(const float* x, const long long* lengths, const float* scale, float* y, float* stats, int B, int S,
                        int normalise, void* stream);
int cpc_seqnorm_backward(const float* x, const float* dy, const long long* lengths, const float* scale, const float* stats,
                         float* dx, int B, int S, int normalise, void* stream);
/* The same on (B, S, D) features, 1 <= D <= 512 (CPC_ERR_SHAPE beyond; checked first), B * S * D < 2^31: x, y, dy, dx dense at
 * row pitch D, scale (B, D), stats (B, 2, D).  The 16-byte path also needs D % 4 == 0.  Channel c of an utterance has the same
 * bits at every D; D = 256 gives the bits of the calls above. */
int cpc_seqnorm_forward_d(const float* x, const long long* lengths, const float* scale, float* y, float* stats, int B, int S,
                          int D, int normalise, void* stream);
int cpc_seqnorm_backward_d(const float* x, const float* dy, const long long* lengths, const float* scale, const float* stats,
                           float* dx, int B, int S, int D, int normalise, void* stream);

/* ------------------------------------------------------- learned-filter-bank encoder (LFBEnconder) ----
 * cpc/model.py:125-152 (csrc/lfb.hip).  x (N, L) mono waveform, W (2D, 400), b (2D), han (400), all fp32 and read only:
 *   y[n,c,t] = b[c] + sum_j W[c,j] x[n,t+j]                  t = 0 .. L-400 (never stored)
 *   e[n,d,t] = y[n,2d,t]^2 + y[n,2d+1,t]^2
 *   s[n,f,d] = sum_{j<400} han[j] e[n,d,160f-350+j]           positions outside [0, L-400] count as zero, F = (L-99)/160 + 1
 * cpc_lfb_energy_forward writes s channels-last (N, F, D) in one launch: the conv is a Toeplitz GEMM on exact-f32 MFMAs whose
 * epilogue squares, pairs and Hann-pools in registers.  cpc_lfb_energy_backward takes gs (N, F, D) and OVERWRITES dW (2D, 400)
 * and db (2D): it recomputes y tile by tile, forms gy = 2 y ge with ge[d,t] = sum_f han[t-160f+350] gs[n,f,d] (at most three
 * terms) and feeds it straight into dW[c,j] = sum_{n,t} gy[n,c,t] x[n,t+j], db[c] = sum gy; per-workgroup partial tiles in
 * ws are summed by one reduce kernel in a fixed order (no float atomics): every result is bit-reproducible.
 * cpc_lfb_layout: sizes[0] = F, sizes[1] / sizes[2] = bytes of ws for the forward (0: ws may be NULL) / the backward; neither
 * grows with N * D * (L - 399).
 * cpc_lfb_lognorm_forward: u = log(1 + |s|); normalise: y = (u - m) / sqrt(v + 1e-5) with m, v the mean and the biased variance
 * (two-pass) of u over the F frames of each (n, d) (nn.InstanceNorm1d without affine parameters or running statistics);
 * stats (N, 2, D) receives m and 1 / sqrt(v + 1e-5), NULL when no gradient will be asked for.  normalise = 0: y = u.
 * cpc_lfb_lognorm_backward: ds from dy, s and stats (not read when normalise = 0).  One launch each; y / ds must not alias an
 * input.
 * CPC_ERR_SHAPE for N < 1, L < 400 (F < 2 for the lognorm calls), D % 32 != 0, D > 512, N * F * D >= 2^31 or
 * N * (L - 399) >= 2^31.  Arguments are checked before any launch; nothing is allocated, copied to the host or waited for. */
int cpc_lfb_layout(int N, int L, int D, long* sizes);
int cpc_lfb_energy_forward(const float* x, const float* W, const float* b, const float* han, float* s, void* ws, int N, int L,
                           int D, void* stream);
int cpc_lfb_energy_backward(const float* x, const float* W, const float* b, const float* han, const float* gs, float* dW,
                            float* db, void* ws, int N, int L, int D, void* stream);
int cpc_lfb_lognorm_forward(const float* s, float* y, float* stats, int N, int F, int D, int normalise, void* stream);
int cpc_lfb_lognorm_backward(const float* s, const float* stats, const float* dy, float* ds, int N, int F, int D, int normalise,
                             void* stream);

/* ------------------------------------------------------- MFCC encoder (MFCCEncoder) ----
 * cpc/model.py:108-122 (csrc/mfcc.hip): torchaudio.transforms.MFCC(n_mfcc = D, melkwargs = {n_mels: M, n_fft: 321}) with
 * M = max(128, D) and torchaudio's documented defaults, restated (not compared with an installed torchaudio).  x (N, L) mono
 * waveform; the three tables are fp32, read only and built by the caller (ops.mfcc_tables):
 *   basis (321, 322)   basis[j][k] = w[j] cos(2 pi j k / 321), basis[j][161 + k] = -w[j] sin(2 pi j k / 321), k = 0 .. 160,
 *                      w the periodic Hann window of 321 points
 *   fb    (161, M)     the HTK mel filter bank over the grid linspace(0, 8000, 161), no area normalisation
 *   dct   (M, D)       dct[m][d] = cos(pi / M (m + 0.5) d) sqrt(2 / M), column 0 times 1 / sqrt(2)
 *   frame f, tap j     xf[j] = x[n, r(160 f - 160 + j)], r reflecting at both ends without repeating the edge sample,
 *                      F = (L - 1) / 160 + 1 frames
 *   p[n,f,k]  = (sum_j xf[j] basis[j][k])^2 + (sum_j xf[j] basis[j][161 + k])^2      (never stored)
 *   db[n,f,m] = 10 log10(max(sum_k fb[k][m] p[n,f,k], 1e-10))
 *   y[n,f,d]  = sum_m dct[m][d] max(db[n,f,m], top - 80),   top = max db over the whole call (rowwise = 1: over row n)
 * cpc_mfcc_meldb writes db channels-last (N, F, M) and one partial maximum per workgroup into ws, in one launch: the three
 * products run on exact-f32 MFMAs, the frames, the spectrum and the power stay in LDS and registers.  cpc_mfcc_dct reduces the
 * partial maxima (a maximum: the same bits in any order, no atomics), clamps and writes y channels-last (N, F, D), one launch.
 * cpc_mfcc_layout: sizes[0] = F, sizes[1] = M, sizes[2] = bytes of ws (N ceil(F / 32) floats).
 * CPC_ERR_SHAPE for N < 1, L < 161 (cpc_mfcc_dct: F < 2), D < 1, D > 512 or N F max(M, D) >= 2^31; CPC_ERR_ARG for a NULL
 * pointer or rowwise outside {0, 1}.  Arguments are checked before any launch; nothing is allocated, copied to the host or
 * waited for. */
int cpc_mfcc_layout(int N, int L, int D, long* sizes);
int cpc_mfcc_meldb(const float* x, const float* basis, const float* fb, float* db, void* ws, int N, int L, int D, void* stream);
int cpc_mfcc_dct(const float* db, const void* ws, const float* dct, float* y, int N, int F, int D, int rowwise, void* stream);

/* ------------------------------------------------------- feed-forward prediction networks ----
 * --rnnMode ffd / conv4 / conv8 / conv12 of cpc/criterion/criterion.py:11-41,69-81 on the equalized layers of
 * custom_layers.py (csrc/pred_conv.hip): G heads of a causal convolution over the time axis, 256 -> 256 channels, ks taps,
 *   y[b, t, g * 256 + o] = act( scale * ( bias[g][o] + sum_{j<ks} sum_{i<256} x_g[b, t - (ks-1) + j, i] * w[g][o][i][j] ) )
 * with frames t' < 0 read as zero, act = ReLU when relu != 0 and the identity otherwise.  scale is the equalized layer's
 * constant sqrt(2 / (256 * ks)), which multiplies the wrapped module's output, bias included.  ShiftedConv is one call
 * (shared = 1, relu = 0); FFNetwork is two with ks = 1: lin1 (shared = 1, relu = 1), then lin2 on lin1's output (shared = 0).
 * x: (B, W, 256), read by every head (shared != 0), or (B, W, G * 256) with head g at columns g * 256 (shared = 0).
 * w (G, 256, 256, ks) and dw: the heads' Conv1d weights one behind the other in torch's layout; bias and db (G, 256);
 * y and dy (B, W, G * 256): the layout cpc_nce_scores_forward reads.  fp32 storage; products at the library's fp32 level, as
 * cpc_gemm_nt's (three bf16 pieces per operand by default, exact-f32 MFMA after cpc_set_mfma_mode(0)); no float atomics
 * and fixed summation orders: identical calls give identical bits, and a batch item's results do not depend on the batch
 * around it.  Arguments are checked before any launch; nothing is allocated and nothing waits for the device.
 * cpc_pred_conv_layout(B, W, G, ks, sizes): 1 <= G <= 64, 1 <= ks <= 16, B, W >= 1, B * W * G * 256 < 2^31 (CPC_ERR_SHAPE
 *   beyond).  sizes[0] = floats of wr (G * ks * 65536), sizes[1] = scratch floats of the backward, sizes[2] = floats of y.
 * cpc_pred_conv_forward: wr receives the weight K-major over a window's floats, wr[g][o][j * 256 + i] (one launch).
 * cpc_pred_conv_backward: dy -> dw, db OVERWRITTEN (row slabs summed in slab order) and, when dx is non-NULL, dx of x's shape:
 *   with a shared input the sum over heads and taps runs inside the call in a fixed order (one accumulator per output, or
 *   up to 8 groups of consecutive heads whose partial sums are added in group order).
 *   relu != 0 masks dy where y <= 0 first (y: the forward's output; not read otherwise and may be NULL). */
int cpc_pred_conv_layout(int B, int W, int G, int ks, long* sizes);
int cpc_pred_conv_forward(const float* x, const float* w, const float* bias, float* wr, float* y, int B, int W, int G, int ks,
                          int shared, float scale, int relu, void* stream);
int cpc_pred_conv_backward(const float* x, const float* w, const float* y, const float* dy, float* scratch, float* dw, float* db,
                           float* dx, int B, int W, int G, int ks, int shared, float scale, int relu, void* stream);

/* ------------------------------------------------------- fused linear-probe step ----
 * The frozen step of cpc/eval/linear_separability.py (train_step :21-47 with feature_maker.optimize == False, val_step :50-68)
 * for SpeakerCriterion / PhoneCriterion: logits = x W^T + b on R rows of 256 features, the mean cross-entropy, the accuracy
 * (argmax == label, the first index on ties), dW and db of the mean loss and torch.optim.Adam's update of W and b, in one call
 * (csrc/probe.hip): cpc_probe_train_step enqueues two kernels for C <= 64 and three beyond, cpc_probe_eval two.  Logits and
 * dlogits stay on the chip; for C > 64 the workspace takes 16 bytes of softmax statistics per row and 64 classes.
 * Exact-f32 FMA products, float64 loss / hit sums, no float atomics and fixed summation orders: identical calls give identical
 * bits.  Nothing is allocated, nothing waits for the device, arguments are checked before any launch.
 * cpc_probe_layout(R, C, sizes): 2 <= C <= 8192, R >= 1, R * C < 2^31 (CPC_ERR_SHAPE beyond).  sizes[0] = workspace floats,
 *   sizes[1] = row slabs (workgroups of the tile kernel), sizes[2] = rows per slab.
 * x: row r at x + r * ldx (ldx >= 256: cFeature[:, -1, :] is read in place); labels: int64 (R).  A label outside [0, C) is clamped
 *   for addressing, raises CPC_DEVERR_LABEL_RANGE and makes that call's loss NaN.
 * workspace: sizes[0] floats, 16-byte aligned; contents are scratch.  loss: one float; acc: one double; accum (or NULL): two
 *   doubles, accum[0] += loss, accum[1] += acc (the epoch's running sums: no host read per step).
 * cpc_probe_train_step: W (C,256), b (C) and their moments exp_avg_* / exp_avg_sq_* are updated in place with the element-wise
 *   arithmetic of cpc_adam_step (same scalars: bias_correction1 = 1 - beta1^step, bias_correction2_sqrt = sqrt(1 - beta2^step));
 *   dW_out (C,256) / db_out (C), when non-NULL, receive the gradients the update was made from.  The loss is that of W, b
 *   BEFORE the update. */
int cpc_probe_layout(int R, int C, long* sizes);
int cpc_probe_train_step(const float* x, long ldx, const long long* labels, int R, int C, float* W, float* b, float* exp_avg_W,
                         float* exp_avg_sq_W, float* exp_avg_b, float* exp_avg_sq_b, double lr, double beta1, double beta2,
                         double eps, double bias_correction1, double bias_correction2_sqrt, float* workspace, float* loss,
                         double* acc, double* accum, float* dW_out, float* db_out, void* stream);
int cpc_probe_eval(const float* x, long ldx, const long long* labels, int R, int C, const float* W, const float* b,
                   float* workspace, float* loss, double* acc, double* accum, void* stream);
/* The same step on D features per row, 1 <= D <= 512 (CPC_ERR_SHAPE beyond; checked first): row r of x at x + r * ldx with
 * ldx >= D (else CPC_ERR_ARG) read in place, W (C,D) dense, the moments, dW_out and the workspace's partials dense at pitch D;
 * the workspace is sized by cpc_probe_layout_d and nothing else.  Every logit is the fmaf chain over k = 0 .. D - 1 in that
 * order, in both walks; LDS rows are padded with zeros to the next multiple of 4 only, and the k loop follows D.  x and W are
 * read 16 bytes at a time where base, row pitch and D allow (base 16-byte aligned, ldx % 4 == 0, D % 4 == 0), one float at a
 * time otherwise.  64 classes per step up to 256 features, 32 above (csrc/probe.hip: probe_wide_kernel).  D = 256 gives the bits
 * of the calls above; limits, flags, orders and everything else are theirs. */
int cpc_probe_layout_d(int R, int C, int D, long* sizes);
int cpc_probe_train_step_d(const float* x, long ldx, const long long* labels, int R, int C, int D, float* W, float* b,
                           float* exp_avg_W, float* exp_avg_sq_W, float* exp_avg_b, float* exp_avg_sq_b, double lr, double beta1,
                           double beta2, double eps, double bias_correction1, double bias_correction2_sqrt, float* workspace,
                           float* loss, double* acc, double* accum, float* dW_out, float* db_out, void* stream);
int cpc_probe_eval_d(const float* x, long ldx, const long long* labels, int R, int C, int D, const float* W, const float* b,
                     float* workspace, float* loss, double* acc, double* accum, void* stream);

/* ------------------------------------------------------------ phone posteriors ----
 * What cpc/feature_loader.py:61-71 (ModelPhoneCombined.forward) computes behind the feature maker: the linear classifier of
 * PhoneCriterion / CTCPhoneCriterion on R rows of 256 features, then softmax -- or argmax and one-hot -- in one launch
 * (csrc/posterior.hip).  The x tile of 32 rows is read once and kept in LDS while the classes are walked 64 at a time; logits
 * and unnormalised values never leave the chip, there is no workspace, and every element of out is stored exactly once.
 * Exact-f32 MFMA products, fixed orders, no atomics: identical calls give identical bits.  Arguments are checked before the launch.
 * 2 <= C <= 8192, R >= 1, R * C < 2^31 (CPC_ERR_SHAPE beyond).  x: row r at x + r * ldx (ldx >= 256; pointers and strides that are
 * not 16-byte aligned are read with scalar loads); W (C,256), b (C).
 * mode 0: out = float (R,C), softmax(x W^T + b) per row.  mode 1: out = long long (R,C), 1 at the row's argmax (the first index
 * of the maximum on ties, as torch.argmax) and 0 elsewhere.  argmax (or NULL): int32 (R), written in both modes. */
int cpc_posterior_forward(const float* x, long ldx, const float* W, const float* b, int R, int C, int mode, void* out,
                          int* argmax, void* stream);
/* The same on D features per row, 1 <= D <= 512 (CPC_ERR_SHAPE beyond; checked first): ldx >= D, W (C,D) dense.  LDS rows hold D
 * rounded up to 16 columns, the padding zero (an MFMA group contracts 16 k; 0 * 0 adds exactly 0).  x and W are read 16 bytes at
 * a time where D % 4 == 0, the base is 16-byte aligned and (x) ldx % 4 == 0, one float at a time otherwise.  Above 256 features
 * the class step is 32 and a tile's logits stay in LDS up to 192 classes (64 and 384 otherwise).  D = 256 gives the bits of the
 * call above. */
int cpc_posterior_forward_d(const float* x, long ldx, const float* W, const float* b, int R, int C, int D, int mode, void* out,
                            int* argmax, void* stream);

/* ---------------------------------------------------------------- ABX evaluation ----
 * cpc/eval/ABX.py and cpc/eval/ABX/{abx_group_computation.py, dtw.pyx}: frame distances, normalised DTW and the per-group
 * score 1 - theta of get_theta_group_dtw, batched over a whole pass (csrc/abx.hip).
 * Frames: feat (n_frames, D) fp32, D <= 1024; segment s is rows [seg_off[s], seg_off[s] + seg_len[s]) (int32), every length in
 *   [1, max_len], max_len <= 1024.  metric 0: cosine, acos(clamp(<x,y>, -1, 1)) / pi (frames normalised by the caller:
 *   normalize_with_singularity); 1: euclidean, sqrt(sum (x - y)^2).  Exact-f32 fmaf chains.  A DTW is a function of its two
 *   segments and the metric alone: the same pair gives the same bits in any group, position or launch.
 * cpc_abx_layout(D, max_len, n_groups, n_pairs, sizes): sizes[0] = floats of the pair scratch (n_pairs = sum over groups of
 *   Nx (Na + Nb)), sizes[1] = longest segment accepted, sizes[2] / sizes[3] = rows / cells of the LDS fast path.
 * cpc_abx_group_scores: plan = members (A ids, B ids, X ids per group), groups (G, 4) int32 = (first member, Na, Nb, Nx),
 *   pair_base (G) int64 = offset of the group's dxa (Nx, Na) then dxb (Nx, Nb) in dist, work (n_work, 2) int32 = (group, x index)
 *   for every x member of every group.  symmetric (within): X is A, only j > i is computed (x_i the rows) and mirrored, the
 *   diagonal is written 0 and replaced by max(dxb) + 1 in the count.  scores[g] = 1 - theta, theta =
 *   f32(cnt_lt + f32(0.5 cnt_eq)) / (n_pos Nb), n_pos = Na (Na - 1) symmetric, Na Nx otherwise.
 * cpc_abx_pair_dtw: out[q] = DTW(rows = segment pairs[2q], columns = segment pairs[2q + 1]).
 * cpc_abx_dtw: DTW on the caller's distance tensor dist (N1, N2, S1, S2), sizes size1 (N1) / size2 (N2) int32, out (N1, N2), with
 *   dtw_batch's ignore_diag (diagonal 0) and symmetric (j >= i computed and mirrored; N1 == N2).
 * A segment id or size out of range is clamped for addressing, raises CPC_DEVERR_ABX_INDEX and makes that score (distance) NaN. */
int cpc_abx_layout(int D, int max_len, int n_groups, long n_pairs, long* sizes);
int cpc_abx_group_scores(const float* feat, const int* seg_off, const int* seg_len, int n_seg, long n_frames, int D, int max_len,
                         int metric, const int* members, const int* groups, const long long* pair_base, int n_groups,
                         const int* work, int n_work, int symmetric, float* dist, float* scores, void* stream);
int cpc_abx_pair_dtw(const float* feat, const int* seg_off, const int* seg_len, int n_seg, long n_frames, int D, int max_len,
                     int metric, const int* pairs, int n_pairs, float* out, void* stream);
int cpc_abx_dtw(const float* dist, const int* size1, const int* size2, int N1, int N2, int S1, int S2, int ignore_diag,
                int symmetric, float* out, void* stream);

/* ---------------------------------------------------------------- PER evaluation ----
 * cpc/criterion/seq_alignment.py: beam_search (CTC prefix beam search) and NeedlemanWunschAlignScore, batched (csrc/ctc_decode.hip).
 * cpc_ctc_decode_layout(B, T_max, P, n_keep, sizes): sizes[0] = bytes of the beam-search scratch, [1] = bytes of one beam's label
 *   row, [2] / [3] = LDS bytes of the float64 / float32 search, [4] = largest n_keep, [5] = largest P, [6] = largest hypothesis
 *   length of cpc_nw_align_score.  CPC_ERR_SHAPE for n_keep outside [1, 128] or P outside [2, 128].
 * cpc_ctc_beam_search: probs (B, T_max, P) probabilities at element strides (stride_b, stride_t, stride_p), dtype 0 float32 /
 *   1 float64 -- the arithmetic is the input's; lengths (B) int32 frames per sequence in [1, T_max].  One workgroup per sequence
 *   runs beam_search(probs[b, :lengths[b]], n_keep, blank) and writes the n_out <= n_keep best beams in the reference's ranked
 *   order: labels (B, n_out, T_max) int32 padded with -1, label_len (B, n_out), scores (B, n_out) in the input dtype, n_beams (B) =
 *   min(n_keep, candidates of the last step); slots past n_beams have length 0 and score 0.  Bit-identical to the reference for
 *   the same input, ties included (broken by its string key).  scratch: sizes[0] bytes (caller-owned, no initialisation).
 * cpc_nw_align_score: out[b] = NeedlemanWunschAlignScore(ref[b, :ref_len[b]], hyp[b, :hyp_len[b]], d, m, r, normalize) in float64,
 *   rows at element strides ref_stride / hyp_stride, ref_len in [0, L1], hyp_len in [0, L2], L2 <= sizes[6].  normalize with
 *   ref_len 0 gives NaN (the reference divides by zero).  get_seq_PER is (d, m, r) = (-1, -1, 0), normalize 1. */
int cpc_ctc_decode_layout(int B, int T_max, int P, int n_keep, long* sizes);
int cpc_ctc_beam_search(const void* probs, int dtype, long stride_b, long stride_t, long stride_p, const int* lengths, int B,
                        int T_max, int P, int blank, int n_keep, int n_out, void* scratch, long scratch_bytes, int* labels,
                        int* label_len, void* scores, int* n_beams, void* stream);
int cpc_nw_align_score(const int* ref, long ref_stride, const int* ref_len, int L1, const int* hyp, long hyp_stride,
                       const int* hyp_len, int L2, int B, double d, double m, double r, int normalize, double* out, void* stream);

/* ---------------------------------------------------------------- transformer layer ----
 * One TransformerLayer of cpc/transformers.py:103-111 (buildTransformerAR, :130-139), d_model 256, 8 heads,
 * d_ff 2048, sequence S <= 128, dropout not applied.  Used as the auto-regressive network (--arMode
 * transformer, cpc/feature_loader.py:138-141, S = 128) and as a prediction network (--rnnMode transformer,
 * cpc/criterion/criterion.py:82-88, S = 128 - K).  BASELINE.json config 4.
 * params / grads: 13 pointers in the reference's state-dict order -- multihead.Wo, Wk, Wq, Wv .weight (256,256),
 * multihead.Att.Krelpos (32,S) (NULL = abspos layer without the relative term), ln_multihead.weight, .bias,
 * ffnetwork.lin1.weight (2048,256), .bias, ffnetwork.lin2.weight (256,2048), .bias, ln_ffnetwork.weight, .bias.
 * sizes[0] = saved floats, [1] = forward scratch floats, [2] = backward scratch floats, [3..7] = offsets inside
 * `saved` of qkv (B*S,768), A (B*8,S,S), o, y (B*S,256), hid (B*S,2048) = relu(lin1(y)).
 * 128 < S <= 512 (a layer built for a longer window -- the 400 frames of a 64000-sample feature-extraction chunk,
 * cpc/feature_loader.py:247-266): FORWARD ONLY, without dropout -- attention as a running-softmax walk over 128-key blocks
 * (attn_fwd_long_kernel); the attention probabilities A are not kept (size 0), the backward entry points refuse such S. */
int cpc_transformer_layout(int B, int S, long* sizes);
int cpc_transformer_layer_forward(const float* x, const float* const* params, float* saved, float* scratch,
                                  float* out, int B, int S, void* stream);
int cpc_transformer_layer_backward(const float* x, const float* const* params, const float* saved,
                                   const float* dy, float* scratch, float* dx, float* const* grads,
                                   int B, int S, void* stream);
/* Training mode with dropout probability p (0 <= p < 1) on the attention probabilities and on the feed-forward hidden
 * layer (cpc/transformers.py:18,50,93,100; the reference hard-codes 0.1).  Masks are a pure function of `seed` and the
 * element index (Philox4x32-10): give the backward call the seed of its forward call.  p = 0 is the plain layer. */
int cpc_transformer_layer_forward_dropout(const float* x, const float* const* params, float* saved, float* scratch,
                                          float* out, int B, int S, float p, unsigned long long seed, void* stream);
int cpc_transformer_layer_backward_dropout(const float* x, const float* const* params, const float* saved,
                                           const float* dy, float* scratch, float* dx, float* const* grads, int B,
                                           int S, float p, unsigned long long seed, void* stream);
/* the hidden layer (B*S, 2048) of the forward call that filled `saved`, as fp32 whatever its storage (the DMA-fed feed-forward
 * GEMMs keep it as two fp16 pieces per element); tests / inspection; synchronises `stream` */
int cpc_transformer_hidden(const float* saved, float* out, int B, int S, void* stream);
/* feed-forward GEMMs of the transformer layer (cpc/transformers.py:86-101) on the DMA-fed tiles: 0 off, 1 (default) where a
 * call's launches fill the chip (the K predictors as a group), 2 always; + 4: without the 128-row tail launch of the one-tile-wide
 * products, + 8: ReLU / dropout as a pass behind lin1 instead of in its epilogue (A/B); must not change between a forward and its backward */
int cpc_set_gemm_dma(int mode);
/* wave tile of the DMA-fed plain NT products' 256-row tiles: 64 = eight waves of 64 x 128 (two per SIMD), 128 = four waves of
 * 128 x 128 (one per SIMD, accumulators in AGPRs, a four-stage 16-k loop: csrc/dma_tile.h); same products in the same order: same bits */
int cpc_set_dma_wave_rows(int rows);
int cpc_set_gemm_tail_cus(int cus);     /* CU count the DMA-fed NT products' tail split plans for (0 = the device's; tests) */
int cpc_set_attn_fwd(int variant);       /* forward attention kernel (S <= 128): 1 = two workgroups per CU (default), 0 = one; same bits */
/* G transformer layers of one shape on ONE input x (B,S,256), every kernel launched once for all of them: the K predictors
 * of the criterion in --rnnMode transformer (cpc/criterion/criterion.py:82-88, :97-118).  params[i] / grads[i]: the G
 * tensors of kind i stacked, layer g at + g * numel; saved / scratch: G workspaces of cpc_transformer_layout's sizes back
 * to back; out / dy: (B*S, G*256) with layer g at columns g*256..; dx (B,S,256): the SUM of the layers' input gradients.
 * Dropout masks of layer g: those of a single-layer call with seed + g. */
int cpc_transformer_group_forward(const float* x, const float* const* params, float* saved, float* scratch, float* out,
                                  int B, int S, int G, float p, unsigned long long seed, void* stream);
int cpc_transformer_group_backward(const float* x, const float* const* params, const float* saved, const float* dy,
                                   float* scratch, float* dx, float* const* grads, int B, int S, int G, float p,
                                   unsigned long long seed, void* stream);
/* Test helper: out[i] = keep_i / (1 - p) of dropout site 0 (attention probabilities, flat ((b*8 + head)*S + i)*S + j; n a
 * multiple of S*S) or 1 (hidden layer, flat row*2048 + col; S ignored) under `seed`. */
int cpc_dropout_keep_mask(float* out, long n, int site, int S, float p, unsigned long long seed, void* stream);

/* ---------------------------------------------------------------- criterion ----
 * CPCUnsupersivedCriterion.forward (criterion.py:225-257) with linear prediction heads
 * (PredictionNetwork, criterion.py:90-91,97-118) and the negatives of sampleClean
 * (criterion.py:174-219) supplied as row indices.
 *   c, z : (B,S,256) context / encoded features;  W = S - K windows per sequence
 *   wall : (K*256, 256) the K head weights `wPrediction.predictors.k.weight` stacked
 *   ext  : (B*W, N) int32, ext[(b*W+t)*N + n] = row of z.view(B*S,256) used as negative n
 *          of window (b,t)  ==  criterion.py:199's extIdx[b,n,t]
 *   losses, acc : K floats (criterion.py:256-257)
 * K <= 16 per call (cpc_nce_head_group walks more), any N > 0.  sizes[0..2] = saved / fwd-scratch / bwd-scratch floats,
 * sizes[3..5] = offsets of pred, logits (B*W,K,1+N), lse (B*W,K) inside `saved`. */
int cpc_nce_layout(int B, int S, int K, int N, long* sizes);
/* Negatives per window as the kernels lay them out: N (criterion.py:176-189 draws any number) rounded up to the 16-wide MFMA
 * tile.  The padding candidates are valid rows whose logits the scoring kernels force to -3e38: weight 0 in the softmax, the
 * arg-max and every gradient.  ext is (B*W, padded) int32, logits (B*W, K, 1 + padded), perm / work count padded + K candidates
 * per window; the draws (batchIdx / seqIdx) stay B*N*W. */
int cpc_nce_padded_negatives(int N);
/* More than 16 prediction steps (criterion.py:225-257 takes any nPredicts): the score tiles hold 16 heads, so such a criterion
 * is walked in groups of at most 16.  After cpc_nce_head_group(k0, k_total) every cpc_nce_* call of the CALLING THREAD works on
 * heads k0 .. k0+K-1 of a criterion with k_total steps: W = S - k_total windows per sequence, head k's positive is
 * z[b, t + k0 + k + 1]; `wall` / `pred` / losses / acc are the group's K heads.  Per-head results are independent, dc / dz of the
 * groups add.  (0, 0) ends it; every call of a group -- layout, prepare, forward, backward -- is made under the same setting. */
int cpc_nce_head_group(int k0, int k_total);
/* Index preparation: the two int64 draws of sampleClean (criterion.py:181-189; B*N*W each, flat (b,n,t)
 * order) -> ext (the rows of criterion.py:191-199, laid out (b,t,n) with the N rows of a window in ASCENDING order: the
 * criterion is invariant under a permutation of a window's negatives, and sorted lists keep the gathers of the scoring
 * kernels inside L2) and the destination-sorted candidate slots (perm, row_ptr) the backward uses.
 * work: B*W*(N+K) + 2*B*S + 2 ints. */
int cpc_nce_prepare(const long* batchIdx, const long* seqIdx, int* ext, int* perm, int* row_ptr, int* work,
                    int B, int S, int K, int N, void* stream);
int cpc_nce_forward(const float* c, const float* z, const float* wall, const int* ext, float* saved,
                    float* scratch, float* losses, float* acc, int B, int S, int K, int N,
                    void* stream);
/* The operand bounds of the criterion's GEMMs (max|c|, max|wall|, kept in `saved`) ahead of time, on any stream: max|wall| is
 * fixed once the optimiser has stepped and a recurrent context is bounded a priori (c_bound > 0: |c| <= c_bound, e.g. 1 for a
 * GRU; otherwise c is reduced here), so the reduction need not sit between the autoregressive network and the prediction
 * GEMM.  cpc_nce_forward_prepared is cpc_nce_forward on a `saved` whose bounds were written by cpc_nce_bounds. */
int cpc_nce_bounds(const float* c, float c_bound, const float* wall, float* saved, int B, int S, int K, int N, void* stream);
int cpc_nce_forward_prepared(const float* c, const float* z, const float* wall, const int* ext, float* saved,
                             float* scratch, float* losses, float* acc, int B, int S, int K, int N, void* stream);
/* cpc_nce_forward (bounds_ready == 0) / cpc_nce_forward_prepared (!= 0) with the loss / accuracy reduction on finalize_stream,
 * ordered behind the scoring kernel by an event: the backward reads the saved logits, never the losses, so a caller that joins
 * finalize_stream before reading losses / acc keeps that launch off its critical stream. */
int cpc_nce_forward_streams(const float* c, const float* z, const float* wall, const int* ext, float* saved, float* scratch,
                            float* losses, float* acc, int B, int S, int K, int N, int bounds_ready, void* stream,
                            void* finalize_stream);
/* The share of the backward that depends on the weights, the operand bounds in `saved` (cpc_nce_bounds) and gloss only --
 * gradient scales, GEMM operand bounds, cleared maximum slots, the zeroed tail rows of dc, wall^T -- ahead of time on any stream
 * that has seen cpc_nce_bounds; cpc_nce_backward_prepared, on a stream that has waited for it, is then
 * cpc_nce_backward_streams(dz = NULL, dwall = NULL) without those launches (cpc_nce_backward_dz / _dwall follow as usual). */
int cpc_nce_backward_prepare(const float* wall, const float* saved, const float* gloss, float* scratch, float* dc, int B, int S,
                             int K, int N, void* stream);
int cpc_nce_backward_prepared(const float* c, const float* z, const float* wall, const int* ext, const int* perm,
                              const int* row_ptr, const float* saved, const float* gloss, float* scratch, float* dc, int B,
                              int S, int K, int N, void* stream);
/* gloss: K upstream gradients dL/dloss_k.  dc, dz (B,S,256) and dwall are overwritten.
 * perm (B*W*(N+K)) / row_ptr (B*S+1): candidate slots sorted by destination row of z (slot =
 * (b*W+t)*(N+K)+j; j<N: negative j -> row ext[..j]; j>=N: positive of head j-N -> row b*S+t+j-N+1);
 * they turn the gradient scatter into an atomics-free, reproducible per-row reduction.  With linear heads
 * (pred_k = W_k c) dz is re-associated through c:  dz[j] = sum_k W_k . G[j,k,:],  G[j,k,:] = sum over the slots landing
 * on row j of dS[slot,k] * c[window(slot)]  -- a per-row gather-GEMM over 1 KB rows of c, then one dense GEMM with the
 * stacked heads; no per-candidate gradient rows are materialised (criterion.py:108-116,199-217 backward). */
int cpc_nce_backward(const float* c, const float* z, const float* wall, const int* ext,
                     const int* perm, const int* row_ptr, const float* saved, const float* gloss,
                     float* scratch, float* dc, float* dz, float* dwall, int B, int S, int K, int N,
                     void* stream);

/* As cpc_nce_backward with the dz path (Wcat + gather-GEMM G + dz GEMM; it depends on the score gradients this call
 * writes first, not on dpred / dc / dwall) launched on dz_stream behind an event, so that it can run beside the
 * auto-regressive network's backward; dz == NULL leaves the dz path out (run it later with cpc_nce_backward_dz, same
 * scratch, on a stream that waits for this call).  Every consumer of dz must wait for dz_stream. */
int cpc_nce_backward_streams(const float* c, const float* z, const float* wall, const int* ext,
                             const int* perm, const int* row_ptr, const float* saved, const float* gloss,
                             float* scratch, float* dc, float* dz, float* dwall, int B, int S, int K, int N,
                             void* stream, void* dz_stream);

int cpc_nce_backward_dz(const float* c, const float* wall, const int* perm, const int* row_ptr, const float* saved,
                        float* scratch, float* dz, int B, int S, int K, int N, void* stream);

/* cpc_nce_backward_streams also accepts dwall == NULL: the head-weight gradient (criterion.py:44-50, the K
 * nn.Linear weights) is then left out and formed later by this call from the dPred kept in `scratch`; nothing on
 * the way to the encoder depends on it.  `stream` must wait for the cpc_nce_backward_streams call. */
int cpc_nce_backward_dwall(const float* c, const float* saved, float* scratch, float* dwall, int B, int S, int K, int N,
                           void* stream);
/* The linear heads' criterion in ONE gather pass (1; default since round 6: 2, below): the scoring kernel of cpc_nce_forward* carries the softmax-weighted
 * sum of the candidate rows along with the log-sum-exp (an online softmax over criterion.py:108-116's candidates) and leaves
 * T = d loss_k / d pred_k for a unit upstream gradient in `saved`; the backward then has no score-gradient pass over the 1 KB
 * candidate rows (criterion.py:200-201's gather, 1.06 GB at B = 64) -- the heads' upstream gradients are folded into the dc
 * GEMM's weight operand and the weight gradient's reduction, the dz path multiplies the softmax rows the forward leaves per
 * candidate slot.  0: the two-pass kernels.  A forward and its backward run under the same setting. */
int cpc_set_nce_fused(int on);
/* (on = 2, round 6: the same one-pass criterion with the scoring kernel on the 16-bit matrix pipe -- both products as hh + hl + lh
 * of two fp16 pieces, the arithmetic of the conv layers -- gathering from an H2 copy of z that goes global -> LDS by DMA, the
 * contraction over candidates fed by the transposing LDS read; on = 3: the dz path's gather-GEMM likewise, from an H2 copy of c.
 * Same interface, same saved tensors.) */
int cpc_get_nce_fused(void);
/* cpc_set_nce_fused(2 / 3): workgroups of the scoring kernel -- 0 = one per four windows, -1 (default) = two per CU, n > 0 = at most n (a capped
 * grid walks its windows with the grid's stride, so that all resident waves sweep their ascending candidate lists in step). */
int cpc_set_nce_grid(int wgs);
/* cpc_set_nce_fused(2 / 3): 1 (default) = the softmax rows the dz path reads are written by a launch of their own, on the stream
 * the loss reduction runs on (cpc_nce_forward_streams' finalize_stream: off the forward's chain), 0 = inside the scoring kernel. */
int cpc_set_nce_rows_apart(int on);
/* The prediction product pred = c . wall^T of the K linear heads (cpc/criterion/criterion.py:108-116): 1 (default) = on the DMA-fed
 * 256 x 256 tile of csrc/gemm_dma.hip (c as an H2 copy, the stacked weights re-laid beside the operand bounds), 0 = on the generic
 * register-staged tile.  Same fp16-piece arithmetic, another order of summation. */
int cpc_set_nce_heads_dma(int on);
/* Measurement switch of the cpc_set_nce_fused(2) scoring kernel (tools/time_nce.py: what each part of it costs): bit 0 leaves the
 * softmax-row pass out, 1 the T epilogue, 2 the weighted row sum, 3 the logits stores.  Results are WRONG while mask != 0. */
int cpc_set_nce_debug(int mask);
/* cpc_set_nce_fused(2 / 3): the H2 copy of z (criterion.py:200-201's gather source) ahead of time on `stream` -- z is final when
 * the encoder has run; the calling thread's next cpc_nce_forward* then skips the two small launches.  No-op in other modes. */
int cpc_nce_prepare_z(const float* z, float* saved, int B, int S, int K, int N, void* stream);
/* Tuning switch: at most n workgroups per launch of cpc_nce_prepare's kernels (each then walks several windows / slots);
 * -1 (default) = the device's CU count, 0 = one per 4 windows / 256 slots.  Same lists either way. */
int cpc_set_index_prep_groups(int n);
/* Tuning switch of the composite step (single-rank calls, phases 3): 1 (default) = the recurrence's weight / bias gradients run on
 * the preparation stream, which is idle during the backward, instead of in front of the conv layers' on the weight-gradient
 * stream (0).  Same kernels, same values. */
int cpc_set_gru_wgrad_stream(int on_prep);

/* The same criterion for predictions formed by the caller -- any prediction network of
 * cpc/criterion/criterion.py:44-118, e.g. K transformer layers (--rnnMode transformer, :82-88):
 * pred (B*W, K*256), row (b,t), head k at columns k*256..; implements :115-116 (mean over 256 of pred * candidate)
 * and :245-257.  Layout / scratch sizes as cpc_nce_layout (the `pred` part of `saved` stays unused).
 * backward overwrites dpred (B*W, K*256) and dz (B,S,256). */
int cpc_nce_scores_forward(const float* pred, const float* z, const int* ext, float* saved, float* scratch,
                           float* losses, float* acc, int B, int S, int K, int N, void* stream);
int cpc_nce_scores_backward(const float* pred, const float* z, const int* ext, const int* perm,
                            const int* row_ptr, const float* saved, const float* gloss, float* scratch,
                            float* dpred, float* dz, int B, int S, int K, int N, void* stream);

/* The same scores at any encoder width 1 <= C <= 512 (cpc/criterion/criterion.py:89-95 takes any dimOutputEncoder; :116's mean is
 * over C), on exact-f32 MFMAs (csrc/nce_wide.hip).  The kernels work on the padded width Cp = cpc_nce_wide_padded_width(C) = C
 * rounded up to a multiple of 64 (0 for C < 1 or C > 512): pred is (B*W, K*Cp), z (B, S, Cp), columns C .. Cp-1 ZERO; dpred and dz
 * have the same shapes and come out exactly zero there.  ext / perm / row_ptr are those of cpc_nce_prepare (they do not depend
 * on the width); K <= 16 per call, more heads through cpc_nce_head_group; any N >= 1 (padded as cpc_nce_padded_negatives).
 * sizes (floats): [0] saved, [1] forward scratch, [2] backward scratch (B*W*(Np+K)*Cp candidate rows: every offset is 64-bit),
 * [3] offset of logits (B*W, K, Np+1) in saved, [4] of lse (B*W, K).  Every output is overwritten completely. */
int cpc_nce_wide_padded_width(int C);
int cpc_nce_wide_layout(int B, int S, int K, int N, int C, long* sizes);
int cpc_nce_wide_forward(const float* pred, const float* z, const int* ext, float* saved, float* scratch,
                         float* losses, float* acc, int B, int S, int K, int N, int C, void* stream);
int cpc_nce_wide_backward(const float* pred, const float* z, const int* ext, const int* perm, const int* row_ptr,
                          const float* saved, const float* gloss, float* scratch, float* dpred, float* dz,
                          int B, int S, int K, int N, int C, void* stream);

/* ---- the whole step ---------------------------------------------------------------------------------------------------
 * cpc/train.py:78-87 for the north-star configuration (CPCEncoder + 2-layer GRU CPCAR + K linear InfoNCE heads): model
 * forward, criterion forward, allLosses.sum().backward() -- every launch of the entry points above, issued from ONE call on
 * four caller-owned streams with the cross-stream order of the package's Python train loop (ops.py / train.Trainer), i.e. the
 * same kernels in the same order: results are bit-identical to that loop.  What it saves is host time (~60 launches, three
 * autograd nodes and a dozen allocator calls per step from Python), which is what an eager data-parallel rank is bound by.
 *   wave (B,1,L); batchIdx, seqIdx: the two int64 draws of sampleClean (criterion.py:181-189), B*N*W each, ready on
 *   side_stream (or earlier on main_stream); h0: NULL or the carried GRU state (2,B,256), hN (2,B,256) receives the final one
 *   (cpc/model.py:193-198); c_bound > 0: an a-priori bound of |c| (1 for a GRU started from zero or from one of its own final
 *   states), <= 0: max|c| is reduced in line; params / grads: 29 pointers -- the 20 encoder tensors (cpc_encoder_forward's
 *   order), the 8 GRU tensors (cpc_gru_forward's order), the K head weights stacked (K*256, 256); grads are OVERWRITTEN
 *   (= zero_grad + backward); gloss: K floats dL/dloss_k (ones for train.py:85's sum); workspace: cpc_train_step_layout
 *   sizes[0] floats, reused from step to step (z and c of the step live in it at sizes[1], sizes[2] until the next call);
 *   losses, acc: K floats each (criterion.py:256-257).
 * phases (bit mask): 1 = forward + backward down to the encoder's input gradient -- on return the heads' gradient is queued
 * on side_stream, the recurrence's on wgrad_stream, everything else of the non-encoder gradients is final on main_stream (a
 * data-parallel caller starts reducing that bucket here); 2 = the encoder's backward, after which main_stream has waited for
 * side_stream and wgrad_stream: every gradient is final on main_stream.  3 = both.  No host synchronisation anywhere.
 * Cross-step pipelining of a single-rank loop (cpc/train.py:78-91 is strictly serial: backward, optimizer.step, next forward):
 *   + 4 (with 2) open tail: main_stream does not wait for the step's LAST kernel, layer 1's weight gradient on wgrad_stream
 *     (0.13 ms past the end of main_stream's chain), and the bias / norm gradient sums of layers 1..4 run on prep_stream beside
 *     the chain's last kernels.  The caller then updates conv0's parameters on main_stream, conv1.weight on wgrad_stream and the
 *     rest on prep_stream (cpc_adam_step three times, cpc_train_step_wait for their gradients), calls cpc_train_step_tail, and gives
 *     the NEXT step + 8 (its weight layouts are ready; main_stream waits for conv1's in front of layer 1) and alternates + 16
 *     (second y0 buffer / bound set of the workspace: the next layer 0 runs while layer 1's weight gradient still reads y0).
 *   A caller that touches parameters or gradients outside these calls first joins with cpc_train_step_wait(main, 2, main).
 *   + 32 (with 1; h0 must be NULL, else CPC_ERR_ARG): the caller reads neither hN nor c beyond step W - 1, W = S - K -- the steps
 *     the criterion reads.  The forward recurrence then runs W steps instead of S: c[:, W:] is zero and hN is NOT written.  Losses,
 *     accuracies, z, c[:, :W] and every gradient are those of the step without the bit.  (Taken up with c_bound > 0; with a
 *     measured bound the step runs all S steps.)  The recurrence's backward runs over W steps in every mask: dc[:, W:] is zero by
 *     construction, and the results are the full run's. */
int cpc_train_step_layout(int B, int L, int K, int N, long* sizes);
int cpc_train_step(const float* wave, const long* batchIdx, const long* seqIdx, const float* h0, float c_bound,
                   const float* const* params, float* const* grads, const float* gloss, float* workspace, float* losses,
                   float* acc, float* hN, int B, int L, int K, int N, int phases, void* main_stream, void* side_stream,
                   void* prep_stream, void* wgrad_stream);
/* The index lists of the NEXT step's draws, one step ahead (optional): queue it on side_stream after the current step's
 * cpc_train_step, with the next step's draws ready there; the next cpc_train_step -- same sizes and workspace -- is then given
 * batchIdx = seqIdx = NULL.  The preparation then runs beside the tail of the current step (layer 1's weight gradient alone on
 * the matrix pipes) instead of beside the next step's first conv layers. */
int cpc_train_step_prefetch(const long* batchIdx, const long* seqIdx, float* workspace, int B, int L, int K, int N,
                            void* side_stream);
/* The tail of an open-tailed step (phases + 4), after the optimiser's three launches (conv0's parameters on main_stream,
 * conv1.weight on wgrad_stream, every other parameter on prep_stream behind cpc_train_step_wait(main, 0 / 3 / 4, prep)): the
 * next step's weight preparation, each share on the stream its parameters arrive on, for parity next_parity, and the events the
 * next step's layer 1 waits for.  params: the 20 encoder tensors (cpc_encoder_forward's order). */
int cpc_train_step_tail(const float* const* params, float* workspace, int B, int L, int K, int N, int next_parity,
                        void* main_stream, void* prep_stream, void* wgrad_stream);
/* waiting_stream waits for events the last cpc_train_step on main_stream recorded: 0 = everything of wgrad_stream but layer 1's
 * weight gradient (the recurrence's and conv2..4's weight gradients: a data-parallel caller's mid gradient bucket), 1 = what an
 * open-tailed step left open (layer 1's weight gradient + the bias / norm gradient sums on prep_stream), 2 =
 * cpc_train_step_tail's end (every updated weight and layout), 3 = the heads' weight gradient, 4 = the bias / norm sums alone. */
int cpc_train_step_wait(void* main_stream, int which, void* waiting_stream);
/* In-step timing (diagnostic): while on, cpc_train_step records timing events around layer 0, layer 1, the two persistent
 * recurrence launches and the criterion's scoring kernel on main_stream; cpc_get_step_timing waits for the last and writes the
 * 5 durations of the most recent step in microseconds (conv0, conv1, forward recurrence, backward recurrence, scoring kernel;
 * each includes one marker's cost). */
/* The forward of a short conv layer (conv2..4 with H2 input, below the 128-row-tile regime; cpc/model.py:87-92,101-104) on
 * 128 x 128 tiles, two workgroups per 128-row tile with the ChannelNorm statistics (cpc/model.py:50-58) exchanged between the pair
 * through global memory, wherever that gives at least min_wgs workgroups (default 256; 0 = the full-row tiles).  spin_limit: polls
 * before a workgroup gives up on its partner (< 0: the default 2^22; tests use 0 to drive CPC_DEVERR_CONV_EXCHANGE). */
int cpc_set_fwd_nsplit(int min_wgs, int spin_limit);
int cpc_set_step_timing(int on);
/* Where the next step's layer 0 takes up an open tail: 0 behind the whole tail (layer 1's weight gradient, its split reduction, the
 * update of conv1.weight and that weight's layouts), 1 under it -- only layer 1 waits (layer 0 gets a quarter of its wave slots
 * beside layer 1's weight gradient) --, 2 (default since the end of round 6: -13 us per step) behind the weight gradient and its
 * reduction, beside the update and the layouts, 3 already behind the weight gradient's GEMM (an event more on that stream: no gain). */
int cpc_set_tail_schedule(int conv0_early);
int cpc_get_step_timing(float* us);
/* Measurement switches of cpc_train_step's schedule.  prep_point: where the criterion's index preparation (190 MB of index
 * traffic at B = 64) is released on side_stream -- 0 at the step's start (beside conv0, the one HBM-bound layer: 50 -> 96 us), 1
 * (default) behind conv0 (beside conv1 / conv2), 2 behind the encoder (beside the recurrence), 3 behind conv1 (beside conv2..conv4).  dz_early: 1 = the dz path on main_stream BEFORE the recurrence's
 * backward (which then has the memory system to itself) instead of beside it on side_stream (0, default); + 2 = the small
 * weight-only launches of the criterion / recurrence stay on main_stream; + 4 = the weight layouts of conv layers 1..4 are
 * prepared beside layer 0 on prep_stream instead of in front of it on main_stream (measured 8 us slower). */
int cpc_set_step_schedule(int prep_point, int dz_early);

/* ---- optimiser -------------------------------------------------------------------------------------------------
 * One Adam step (cpc/train.py:335-337: torch.optim.Adam(params, lr, betas, eps); :88-89 optimizer.step()) on n dense
 * fp32 tensors in one launch: exp_avg <- lerp(exp_avg, grad, 1 - beta1), exp_avg_sq <- beta2 exp_avg_sq + (1 - beta2)
 * grad^2, param <- param - (lr / bias_correction1) exp_avg / (sqrt(exp_avg_sq) / bias_correction2_sqrt + eps), all in
 * place.  bias_correction1 = 1 - beta1^step, bias_correction2_sqrt = sqrt(1 - beta2^step), step counted from 1.
 * No weight decay / amsgrad / maximize (the reference uses none). */
int cpc_adam_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                  const long* numel, int n, double lr, double beta1, double beta2, double eps, double bias_correction1,
                  double bias_correction2_sqrt, void* stream);
/* The same with the step counter on the device: nothing changes from call to call on the host side, so the launch can be
 * part of a captured HIP graph.  step: one device double = updates done so far (incremented by the call); coef: 8 device
 * floats of scratch. */
int cpc_adam_step_capturable(float* const* params, const float* const* grads, float* const* exp_avg,
                             float* const* exp_avg_sq, const long* numel, int n, double lr, double beta1, double beta2,
                             double eps, double* step, float* coef, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CPC_HIP_H */
