/*
 * onssen_hip.h -- C ABI of libonssen_hip.so, the MI355X (gfx950) implementation of
 * onssen's STFT-domain separation forward pass.
 *
 * The upstream project is pure Python on PyTorch ATen ops; it has no FFI of its
 * own ("C ABI ... new; nothing in the reference to mirror").
 * Each entry point below therefore cites the reference *call site* it replaces
 * (paths relative to the upstream tree).  The binding a maintainer adds on the
 * reference side is a ctypes stub; see INTEGRATION.md.
 *
 * Conventions
 *  - All pointers are DEVICE pointers (HBM) unless the parameter name ends in
 *    `_host`.  The caller owns every buffer including workspaces; the library
 *    never allocates, frees or synchronises (safe under hipGraph capture).
 *  - `stream` is a hipStream_t passed as void*; work is stream-ordered.
 *  - Return value: 0 = ok; >0 = hipError_t of a failed launch; <0 = ONSSEN_E_*.
 *    No exceptions cross the ABI.  Functions are re-entrant; one in-flight call
 *    per workspace.
 *  - dtype: fp32 at every boundary.  Contractions run either on the exact-fp32 MFMA
 *    (v_mfma_f32_16x16x4_f32; the *_f32 GEMM and the default BLSTM flags) or in split-bf16
 *    (three v_mfma_f32_16x16x32_bf16 per fp32 product, fp32 accumulate, ~1e-5 relative;
 *    ONSSEN_BLSTM_BF16X3, *_bf16x3, *_x3p) -- the caller chooses.  STFT / iSTFT butterflies
 *    run in fp64 like the reference's NumPy FFT.
 */
#ifndef ONSSEN_HIP_H
#define ONSSEN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ONSSEN_ABI_VERSION 14   /* 14 (additions, no signature changed): onssen_dc_cluster_k_f32 and onssen_dc_cluster_k_workspace_bytes (the deep-clustering back end for 2 .. 4 speakers).  14 (additions, no signature changed): onssen_sisnr_pit_* (Conv-TasNet's SI-SNR permutation-invariant training loss and its gradient).  14 (additions, no signature changed): onssen_tasnet_stream_* (stateful streaming inference of causal Conv-TasNet models).  14 (additions, no signature changed): onssen_tasnet_forward_ragged_f32 and onssen_tasnet_ragged_workspace_bytes (Conv-TasNet over whole utterances of different lengths).  14 (additions, no signature changed): onssen_tasnet_train_forward_f32, onssen_tasnet_backward_f32 and their two size queries (Conv-TasNet training).  14 (additions, no signature changed): onssen_tasnet_* (the Conv-TasNet separation forward).  14: onssen_blstm_pipe2_forward_ragged_f32 (the pipelined pair launch over a stream of RAGGED batches of whole utterances: each half of the launch runs its own batch's time steps and row lengths).  13: onssen_blstm_pipe2_* (a two-layer stack software-pipelined over consecutive calls: layer 1 of batch n-1 and layer 0 of batch n in ONE persistent launch, each on half of the XCDs).  12: onssen_log_magnitude_f32, onssen_cos_difference_f32, onssen_one_hot_f32 (the reference's stand-alone feature helpers).  11: onssen_wav_info, onssen_wav_read_batch_f32 (host-side batch RIFF reader of the file loader), onssen_lstm_pack_wih_image_f32, onssen_clip_adam_f32, onssen_lstm_train_backward_img_f32, onssen_lstm_pack_train_f32.  10: onssen_linear_x3p_norms, onssen_l2norm_rows_grad_y_f32, onssen_linear_x3p_batched_split_alt, onssen_x3_image_both_colsum_f32, onssen_dc_head_grad_images_f32, onssen_lstm_wgrad_images_f32, onssen_linear_x3t, onssen_blstm_x_image; ug = 24 (640 < H <= 768) in the persistent split-bf16 recurrence.  9: ragged batches of whole utterances (onssen_*_ragged_f32), the compacted deep-clustering back end, `tol` of onssen_dc_cluster_*, onssen_lstm_train_forward_form_f32.  8: onssen_linear_x3p_resid, onssen_linear_x3p_pair, onssen_x3_image_both_f32.  7: onssen_xcd_spin_limit, onssen_debug_cotenant_spin, chimera mask-loss gradient, compacted clustering.  6: onssen_dropout_f32, onssen_loss_dc_grad_f32, onssen_linear_x3p_batched_split, db_rows of onssen_lstm_train_backward_f32, l2norm_rows and bn_rows kernels; backward recurrence exchanges tagged partial sums.  5: status word [282] (non-finite h), W_hh fragment images unit-major, fp64 SDR workspace */

#define ONSSEN_OK 0
#define ONSSEN_E_ARG (-1)         /* invalid argument / unsupported shape */
#define ONSSEN_E_WORKSPACE (-2)   /* workspace too small */
#define ONSSEN_E_ALIGN (-3)       /* pointer / stride alignment requirement violated */
/* onssen_wav_*: per-file status / return codes (host-side reader, no device work) */
#define ONSSEN_WAV_TRUNCATED 1          /* the file holds more frames than the row: the first row_stride frames were read */
#define ONSSEN_WAV_E_OPEN (-16)         /* cannot open the file */
#define ONSSEN_WAV_E_FORMAT (-17)       /* not RIFF/WAVE, no fmt / data chunk, malformed */
#define ONSSEN_WAV_E_UNSUPPORTED (-18)  /* sample format other than PCM 8/16/24/32-bit or IEEE float 32/64 */
#define ONSSEN_WAV_E_SOME_FAILED (-19)  /* onssen_wav_read_batch_f32: at least one status_host[i] < 0 */

/* flags of onssen_blstm_forward_f32 */
#define ONSSEN_BLSTM_SPLIT_ROWS 1 /* 16 batch rows per recurrence workgroup instead of 32: more workgroups */
#define ONSSEN_BLSTM_BF16X3 2     /* recurrent product h W_hh^T in split-bf16 (3 bf16 MFMAs per fp32 product,
                                     ~1e-5 relative); whh_p_host[l] must then point to the images made by
                                     onssen_lstm_pack_whh_bf16x3 ([2 directions][whh_x3_elems] uint16), and
                                     wih_p_host[l] to onssen_linear_pack_bf16x3 planes of the [2*NP][K_l] matrix
                                     (ld = K_l rounded up to 32): the input projections run split-bf16 too.
                                     H <= 640. */
#define ONSSEN_BLSTM_XCD 4        /* (with BF16X3) one persistent launch per layer: every (direction, 4 / 8 / 16-row group)
                                     recurrence runs inside one XCD, W_hh register-resident, h_t exchanged through
                                     that XCD's L2 as data-tagged bf16 words (no flags).  Needs ceil(H/ug) <= 32,
                                     H <= 640, ug <= 20 -- or (round 4, split-bf16 only, without FUSE_IN0 / BF16 and
                                     not in the training forward) ug = 24: 640 < H <= 768.  The kernel verifies the placement itself and otherwise
                                     uses placement-independent (write-through / system-scope) accesses; bounded
                                     waits: ws word [281] = 1 reports that, word [280] != 0 an aborted launch
                                     (outputs invalid), word [282] = 1 a non-finite activation (a NaN cannot carry
                                     the exchange's tag: it was replaced by 0 -- outputs are NOT nn.LSTM's NaNs;
                                     the launch-per-step form propagates them).
                                     In this form the activations travel between the layers as x3 images (see
                                     onssen_linear_x3p) written by the recurrence epilogue: wih_p_host[l] must be the
                                     x3 image (onssen_x3_image_f32) of the packed [2*NP][K_l] input-projection
                                     matrix, and the last layer's output image stays in the workspace for the
                                     heads (onssen_blstm_y_image).
                                     WITHOUT ONSSEN_BLSTM_BF16X3 (round 3): the same persistent launch in EXACT fp32
                                     (v_mfma_f32_16x16x4_f32; h exchanged as tagged fp32 words): wih_p_host / whh_p_host /
                                     bias_p_host are the fp32 arrays of onssen_lstm_pack_f32 (as for the launch-per-step
                                     form), G comes from the exact-fp32 GEMM, the layers hand fp32 rows to each other,
                                     y must not be NULL; same limits (H <= 640, ug <= 20). */
#define ONSSEN_BLSTM_FUSE_IN0 16   /* (with XCD, in_dim <= 128, or = 129 with FUSE_TAIL) the first layer's input projection is computed inside its
                                     recurrence launch: wih_p_host[0] must be the B-fragment image made by
                                     onssen_lstm_pack_wih_bf16x3 of the layer's two W_ih, back to back; no G is
                                     written or read for that layer. */
#define ONSSEN_BLSTM_FUSE_TAIL 32   /* (with FUSE_IN0, in_dim = 32k + 1, e.g. F = 129) the lone last input column is a rank-1
                                     update on the VALU instead of a whole MFMA k-chunk: bias_p_host[0] then holds 4*NP
                                     floats -- the bias, then column in_dim-1 of the packed W_ih ([2*NP]). */
#define ONSSEN_BLSTM_BF16 64        /* (with BF16X3 | XCD) OPT-IN reduced precision: every product of the stack (input
                                     projections, h W_hh^T) uses the bf16 hi halves only -- one MFMA instead of
                                     three, bf16-grade results (~1e-2 relative), outside the 1e-4 parity contract.
                                     Same images, same workspace; accumulation, gates and cell state stay fp32. */
#define ONSSEN_BLSTM_G_READY 128     /* measurement aid (bench.py times the recurrence kernel by itself): skip the input
                                       projection of every layer -- G is what an earlier call with the same arguments left
                                       in the workspace (L = 1 calls only make sense) */
#define ONSSEN_BLSTM_WS_DIRTY 65536  /* (with XCD | BF16X3) the workspace behind its header was NOT zeroed for this shape (a grow-only
                                       scratch buffer reused across ragged batches of changing length): the call clears the k
                                       padding of the recurrence output images itself (two tiny launches) before it runs.  The
                                       header must still have been zeroed once by the owner. */
/* Debug flags (0 in production).  Launch-per-step form only: bits 8..11 switch off parts of the kernel for profiling
 * ablations (results are then meaningless): 0x100 h loads, 0x200 W_hh loads, 0x400 MFMA, 0x800 G/c loads; 0x1000 selects
 * libm-grade gate non-linearities.  ONSSEN_BLSTM_XCD form: 0x800 = TEST bit, rotates the exchange groups across the XCDs
 * so that the placement-independent accesses run; its profiling switches are build variants (lstm.inc). */

/* epilogue modes of onssen_linear_f32 */
#define ONSSEN_EPI_BIAS 0     /* C = A W^T + b                                   (nn.Linear)            */
#define ONSSEN_EPI_L2NORM 1   /* ... then x / max(||x||_2, eps) over `group` consecutive outputs        */
#define ONSSEN_EPI_SIGMOID 2  /* ... then logistic                                                      */
#define ONSSEN_EPI_BF16 0x100 /* OR-ed into `mode` of onssen_linear_x3p: plain bf16 products (the hi halves of the x3 images only,
                                 fp32 accumulate; ~2^-9 relative per product) instead of split-bf16                       */
#define ONSSEN_EPI_RELU 3     /* ... then max(x, 0), times `resid` (laid out like C) if given -- onssen_linear_f32 only
                                 (enhance: fc_pre / fc_post, onssen/nn/enhancement.py:49-51)           */

int onssen_abi_version(void);
const char* onssen_error_string(int code);

/* ---------------------------------------------------------------------------------------------
 * K1+K2  framed STFT + log-magnitude.
 * Replaces onssen/data/feature_utils.py:20 (librosa.core.stft(sig, n_fft, hop_length), transposed)
 * fused with :49-51 get_log_magnitude and :54-64 get_phase.
 *   wav      (B, n_samples) float32, row stride `wav_stride` elements
 *   logmag   (B, T, F) float32 = log10(|X| + eps),  T = 1 + n_samples/hop, F = n_fft/2 + 1
 *   stft_ri  (B, T, F, 2) float32 (Re, Im) of the complex64 STFT, or NULL
 * n_fft in {256, 512, 1024}; reflect padding needs n_samples > n_fft/2.
 */
int onssen_stft_logmag_f32(const float* wav, int B, int n_samples, int64_t wav_stride, int n_fft, int hop,
                           float eps, float* logmag, float* stft_ri, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Packed-weight geometry of one LSTM direction for unit-group size `ug` (a multiple of 4, <= 20).
 *   Hp = H rounded up to ug; NP = 4*Hp packed gate columns; KQ = ceil(Hp/16) k-chunks;
 *   whh_elems = floats of the MFMA-fragment-ordered recurrent weight image.
 */
int onssen_lstm_geometry(int H, int ug, int* Hp, int* NP, int* KQ, int64_t* whh_elems);

/* Pack one (layer, direction) of nn.LSTM parameters (state_dict layout, gate rows i,f,g,o;
 * onssen/nn/deep_clustering.py:15-22) into the images the kernels consume.
 *   w_ih (4H, in_dim), w_hh (4H, H), b_ih, b_hh (4H)
 *   bidir_in = 0: the layer input has in_dim plain columns; wih_p is [NP][Kp], Kp = in_dim rounded up to 4
 *   bidir_in = 1: the layer input is the previous layer's [fwd(H) | rev(H)]; it is stored by this
 *                 library as [fwd(Hp) | rev(Hp)], so wih_p is [NP][2*Hp] (in_dim must equal 2H)
 *   whh_p   [NU][KQ][ug/4][64][4]   bias_p [NP] = b_ih + b_hh (gate-permuted)
 */
int onssen_lstm_pack_f32(const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int in_dim,
                         int bidir_in, int H, int ug, float* wih_p, float* whh_p, float* bias_p, void* stream);

/* (round 5) One direction's packed W_ih, its bias and the x3 image of the packed matrix in ONE pass: what onssen_lstm_pack_f32's
 * wih_p / bias_p and onssen_x3_image_f32(wih_p, ...) give, bit for bit, without the fp32 whh image nobody reads on the persistent
 * training path.  The training forward re-packs every step (the optimizer moves the weights between two forwards), so
 * the pack is part of the training step (onssen/utils/train.py:75-86).  wih_img: this direction's NP rows of the
 * [2*NP][ceil(K/32)][2][32] image (K = in_dim, or 2*Hp with bidir_in), 16-byte aligned. */
int onssen_lstm_pack_wih_image_f32(const float* w_ih, const float* b_ih, const float* b_hh, int in_dim, int bidir_in, int H, int ug,
                                   float* wih_p, float* bias_p, uint16_t* wih_img, void* stream);

/* (round 5) ... and the whole stack's training images in ONE launch: per (layer l, direction d), index i = 2 l + d of every HOST
 * pointer array: onssen_lstm_pack_wih_image_f32 (layer 0: in_dim plain columns; deeper layers: bidir_in), onssen_lstm_pack_whh_bf16x3
 * and -- when whhR_host is not NULL -- onssen_lstm_pack_whhR_bf16x3, bit for bit what the single calls give.  wih_img_host[i]:
 * direction d's NP rows of layer l's image. */
int onssen_lstm_pack_train_f32(int L, int in_dim, int H, int ug, const float* const* w_ih_host, const float* const* w_hh_host,
                               const float* const* b_ih_host, const float* const* b_hh_host, float* const* wih_p_host,
                               float* const* bias_p_host, uint16_t* const* wih_img_host, uint16_t* const* whh_x3_host,
                               uint16_t* const* whhR_host, void* stream);

/* Split-bf16 image of one direction's W_hh (see ONSSEN_BLSTM_BF16X3): hi = bf16(w), lo = bf16(w - hi), in
 * v_mfma_f32_16x16x32_bf16 B-fragment order [NU][KQ2][ug/4][hi|lo][64][8], KQ2 = ceil(Hp/32). */
int onssen_lstm_geometry_x3(int H, int ug, int* KQ2, int* Hs, int64_t* whh_x3_elems);
int onssen_lstm_pack_whh_bf16x3(const float* w_hh, int H, int ug, uint16_t* whh_x3, void* stream);
/* The same B-fragment image for one direction's W_ih [4H][in_dim] (ONSSEN_BLSTM_FUSE_IN0):
 * [NU][ceil(in_dim/32)][ug/4][hi|lo][64][8] uint16, zero beyond in_dim. */
int onssen_lstm_pack_wih_bf16x3(const float* w_ih, int in_dim, int H, int ug, uint16_t* wih_x3, void* stream);

/* Pack a head nn.Linear(2H -> N) for the [fwd(Hp) | rev(Hp)] activation layout, optionally folding an
 * eval-mode nn.BatchNorm1d(2H) that precedes it (onssen/nn/deep_clustering.py:36-39):
 *   w_p[n][d*Hp+j] = w[n][d*H+j] * s[d*H+j],  b_p[n] = b[n] + sum_k w[n][k] * (beta[k] - mean[k]*s[k]),
 *   s = gamma / sqrt(var + bn_eps).  Pass bn_gamma = NULL for no BatchNorm (chimera heads).
 */
int onssen_head_pack_f32(const float* w, const float* b, int N, int H, int Hp, const float* bn_gamma,
                         const float* bn_beta, const float* bn_mean, const float* bn_var, float bn_eps,
                         float* w_p, float* b_p, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K3/K7/K8/K9  C = epilogue(A W^T + bias)   (exact-fp32 MFMA GEMM, fused epilogue).
 * Replaces nn.Linear + F.normalize / torch.sigmoid at onssen/nn/deep_clustering.py:39-42,
 * onssen/nn/chimera.py:37-42, onssen/nn/phase_network.py:53-66, and nn.LSTM's input projection.
 *   logical row m in [0, M):  i0 = m / R, i1 = m % R
 *     A row  at  A + i0*a_s0 + i1*a_s1  (K contiguous floats)
 *     C row  at  C + i0*c_s0 + i1*c_s1  (N contiguous floats); `resid` (nullable) is laid out like C
 *   W[n][k] row-major with leading dimension ldw (multiple of 4, zero-filled beyond K), bias[N]
 *   mode L2NORM: `group` must divide 80 and N; the residual (phase head) is added before the norm.
 */
int onssen_linear_f32(const float* A, int64_t a_s0, int64_t a_s1, int R, int M, int K, const float* W, int ldw,
                      const float* bias, int N, int mode, int group, float eps, const float* resid, float* C,
                      int64_t c_s0, int64_t c_s1, void* stream);

/* Split-bf16 form of onssen_linear_f32: every fp32 product is a_hi*b_hi + a_hi*b_lo + a_lo*b_hi on the bf16
 * MFMA pipe with fp32 accumulation (~1e-5 relative on a dot product; measured 1e-6 abs on the network
 * outputs).  A is plain fp32 and split on the fly; the weights are pre-split by onssen_linear_pack_bf16x3 into
 * `w_planes` = [N][ldw] bf16 hi plane followed by the [N][ldw] lo plane, ldw a multiple of 32 (zero beyond K).
 * Same row maps, epilogues and argument meaning as onssen_linear_f32; L2NORM `group` must divide 160.
 */
int onssen_linear_pack_bf16x3(const float* w, int N, int K, int ld_in, int ld_out, uint16_t* w_planes, void* stream);
int onssen_linear_bf16x3(const float* A, int64_t a_s0, int64_t a_s1, int R, int M, int K, const uint16_t* w_planes,
                         int ldw, const float* bias, int N, int mode, int group, float eps, const float* resid,
                         float* C, int64_t c_s0, int64_t c_s1, void* stream);

/* `batch` independent problems C_z = A_z W_z^T + bias of one shape in ONE launch (gridDim.z): A_z = a_img + z*a_bs,
 * W_z = w_img + z*w_bs (uint16 elements, multiples of 8), C_z = C + z*c_bs with row stride ldc; the bias is shared.
 * Used by the training path: the two directions' weight-gradient GEMMs fill the chip only together. */
int onssen_linear_x3p_batched(const uint16_t* a_img, int64_t a_bs, int M, int K, const uint16_t* w_img, int64_t w_bs,
                              const float* bias, int N, float* C, int64_t c_bs, int64_t ldc, int batch, void* stream);
/* The same with row map and TWO dense outputs: row m of problem z goes to C + z*c_bs + (m / R)*c_s0 + (m % R)*c_s1 for the
 * columns n < n_split and to C2 + z*c2_bs + (m / R)*c2_s0 + (m % R)*c2_s1 (column n - n_split) for the rest.  The training
 * path uses it to write [dW_ih | dW_hh] of both directions straight into nn.LSTM's row order (packed row 4u + gate ->
 * row gate*H + u: R = 4, c_s0 = ld, c_s1 = H*ld) and into two contiguous matrices: no gather, no strided copies. */
int onssen_linear_x3p_batched_split(const uint16_t* a_img, int64_t a_bs, int M, int K, const uint16_t* w_img, int64_t w_bs,
                                    const float* bias, int N, int R, float* C, int64_t c_bs, int64_t c_s0, int64_t c_s1,
                                    int n_split, float* C2, int64_t c2_bs, int64_t c2_s0, int64_t c2_s1, int batch, void* stream);
/* ... with the roles of the two outputs alternating: even problems as above, ODD problems write their columns n < n_split_odd
 * to C2 (+ z*c2_bs, column n) and the rest to C (+ z*c_bs, column n - n_split_odd).  With w_bs smaller than a problem's N rows the
 * problems' W windows overlap: the training path lays out [h_prev forward | x | h_prev reverse] (Hp | Kx | Hp image rows),
 * w_bs = Hp rows -- problem 0 reads [h_f | x], problem 1 [x | h_r], and the layer input's transposed image exists once. */
int onssen_linear_x3p_batched_split_alt(const uint16_t* a_img, int64_t a_bs, int M, int K, const uint16_t* w_img, int64_t w_bs,
                                        const float* bias, int N, int R, float* C, int64_t c_bs, int64_t c_s0, int64_t c_s1,
                                        int n_split, float* C2, int64_t c2_bs, int64_t c2_s0, int64_t c2_s1, int n_split_odd,
                                        int batch, void* stream);

/* The weight gradients of one bidirectional LSTM layer from ROW-MAJOR x3 images, as the kernels that produced them left them --
 * no transposed image is made (round 4; gfx950's transposing LDS read delivers the MFMA fragments):
 *   dp_img [K = T*B][2*NP / 32][2][32]  dL/d(pre-activation), columns direction*NP + packed gate column
 *   y_img  [K][ceil(2*Hp / 32)][2][32]   the layer's output (onssen_blstm_y_image),   x_img [K][ceil(Kx / 32)][2][32]  its input
 *   dW_hh[d] = dP_d^T h_prev_d (h_prev = y rows k - B for the forward, k + B for the reverse direction),  dW_ih[d] = dP_d^T x,
 *   direction d at dW_* + d*bs, packed row m at (m / R)*s0 + (m % R)*s1 (R = 4, s0 = ld, s1 = H*ld writes nn.LSTM's row order).
 * NP % 32 == 0, Hp % 8 == 0 (x_img's zero padding past Kx is read up to the next multiple of 8, never stored).  zero16: 16 readable zero bytes.  Bit-identical to
 * onssen_linear_x3p_batched_split_alt on the transposed images. */
int onssen_lstm_wgrad_images_f32(const uint16_t* dp_img, const uint16_t* y_img, const uint16_t* x_img, int K, int B, int NP, int Hp,
                                 int Kx, const float* zero16, int R, float* dW_ih, int64_t ih_bs, int64_t ih_s0, int64_t ih_s1,
                                 float* dW_hh, int64_t hh_bs, int64_t hh_s0, int64_t hh_s1, void* stream);
/* The same kernel for one plain weight gradient: C [M][N] (row stride ldc) = A^T W, contraction over the K rows of the row-major
 * x3 images A [K][ceil(M/32)][2][32] and W [K][ceil(N/32)][2][32] (their zero padding past M / N is read, never stored). */
int onssen_linear_x3t(const uint16_t* a_img, const uint16_t* w_img, int K, int M, int N, const float* zero16, float* C, int64_t ldc,
                      void* stream);

/* x3 image of the TRANSPOSE of a row-major fp32 matrix src [K][ld >= M], optionally shifted along k: image row m
 * (0 <= m < M), element k (0 <= k < K) = src[(k + k_shift) * ld + m], 0 where k + k_shift is outside [0, K).  Operands of
 * the training path's weight-gradient GEMMs (contraction over the T*B rows of row-major activations; k_shift = -+B turns
 * the layer output into "h of the step before" for the forward / reverse direction). */
int onssen_x3_image_t_f32(const float* src, int64_t ld, int M, int K, int k_shift, uint16_t* img, void* stream);
/* Both images of a row-major [K][M] matrix (leading dimension ld) in one pass: img_rows = its x3 image [K][ceil(M/32)][2][32]
 * (what onssen_x3_image_f32 gives), img_t = the image of its transpose [M][ceil(K/32)][2][32] (onssen_x3_image_t_f32 with
 * k_shift 0).  The training path's dP feeds the input-gradient GEMM as the first and the weight-gradient GEMM as the second. */
int onssen_x3_image_both_f32(const float* src, int64_t ld, int M, int K, uint16_t* img_rows, uint16_t* img_t, void* stream);
/* ... also leaving colsum [ceil(K/32)][M]: the column sums of every 32-row block of src -- their sum over the blocks is the
 * column sum of src (the bias gradient of the layer whose output gradient src is) without another pass over it. */
int onssen_x3_image_both_colsum_f32(const float* src, int64_t ld, int M, int K, uint16_t* img_rows, uint16_t* img_t, float* colsum,
                                    void* stream);

/* Split-bf16 GEMM over PRE-SPLIT operands.  An "x3 image" of a row-major [rows][K] fp32 matrix is
 * [rows][KB][2][32] bf16, KB = ceil(K/32): per row and 32-wide k block, 32 x hi = bf16(x) then 32 x lo =
 * bf16(x - hi), zeros beyond K (16-byte aligned).  onssen_x3_image_f32 builds one from fp32 rows (row m at
 * src + (m / R)*s0 + (m % R)*s1); the BLSTM's split-bf16 recurrence writes its output in this form as well.
 *   C row m at C + (m / R)*c_s0 + (m % R)*c_s1 = epilogue(a_img[m] . w_img[n] + bias[n]), n < N
 *   mode BIAS | SIGMOID | L2NORM (group in {20, 40, 80}: multiple of 4 dividing 80, N % group == 0; no residual).
 * Same arithmetic as onssen_linear_bf16x3 (three bf16 MFMAs per product, fp32 accumulate); ~2x its speed because
 * staging is a plain copy and the epilogue stays in registers.
 */
int onssen_x3_image_f32(const float* src, int64_t s0, int64_t s1, int R, int rows, int K, uint16_t* img, void* stream);
int onssen_linear_x3p(const uint16_t* a_img, int M, int K, const uint16_t* w_img, const float* bias, int N, int mode,
                      int group, float eps, float* C, int R, int64_t c_s0, int64_t c_s1, void* stream);
/* TWO heads over the same activations in one launch (onssen/nn/chimera.py:37-45: fc_dc + F.normalize and fc_mi + sigmoid
 * both read the BLSTM output): w_img / bias hold the N rows of both layers, rows [0, n_split) are normalised over `group`
 * consecutive outputs (a multiple of 4 dividing 80; n_split % group == 0) and go to C, rows [n_split, N) pass through the
 * logistic and go to columns n - n_split of C2 (row m at C2 + (m / R)*c2_s0 + (m % R)*c2_s1).  The embedding's last
 * 320-column tile is mostly padding (2 580 = 8 x 320 + 20): the second head's columns fill it, its own launch disappears. */
int onssen_linear_x3p_pair(const uint16_t* a_img, int M, int K, const uint16_t* w_img, const float* bias, int N, int n_split,
                           int group, float eps, float* C, int R, int64_t c_s0, int64_t c_s1, float* C2, int64_t c2_s0,
                           int64_t c2_s1, int bf16_only, void* stream);
/* The embedding head of a TRAINING forward (onssen/nn/deep_clustering.py:39-41: fc_dc, then F.normalize over each bin's D
 * features): C [M][N] = the normalised rows as with ONSSEN_EPI_L2NORM, and inv_norm [M][N / group] = 1 / max(||x||, eps) of
 * every group (group a multiple of 4 dividing 80).  With the two, the backward of the normalisation needs no raw product
 * (onssen_l2norm_rows_grad_y_f32): the 4 M N bytes of x are neither written nor read back, and the separate normalisation
 * pass of the forward disappears. */
int onssen_linear_x3p_norms(const uint16_t* a_img, int M, int K, const uint16_t* w_img, const float* bias, int N, int group,
                            float eps, float* C, float* inv_norm, void* stream);

/* The same GEMM with phase_net's head epilogue (onssen/nn/phase_network.py:58-66: fc_phase(bn(rnn)) + mix phase, then
 * F.normalize over (re, im)): C = normalise_group(a_img . w_img^T + bias + resid), group = 2 (pairs of consecutive
 * outputs, N even) or a multiple of 4 dividing 80.  resid has C's row addressing with the row-in-block index taken
 * modulo resid_mod: row m reads resid + (m / R)*c_s0 + ((m % R) % resid_mod)*c_s1 -- both speakers of the phase network
 * (batch rows b and b + B of the shared phase BLSTM) add the SAME mixture phase, so one launch serves both.
 * bf16_only != 0: plain bf16 products (ONSSEN_EPI_BF16). */
int onssen_linear_x3p_resid(const uint16_t* a_img, int M, int K, const uint16_t* w_img, const float* bias, int N, int group,
                            float eps, const float* resid, int resid_mod, float* C, int R, int64_t c_s0, int64_t c_s1,
                            int bf16_only, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K3+K4  stacked bidirectional LSTM, eval semantics (zero initial state, no dropout).
 * Replaces `rnn_output, hidden = self.rnn(x)` (onssen/nn/deep_clustering.py:35, chimera.py:35,
 * phase_network.py:48,55).
 *   x         element (b, t, k) at x + b*xs_b + t*xs_t + k, k < in_dim
 *   wih_p_host / whh_p_host / bias_p_host: HOST arrays of L device pointers; entry l holds both
 *             directions back to back: wih [2*NP][Kp_l], whh [2][whh_elems], bias [2*NP]
 *   y         (T, B, 2*Hp) time-major output of the last layer: [fwd(Hp) | rev(Hp)], padded units are 0.  May be
 *             NULL in the ONSSEN_BLSTM_XCD form when the caller only consumes the x3 image (onssen_blstm_y_image):
 *             the recurrence then skips its fp32 stores.
 *   ws        workspace of onssen_blstm_workspace_bytes() bytes, 256-byte aligned, ZEROED ONCE by its owner when
 *             it is allocated and never again.  Its first ONSSEN_BLSTM_WS_HEADER_BYTES hold the exchange state
 *             of the ONSSEN_BLSTM_XCD form (flags, generations, status words): everything in there is monotonic,
 *             and no call memsets it (so a hipGraph replay does not depend on a memset node reaching the kernel's
 *             L2); the k padding of the x3 images further back is never written and must read as zero (the h hand-off
 *             area needs nothing: the ONSSEN_BLSTM_XCD kernels clear their slots at start-up, the launch-per-step form
 *             memsets it).  u32 word
 *             [280] != 0: a launch gave up waiting (outputs invalid); word [281] = 1: some launch used the
 *             placement-independent accesses; word [282] = 1: a non-finite activation was replaced by 0 (see
 *             ONSSEN_BLSTM_XCD).  The host resets [280] and [282] after reporting them.
 * Default form: one input-projection GEMM + T recurrence launches per layer; capture the call in a hipGraph
 * to amortise launch cost.  ONSSEN_BLSTM_XCD: one GEMM + ONE persistent launch per layer (DESIGN.md,
 * "XCD-local persistent recurrence").
 */
#define ONSSEN_BLSTM_WS_HEADER_BYTES 32768
size_t onssen_blstm_workspace_bytes(int B, int T, int in_dim, int H, int L, int ug);
/* Where the ONSSEN_BLSTM_XCD form leaves the x3 image [T*B][KB][2][32] (row m = t*B + b, KB = ceil(2*Hp/32),
 * k = d*Hp + j) of the LAST layer's output: byte offset inside the workspace.  Feed it to onssen_linear_x3p. */
int onssen_blstm_y_image(int B, int T, int in_dim, int H, int L, int ug, size_t* offset_bytes, int* KB);
/* ... and the x3 image [T*B][ceil(in_dim/32)][2][32] of the stack's INPUT (row m = t*B + b), made by the XCD form for its first
 * projection GEMM (not with ONSSEN_BLSTM_FUSE_IN0): the training path's weight-gradient GEMM over row-major images reads it back. */
int onssen_blstm_x_image(int B, int T, int in_dim, int H, int L, int ug, size_t* offset_bytes, int* KB);
int onssen_blstm_forward_f32(const float* x, int64_t xs_b, int64_t xs_t, int B, int T, int in_dim, int H, int L,
                             int ug, const float* const* wih_p_host, const float* const* whh_p_host,
                             const float* const* bias_p_host, float* y, void* ws, size_t ws_bytes, int flags,
                             void* stream);

/* ---- Two-layer stack, SOFTWARE-PIPELINED over consecutive calls (round 6) -----------------------------------------------
 * The same `self.rnn(x)` (onssen/nn/deep_clustering.py:35) for num_layers = 2 and B <= 32, arranged for THROUGHPUT over a stream
 * of batches (the evaluation loop of onssen/utils/test.py:29-41 hands over one batch after the other): a B <= 32 layer fills the
 * chip's 8 XCDs only with 8-row groups, whose time step costs what a 16-row group's does bar the MFMAs (1.42 vs 1.88 us at
 * H = 600) -- so call n runs layer 1 of batch n-1 and layer 0 of batch n in ONE persistent launch, 16-row groups (stacked 8-row
 * groups up to B = 16), each layer on its own half of the XCDs:
 *     x3 image + input projection of x (batch n)  ->  [ layer 1 (batch n-1)  ||  layer 0 (batch n) ]  ->  layer 1's input
 *     projection of batch n (kept in ws for call n+1).
 * After call n the x3 image [T*B][KB][2][32] of layer 1's output FOR BATCH n-1 is at onssen_blstm_pipe2_y_image (feed it to
 * onssen_linear_x3p*); call 0's image is the stack's answer to an all-zero layer-1 input projection (finite, meaningless), and one
 * extra call (any x) drains the last batch.  Per batch the results are bit for bit those of onssen_blstm_forward_f32 on 16-row
 * groups without ONSSEN_BLSTM_FUSE_IN0 (e.g. the same rows inside a B = 64 call); against the default B = 32 call (stacked 8-row
 * groups, which add the lo x lo products) they differ in the last bits, inside the same tolerance.
 *   flags: ONSSEN_BLSTM_BF16X3 | ONSSEN_BLSTM_XCD exactly (the plain split-bf16 persistent recurrence), H <= 640; plus, as a
 *   measurement aid, ONSSEN_BLSTM_G_READY: only the persistent launch, on the projections an earlier call left in ws.
 *   wih_p_host / whh_p_host / bias_p_host: HOST arrays of 2 device pointers as for onssen_blstm_forward_f32 in that form (x3 image
 *   of the packed projection, the two directions' onssen_lstm_pack_whh_bf16x3 images, packed bias).
 *   ws: onssen_blstm_pipe2_workspace_bytes() bytes, 256-byte aligned, ZEROED ONCE by its owner; header words as above. */
size_t onssen_blstm_pipe2_workspace_bytes(int B, int T, int in_dim, int H, int ug);
int onssen_blstm_pipe2_y_image(int B, int T, int in_dim, int H, int ug, size_t* offset_bytes, int* KB);
int onssen_blstm_pipe2_forward_f32(const float* x, int64_t xs_b, int64_t xs_t, int B, int T, int in_dim, int H, int ug,
                                   const float* const* wih_p_host, const float* const* whh_p_host,
                                   const float* const* bias_p_host, void* ws, size_t ws_bytes, int flags, void* stream);
/* ... that ALSO builds the deep-clustering target map of batch n (x is its log-magnitude, dense [B][T][in_dim]: xs_t = in_dim,
 * xs_b = T * in_dim): what onssen_dc_index_f32(x, B, T, NULL, in_dim, D, db_threshold, map_ws, map_ws_bytes) leaves in map_ws, byte
 * for byte, built by min(16, B) extra workgroups at the end of the persistent launch's grid -- on the CUs its members leave free --
 * instead of three launches in front of it.  map_ws is validated as onssen_dc_index_f32 validates its workspace; everything else
 * is onssen_blstm_pipe2_forward_f32 (ONSSEN_BLSTM_G_READY included: the launch alone still builds the map).  The map is complete
 * when the call's launches are, whether or not the recurrence gave up a wait. */
int onssen_blstm_pipe2_map_forward_f32(const float* x, int64_t xs_b, int64_t xs_t, int B, int T, int in_dim, int H, int ug,
                                       const float* const* wih_p_host, const float* const* whh_p_host,
                                       const float* const* bias_p_host, void* ws, size_t ws_bytes, int flags, float db_threshold, int D,
                                       void* map_ws, size_t map_ws_bytes, void* stream);
/* ... over a stream of RAGGED batches of whole utterances (round 6c; the reference evaluates them one by one, onssen/utils/test.py:29-41;
 * onssen_blstm_forward_ragged_f32 runs K of different lengths per call): batch n is B <= 16 rows padded to ITS longest utterance,
 * T frames, row b live for frames[b] <= T of them; the launch's other half still works on batch n-1 (T_prev, frames_prev -- the
 * values that call n-1 was given; call 0: any valid pair, e.g. this call's own).  The workspace is laid out for T_cap >= every T
 * of the stream (onssen_blstm_pipe2_workspace_bytes / _y_image with T = T_cap); the image of batch n-1 holds T_prev * B rows, zeros
 * at t >= frames_prev[b].  Every row's outputs at its own frames are bit for bit those of onssen_blstm_forward_ragged_f32 (i.e. of
 * its own batch-1 run): stacked tiles in both. */
int onssen_blstm_pipe2_forward_ragged_f32(const float* x, int64_t xs_b, int64_t xs_t, int B, int T_cap, int T, const int32_t* frames,
                                          int T_prev, const int32_t* frames_prev, int in_dim, int H, int ug,
                                          const float* const* wih_p_host, const float* const* whh_p_host,
                                          const float* const* bias_p_host, void* ws, size_t ws_bytes, int flags, void* stream);

/* ---- Training: nn.LSTM forward with saved state and its backward recurrence ------------------
 * What `loss.backward()` does for `self.rnn` (onssen/utils/train.py:80-84; nn.LSTM autograd), one layer at a time so that
 * the caller can apply the inter-layer dropout (nn.LSTM(dropout=0.3), onssen/nn/deep_clustering.py:15-22) in between.
 *
 * onssen_lstm_train_forward_f32: one bidirectional layer in the ONSSEN_BLSTM_XCD | ONSSEN_BLSTM_BF16X3 form (same
 *   operands as onssen_blstm_forward_f32 with L = 1: wih_img = x3 image of the packed [2*NP][in_dim] projection,
 *   whh_x3 = the two directions' onssen_lstm_pack_whh_bf16x3 images, bias_p [2*NP]; ws as for L = 1).  Besides
 *   y [T][B][2][Hp] it leaves gates [T][B][2][NP] = the activations (i, f, g, o) of every unit in the packed column
 *   layout of G (column = ugi*4*ug + ju*4 + gate) and cs [T][B][2][Hp] = the cell states c_t.  H <= 768 (ug = 24 above 640).
 * onssen_lstm_train_backward_f32: given dy [T][B][2][Hp] = dL/dy (padded units 0), overwrites `gates_dp` in place with
 *   dL/d(pre-activation) (same layout) -- the operand of the weight / input gradient GEMMs:
 *     dW_ih(packed) = dP^T x,  dW_hh(packed, per direction) = dP_d^T h_prev,  db = sum_rows dP,  dx = dP W_ih(packed).
 *   form ONSSEN_LSTM_BWD_XCD (default of the Python layer; H <= 640): ONE persistent launch per layer, every (direction, row
 *     group) inside one XCD like the forward; each member keeps the rows of W_hh of its own gate columns in registers,
 *     multiplies them with the dP it has just produced and the members reduce-scatter fp32 partial sums of dh through
 *     the XCD's L2.  whh_img = the two directions' onssen_lstm_pack_whhR_bf16x3 images (onssen_lstm_whhR_elems uint16
 *     each).  ws: zeroed ONCE by its owner (header words [280] / [281] report aborts / the placement-independent
 *     protocol exactly as in onssen_blstm_forward_f32).
 *   form ONSSEN_LSTM_BWD_STEPS: one launch per time step (T launches); whh_img = onssen_lstm_pack_whhT_bf16x3 images
 *     (onssen_lstm_whhT_elems).  No requirements on ws contents.
 *   Split-bf16 products, fp32 accumulation and state in both forms.
 *   db_rows (ONSSEN_LSTM_BWD_XCD only, may be NULL): [B][2][NP], receives sum_t dP[t][b] per batch row -- the kernel has every
 *   dP in registers as it goes; the bias gradient is the sum of its B rows instead of a pass over all T*B rows of dP. */
/* onssen_lstm_train_backward_img_f32 (round 5): the ONSSEN_LSTM_BWD_XCD form that leaves dP as the x3 image
 *   dp_img [T*B][2*NP/32][2][32] (row m = t*B + b, column k = d*NP + packed gate column; onssen_x3_image_f32's layout, bit for bit
 *   what it makes of the fp32 dP) INSTEAD of overwriting the gates: the gradient GEMMs read that image, the fp32 -> image pass over
 *   all of dP disappears.  `gates` is only read (padded rows / columns of dp_img that no unit owns are NOT written: 2*NP % 32 == 0
 *   and Hp == H give an image without such holes; otherwise zero it first). */
#define ONSSEN_LSTM_BWD_STEPS 0
#define ONSSEN_LSTM_BWD_XCD 1
int onssen_lstm_train_forward_f32(const float* x, int64_t x_stride_b, int64_t x_stride_t, int B, int T, int in_dim, int H,
                                  int ug, const uint16_t* wih_img, const uint16_t* whh_x3, const float* bias_p, float* y,
                                  float* gates, float* cs, void* ws, size_t ws_bytes, void* stream);
int onssen_lstm_train_backward_img_f32(int B, int T, int H, int ug, const uint16_t* whh_img, const float* dy, const float* gates,
                                       const float* cs, void* ws, size_t ws_bytes, float* db_rows, uint16_t* dp_img, void* stream);
/* The same training forward in a chosen FORM of onssen_blstm_forward_f32 (round 4: the training path no longer leaves the
 * library when the persistent launch cannot be used -- the re-run of a step whose persistent launch aborted, H > 640):
 *   flags = ONSSEN_BLSTM_XCD | ONSSEN_BLSTM_BF16X3   the persistent launch (= onssen_lstm_train_forward_f32; wih = x3 image,
 *                                                    whh = onssen_lstm_pack_whh_bf16x3 images)
 *   flags = ONSSEN_BLSTM_BF16X3                      one launch per time step, split-bf16 (wih = onssen_linear_pack_bf16x3
 *                                                    planes, whh as above; H <= 640)
 *   flags = 0                                        one launch per time step, exact fp32 (wih / whh = onssen_lstm_pack_f32
 *                                                    arrays; any H)
 * gates / cs as above; pair it with onssen_lstm_train_backward_f32 (either form: both read the same saved state). */
int onssen_lstm_train_forward_form_f32(const float* x, int64_t x_stride_b, int64_t x_stride_t, int B, int T, int in_dim, int H,
                                       int ug, const void* wih, const void* whh, const float* bias_p, float* y, float* gates,
                                       float* cs, void* ws, size_t ws_bytes, int flags, void* stream);
int64_t onssen_lstm_whhT_elems(int H, int ug);
int onssen_lstm_pack_whhT_bf16x3(const float* w_hh, int H, int ug, uint16_t* out, void* stream);
int64_t onssen_lstm_whhR_elems(int H, int ug);
int onssen_lstm_pack_whhR_bf16x3(const float* w_hh, int H, int ug, uint16_t* out, void* stream);
size_t onssen_lstm_train_backward_workspace_bytes(int B, int H, int ug, int form);
int onssen_lstm_train_backward_f32(int B, int T, int H, int ug, const uint16_t* whh_img, const float* dy, float* gates_dp,
                                   const float* cs, void* ws, size_t ws_bytes, int form, float* db_rows, void* stream);
/* The inter-layer dropout of nn.LSTM(dropout=p) (onssen/nn/deep_clustering.py:15-22) as ONE pass:
 *   out[i] = keep(seed, i) ? x[i] / (1 - p) : 0,   keep = counter-based hash of (seed, i) compared with p
 * -- no mask tensor: the backward pass calls it again on dL/d(out) with the same seed.  Like the reference's (the RNN
 * library's own generator) the random stream is not torch's; the caller draws `seed` from torch's generator, so runs
 * repeat under torch.manual_seed.  0 <= p < 1; out may alias x; n elements, 16-byte aligned when n % 4 == 0. */
int onssen_dropout_f32(const float* x, int64_t n, float p, uint64_t seed, float* out, void* stream);
/* (round 5) Gradient-norm clipping + Adam over n parameter tensors in two passes (onssen/utils/train.py:83-84:
 * `clip_grad_norm_(model.parameters(), 5)` then `optimizer.step()`; Adam without weight decay / amsgrad, torch.optim.Adam's
 * formulas):  coef = min(1, max_norm / (||g|| + 1e-6)), g' = coef g, m += (g' - m)(1 - beta1), v = beta2 v + (1 - beta2) g'^2,
 * p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps).  The scaled gradient is not written back unless
 * write_grads != 0.  max_norm <= 0 or +inf: no clipping (one pass, ws may be NULL).  *_host: HOST arrays of n DEVICE pointers /
 * element counts; step >= 1 is the step being taken; lr / betas / eps are doubles (rounded once, after 1 - beta is formed).  ws: onssen_clip_adam_workspace_bytes() bytes, 16-byte aligned; after the
 * call ws[0] (float) holds ||g|| before clipping (clip_grad_norm_'s return value). */
size_t onssen_clip_adam_workspace_bytes(const int64_t* numel_host, int n);
int onssen_clip_adam_f32(int n, float* const* p_host, float* const* g_host, float* const* m_host, float* const* v_host,
                         const int64_t* numel_host, float max_norm, double lr, double beta1, double beta2, double eps, int step,
                         int write_grads, void* ws, size_t ws_bytes, void* stream);
/* F.normalize(x, p=2, dim=-1, eps) over `rows` rows of D floats and its backward -- the embedding's unit norm per TF bin in a
 * TRAINING forward (onssen/nn/deep_clustering.py:40-41; inference normalises in the GEMM epilogue):
 *   y = x / max(||x||, eps);   dx = (g - y (y . g)) / ||x||  where ||x|| > eps,  g / eps  elsewhere.   D % 4 == 0, D <= 64. */
int onssen_l2norm_rows_f32(const float* x, int64_t rows, int D, float eps, float* y, void* stream);
/* Train-mode BatchNorm1d over the rows of a row-major (M, C) matrix (onssen/nn/deep_clustering.py:12,36-38: per channel, over all
 * B*T frames of the batch): y = (x - mean) * invstd * gamma + beta with the batch's biased variance, mean / invstd returned
 * for the backward pass (the caller updates running_mean / running_var from mean and 1 / invstd^2 - eps, unbiased by
 * M / (M - 1), as nn.BatchNorm1d does); and its backward: dbeta = sum dy, dgamma = sum dy * xhat,
 * dx = gamma * invstd * (dy - dbeta / M - xhat * dgamma / M).  Column sums are partial sums of 32-row strips added in a
 * fixed order (deterministic).  ws: onssen_bn_rows_workspace_bytes(M, C). */
size_t onssen_bn_rows_workspace_bytes(int64_t M, int C);
int onssen_bn_rows_train_f32(const float* x, int64_t M, int C, const float* gamma, const float* beta, float eps, float* y,
                             float* mean, float* invstd, void* ws, size_t ws_bytes, void* stream);
int onssen_bn_rows_grad_f32(const float* x, const float* dy, int64_t M, int C, const float* gamma, const float* mean,
                            const float* invstd, float* dx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream);
int onssen_l2norm_rows_grad_f32(const float* x, const float* g, int64_t rows, int D, float eps, float* dx, void* stream);
/* ... from the normalisation's output y and inv_norm = 1 / max(||x||, eps) per row (what onssen_linear_x3p_norms leaves):
 * dx = (g - y (y . g)) * inv_norm where the norm was not clamped, g * inv_norm otherwise. */
int onssen_l2norm_rows_grad_y_f32(const float* y, const float* inv_norm, const float* g, int64_t rows, int D, float eps, float* dx,
                                  void* stream);

/* ---------------------------------------------------------------------------------------------
 * K11 glue  recurrent input of the phase network for all C speakers at once:
 *   out[(s*B + b), t, :] = cat(x_mag[b,t,:] * mask[b,s,t,:], x_phase[b,t,:,:].view(2F))      (C*B, T, 3F)
 * Replaces `mag_A = x_mag * mask_A; input_A = torch.cat((mag_A, x_phase.view(B,T,-1)), 2)` (and _B) at
 * onssen/nn/phase_network.py:45-47,54.  mask element (b,s,t,f) at mask + b*m_sb + s*m_sc + t*m_st + f*m_sf.
 */
int onssen_phase_input_f32(const float* x_mag, const float* mask, int64_t m_sb, int64_t m_sc, int64_t m_st,
                           int64_t m_sf, const float* x_phase, int B, int C, int T, int F, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * N3  training-label features of a chunk from the complex STFTs of mixture and sources ((B,T,F,2) float32 each,
 * as written by onssen_stft_logmag_f32) and the mixture's log-magnitude (B,T,F).
 * Replaces get_one_hot / get_cos_difference / np.abs in onssen/data/feature_utils.py:77-95 and
 * onssen/data/wsj0_2mix.py:130-152:
 *   one_hot (B,T,F,2) float32: e_argmax(|s1|,|s2|) (speaker 0 on ties), all-zero where
 *           feature < max_over_the_chunk(feature) - db_threshold/20;   utt_max (B) scratch
 *   mag_mix, mag_s1, mag_s2 (B,T,F);  cos_s1, cos_s2 (B,T,F) = cos(angle(mix) - angle(s)), both NULL to skip
 */
int onssen_labels_f32(const float* stft_mix, const float* stft_s1, const float* stft_s2, const float* feature_mix, int B,
                      int T, int F, float db_threshold, float* utt_max, float* one_hot, float* mag_mix, float* mag_s1,
                      float* mag_s2, float* cos_s1, float* cos_s2, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Weight guard: do packed weight images still belong to the live parameters?  `ptrs` / `numel` are DEVICE arrays of n parameter
 * tensors (float32, any 4-byte type) and their element counts.  mode 0: ref[t] = a 32-bit fold of a strided sample (<= `samples`
 * elements, first and last included) of tensor t -- call when the images are built; mode 1: the same fold compared with ref[t],
 * `*flag |= 1` on a difference (sticky; the caller reads and clears it asynchronously).  One launch of n small workgroups,
 * stream-ordered, capturable.  Nothing in the reference corresponds to it: there a module's weights ARE its parameters
 * (onssen/utils/test.py:21-35 loads a checkpoint and runs); here it keeps a cached re-layout honest against updates that bypass
 * autograd's version counter (fused optimizers, p.data arithmetic).
 */
int onssen_param_guard_u32(const void* const* ptrs, const int64_t* numel, int n, int samples, int mode, uint32_t* ref, uint32_t* flag,
                           void* stream);

/* ---------------------------------------------------------------------------------------------
 * The reference's stand-alone feature helpers on ONE utterance's arrays (onssen_amd/data/feature_utils.py binds them under
 * the reference's names).  `stft*` are complex arrays as interleaved (re, im) float32 pairs, `n` complex elements.
 *   onssen_log_magnitude_f32   out[e] = log10f(|stft[e]| + epsilon)           get_log_magnitude, onssen/data/feature_utils.py:49-51
 *   onssen_cos_difference_f32  out[e] = cos(angle(stft_1[e]) - angle(stft_2[e]))   get_cos_difference, feature_utils.py:77-80
 *   onssen_one_hot_f32         one_hot (B, per_utt, 2) float32 from B utterances of per_utt bins each: e_argmax(mag_s1, mag_s2)
 *                              (speaker 0 on ties), all-zero where feature < max_over_the_utterance(feature) - db_threshold/20;
 *                              utt_max (B) scratch                             get_one_hot, feature_utils.py:83-95
 */
int onssen_log_magnitude_f32(const float* stft_ri, int64_t n, float epsilon, float* out, void* stream);
int onssen_cos_difference_f32(const float* stft_1, const float* stft_2, int64_t n, float* out, void* stream);
int onssen_one_hot_f32(const float* feature_mix, const float* mag_s1, const float* mag_s2, int B, int64_t per_utt,
                       float db_threshold, float* utt_max, float* one_hot, void* stream);

/* ---------------------------------------------------------------------------------------------
 * N2  deep-clustering back end: per utterance, 2-means over the D-dimensional embeddings of the bins with
 * feature >= max(feature) - db_threshold/20, then binary masks (B,T,F,2): mask[...,0] = label, mask[...,1] =
 * 1 - label on active bins, 0 in both on silent bins.
 * Replaces `KMeans(n_clusters=2, random_state=0).fit_predict(emb)` + the mask fill at
 * egs/wsj0-2mix/deep_clustering/evaluate.py:36-41 (sklearn on the host upstream).  Deterministic farthest-point
 * initialisation and at most `iters` Lloyd iterations; an utterance stops earlier when its assignment reaches its exact
 * fixed point or -- sklearn's own rule, KMeans(tol=1e-4) being the reference's default -- when the summed squared shift of
 * the two centroids is <= tol x the mean per-feature variance of the clustered rows (tol = 0: the fixed point only).  The
 * rows are unit vectors (F.normalize, onssen/nn/deep_clustering.py:41): that variance is taken as (1 - |mean|^2) / D.
 * Cluster numbering is arbitrary, as it is upstream.  D <= 32.
 * Default form: the active bins are compacted once into the workspace and ALL iterations run in one persistent launch
 * (8 workgroups per utterance that meet at a counter; every wait is bounded by onssen_xcd_spin_limit: a wait that gives up
 * sets the u32 at ws + onssen_dc_cluster_status_offset(B, D) -- the masks of that call are then not the converged ones and
 * the caller repeats it with ONSSEN_DC_CLUSTER_LAUNCH_PER_ITERATION).  flags = ONSSEN_DC_CLUSTER_LAUNCH_PER_ITERATION: two
 * launches per iteration over the uncompacted embeddings, no inter-workgroup waits.  The owner zeroes the status word once.
 * emb 16-byte aligned, ws 256-byte aligned.
 */
#define ONSSEN_DC_CLUSTER_LAUNCH_PER_ITERATION 1
size_t onssen_dc_cluster_workspace_bytes(int B, int T, int F, int D);
size_t onssen_dc_cluster_status_offset(int B, int D);
int onssen_dc_cluster_f32(const float* emb, const float* feature, int B, int T, int F, int D, float db_threshold,
                          int iters, float tol, float* masks, void* ws, size_t ws_bytes, int flags, void* stream);

/* ---------------------------------------------------------------------------------------------
 * N1  deep-clustering loss: VALUE (onssen_loss_dc_f32) and its GRADIENT w.r.t. the embedding (onssen_loss_dc_grad_f32):
 *   per_utt[b] = ||V^T V||_F - 2 ||V^T Y||_F + ||Y^T Y||_F,  V = w * (sum_c Y) * emb, Y = w * one_hot,
 *   w_r = sqrt(mag_r / total_mag[b]),  total_mag[b] = sum_r mag_r            (Frobenius NORMS, as upstream)
 * Replaces onssen/loss/loss_dc.py:24-43 + loss_util.py:4-11; the caller forms upstream's (B,B) product
 * per_utt[None,:] * total_mag[:,None] (loss_dc.py:44) and its mean (utils/train.py:78-79).
 *   emb (B, TF, D), one_hot (B, TF, C) as float, mag (B, TF); D + C <= 34.
 */
/* Mask-inference term of the chimera losses: out[b] = min over the two speaker assignments of
 *   sum |mask_x * mag_mix - t_1| + sum |mask_y * mag_mix - t_2|,  t_s = mag_s (MSA: cos_* = NULL) or
 *   min(mag_mix, relu(mag_s * cos_s)) (PSA).  Replaces onssen/loss/loss_chimera.py:25-29 and :53-57.
 *   mask element (b, e) at mask_* + b*m_sb + e*m_se (the strided views of the (B,T,F,2) mask buffer); maps (B, TF).
 *   perm_out (B) int32 or NULL: the assignment that won (0: A->1, B->2; 1: A->2, B->1; ties -> 0) -- what the gradient follows.
 * onssen_loss_mask_grad_f32: d out[b] / d mask_{A,B} times the incoming gradient g[b], one pass over the maps:
 *   d_mask_A[b,e] = g[b] * mag_mix * sign(mask_A * mag_mix - t_A)  (sign(0) = 0, like torch.abs' backward), t_A the target
 *   `perm` gives speaker A; written at d_mask_* + b*d_sb + e*d_se (e.g. the two planes of one interleaved (B,TF,2) buffer). */
size_t onssen_loss_mask_workspace_bytes(int B);
int onssen_loss_mask_f32(const float* mask_a, const float* mask_b, int64_t m_sb, int64_t m_se, const float* mag_mix,
                         const float* mag_s1, const float* mag_s2, const float* cos_s1, const float* cos_s2, int B, int TF,
                         float* out, int32_t* perm_out, void* ws, size_t ws_bytes, void* stream);
int onssen_loss_mask_grad_f32(const float* mask_a, const float* mask_b, int64_t m_sb, int64_t m_se, const float* mag_mix,
                              const float* mag_s1, const float* mag_s2, const float* cos_s1, const float* cos_s2, int B, int TF,
                              const float* g, const int32_t* perm, float* d_mask_a, float* d_mask_b, int64_t d_sb, int64_t d_se,
                              void* stream);
/* Mask term and phase term of phase_net's training loss (onssen/loss/loss_phase.py:15-35, with its strict comparison), one
 * pass over the eleven maps.  Masks, mag_mix, mag_s* as above; phase_a, phase_b (the estimates) and phase_s1, phase_s2 (the
 * targets: raw (Re, Im) STFT values, exactly 0 in silent bins) are (B, TF, 2), contiguous and 8-byte aligned.  eps = 1e-8:
 *   l1 = sum |mA x - s1| + sum |mB x - s2|,  l2 = sum |mB x - s1| + sum |mA x - s2|,
 *   cos(p, q) = <p / max(|p|, eps), q / max(|q|, eps)>                      (F.cosine_similarity: each norm clamped)
 *   perm[b] = 0 (A->1, B->2) if and only if l1 < l2, else 1 (A->2, B->1): a tie is SWAPPED, unlike onssen_loss_mask_f32
 *   out_mask[b] = the chosen l,  out_phase[b] = -sum mag_mix (cos(pA, q_A) + cos(pB, q_B)) under the same assignment.
 * Per-bin terms in fp32, sums in fp64 in a fixed order (no atomics: bit-repeatable).  ws: caller-owned, 8-byte aligned,
 * onssen_loss_phase_workspace_bytes bytes, needs no zeroing.
 * onssen_loss_phase_grad_f32, one elementwise pass under `perm`:
 *   d_mask_A[b,e]  = g_mask[b] * mag_mix * sign(mask_A * mag_mix - s_A)     (as onssen_loss_mask_grad_f32; strided by d_sb, d_se)
 *   d_phase_A[b,e] = -g_phase[b] * mag_mix * (q^ - c p^) / N,  N = max(|p|, eps), c = <p / N, q^>, p^ = p / |p| (0 at p = 0),
 *                    q^ = q / max(|q|, eps): what autograd derives from F.cosine_similarity (the norm's value is clamped, its
 *                    derivative is not); a zero target gives 0.
 *   d_phase_* (B, TF, 2) contiguous, 8-byte aligned. */
size_t onssen_loss_phase_workspace_bytes(int B);
int onssen_loss_phase_f32(const float* mask_a, const float* mask_b, int64_t m_sb, int64_t m_se, const float* mag_mix,
                          const float* mag_s1, const float* mag_s2, const float* phase_a, const float* phase_b,
                          const float* phase_s1, const float* phase_s2, int B, int TF, float* out_mask, float* out_phase,
                          int32_t* perm, void* ws, size_t ws_bytes, void* stream);
int onssen_loss_phase_grad_f32(const float* mask_a, const float* mask_b, int64_t m_sb, int64_t m_se, const float* mag_mix,
                               const float* mag_s1, const float* mag_s2, const float* phase_a, const float* phase_b,
                               const float* phase_s1, const float* phase_s2, int B, int TF, const float* g_mask,
                               const float* g_phase, const int32_t* perm, float* d_mask_a, float* d_mask_b, int64_t d_sb,
                               int64_t d_se, float* d_phase_a, float* d_phase_b, void* stream);
/* Speech enhancement (egs/daps), csrc/enhance.inc.
 * onssen_labels_enhance_f32: the label maps of onssen/data/daps_enhance.py:104-106 in one pass over the two (n_bins, 2) spectra
 * (contiguous, 8-byte aligned): mag_noisy = hypotf(Re X, Im X), mag_clean likewise, cos_diff = cosf(atan2f(X) - atan2f(S)) -- the
 * bits of onssen_cos_difference_f32(stft_noisy, stft_clean).  cos_diff may be NULL (evaluation needs the magnitudes only);
 * stft_clean, mag_clean and cos_diff may all three be NULL (separation has the noisy spectrum only: mag_noisy alone).
 * onssen_loss_enhance_f32: onssen/loss/loss_mask.py, `mode` selecting the loss; every map (B, TF) contiguous:
 *   ONSSEN_ENHANCE_MSA  per_utt[b] = sum_bins (est - mag_clean)^2                       (mag_noisy, cos_diff unused: may be NULL)
 *   ONSSEN_ENHANCE_PSA  per_utt[b] = sum_bins |est * mag_noisy - t|,  t = min(mag_noisy, relu(mag_clean * cos_diff))   (est: the mask)
 *   total[0] = scale * sum_b per_utt[b]  (nullable; MSELoss's mean is scale = 1 / (B * TF)).
 * Per-bin terms in fp32 (the PSA residual is one fused multiply-add), sums in fp64 in a fixed order (no atomics:
 * bit-repeatable).  ws: caller-owned, 8-byte aligned, onssen_loss_enhance_workspace_bytes(B) bytes, needs no zeroing.
 * onssen_loss_enhance_grad_f32, one elementwise pass, d_est (B, TF) contiguous:
 *   MSA  d_est = g[0] * 2 * scale * (est - mag_clean)            (g: the incoming gradient of total, one float)
 *   PSA  d_est = g[b] * mag_noisy * sign(est * mag_noisy - t)    (g: the incoming gradient of per_utt, B floats; sign(0) = 0) */
#define ONSSEN_ENHANCE_MSA 0
#define ONSSEN_ENHANCE_PSA 1
int onssen_labels_enhance_f32(const float* stft_noisy, const float* stft_clean, int64_t n_bins, float* mag_noisy, float* mag_clean,
                              float* cos_diff, void* stream);
size_t onssen_loss_enhance_workspace_bytes(int B);
int onssen_loss_enhance_f32(int mode, const float* est, const float* mag_noisy, const float* mag_clean, const float* cos_diff, int B,
                            int TF, float scale, float* per_utt, float* total, void* ws, size_t ws_bytes, void* stream);
int onssen_loss_enhance_grad_f32(int mode, const float* est, const float* mag_noisy, const float* mag_clean, const float* cos_diff,
                                 int B, int TF, float scale, const float* g, float* d_est, void* stream);
/* uPIT (the permutation-invariant mask network), csrc/loss_upit.inc: the utterance-level mask loss for S = 2 .. 4 speakers.
 * Per utterance b over its bins, x = mag_mix, m_k the S mask estimates, t_j = mag_s_j (cos_src NULL: MSA) or
 * min(x, relu(mag_s_j * cos_j)) (PSA):
 *   pair[b][k][j] = sum_bins |m_k x - t_j|,   total[b][p] = sum_k pair[b][k][p[k]] for the S! assignments p in the order of
 *   itertools.permutations(range(S)),   out[b] = min_p total[b][p],   perm[b] = the index of that p (of equal totals the smallest).
 * Mask k at bin e of row b sits at masks[b * m_sb + e * m_se + k * m_ss] (the network's interleaved (B, TF, S) buffer: TF * S, S, 1;
 * S contiguous maps: TF, 1, B * TF).  mag_mix (B, TF) contiguous; source j's map (B, TF) contiguous at mag_src + j * s_sd,
 * cos_src + j * c_sd (16-byte loads where the rows are aligned, the same bits where they are not).  frames (nullable, B values,
 * with F | TF): row b covers its first frames[b] * F bins only -- bit for bit the value of a batch-1 call on them; its gradient
 * beyond them is written as zero.  perm and pair (B, S, S) may be NULL.  Per-bin terms in fp32 (the residual is one fused
 * multiply-add), sums in fp64 in a fixed order (no atomics: bit-repeatable).  ws: caller-owned, 8-byte aligned,
 * onssen_loss_upit_workspace_bytes(B, S) bytes, needs no zeroing.
 * onssen_loss_upit_grad_f32, one elementwise pass: d_masks (strided like masks; every element written)
 *   d m_k = g[b] * x * sign(m_k x - t_p[k]),  p = assignment number perm[b];  sign(0) = 0. */
size_t onssen_loss_upit_workspace_bytes(int B, int S);
int onssen_loss_upit_f32(const float* masks, int64_t m_sb, int64_t m_se, int64_t m_ss, const float* mag_mix, const float* mag_src,
                         int64_t s_sd, const float* cos_src, int64_t c_sd, const int32_t* frames, int F, int B, int TF, int S,
                         float* out, int32_t* perm, float* pair, void* ws, size_t ws_bytes, void* stream);
int onssen_loss_upit_grad_f32(const float* masks, int64_t m_sb, int64_t m_se, int64_t m_ss, const float* mag_mix,
                              const float* mag_src, int64_t s_sd, const float* cos_src, int64_t c_sd, const int32_t* frames, int F,
                              int B, int TF, int S, const float* g, const int32_t* perm, float* d_masks, int64_t d_sb, int64_t d_se,
                              int64_t d_ss, void* stream);
size_t onssen_loss_dc_workspace_bytes(int B);
int onssen_loss_dc_f32(const float* emb, const float* one_hot, const float* mag, int B, int TF, int D, int C,
                       float* per_utt, float* total_mag, void* ws, size_t ws_bytes, void* stream);
/* d_emb (B, TF, D) = sum_b g_per_utt[b] * d per_utt[b] / d emb -- what autograd derives from loss_dc.py:36-44 (the norms of the
 * affinity blocks): with Z = [V | Y] (weighted as above) and G = Z^T Z, dV = Z [2 Gvv/||Gvv|| ; -2 Gvy^T/||Gvy||], scaled back
 * through the weights.  `ws` must be the workspace onssen_loss_dc_f32 has just filled for the SAME emb / one_hot / mag (its
 * partial Grams are reused); the embedding is read once and d_emb written once.  C <= 4. */
int onssen_loss_dc_grad_f32(const float* emb, const float* one_hot, const float* mag, int B, int TF, int D, int C,
                            const float* g_per_utt, float* d_emb, void* ws, size_t ws_bytes, void* stream);
/* Fusion at the train-step level (the labels are in hand there): from the normalised embedding `emb` [B*T][F*D] and the
 * reciprocal norms `inv_norm` [B*T][F] of onssen_linear_x3p_norms, with the partial Grams onssen_loss_dc_f32 left in ws, straight
 * to the operands of fc_dc's gradient GEMMs -- the gradient of loss_dc w.r.t. the embedding, taken through F.normalize, written as
 * the row-major x3 image [B*T][ceil(F*D/32)][2][32] (dx = draw W), the transposed x3 image [F*D][ceil(B*T/32)][2][32]
 * (dW = draw^T x; img_t may be NULL: onssen_linear_x3t takes the row-major one) and colsum [ceil(B*T/32)][F*D] (db = its sum over the blocks).  Neither d(loss)/d(embedding) nor the gradient of
 * the raw product exists in memory.  D = 20, C <= 4, T >= 32.  g_per_utt [B]: dL/d(per-utterance loss). */
int onssen_dc_head_grad_images_f32(const float* emb, const float* inv_norm, const float* one_hot, const float* mag, int B, int T,
                                   int F, int D, int C, float eps, const float* g_per_utt, void* ws, size_t ws_bytes,
                                   uint16_t* img_rows, uint16_t* img_t, float* colsum, void* stream);

/* ---------------------------------------------------------------------------------------------
 * N4  batch SI-SDR with the best source permutation (evaluation metric of tester.eval):
 *   sdr_out[b] = max over permutations P of (1/C) sum_i SDR(est[b,i], org[b,P(i)]), signals zero-mean, optional
 *   (B, n) mask applied after centring; perm_out[b] (nullable) = index of P in lexicographic order.
 * Replaces calc_sdr_torch + batch_SDR_torch (onssen/evaluate/sdr.py:11-87).  est, org (B, C, n); C <= 4.
 * Means, Gram matrix and the SDR table are accumulated / evaluated in fp64 (the residual power from a Gram matrix cancels:
 * fp32 sums were wrong by 0.1 dB at 50 dB and NaN from ~70 dB); ws 8-byte aligned.
 */
size_t onssen_batch_sdr_workspace_bytes(int B);
int onssen_batch_sdr_f32(const float* est, const float* org, const float* mask, int B, int C, int n, float* sdr_out,
                         int* perm_out, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * SI-SNR permutation-invariant training loss of Conv-TasNet, value and gradient (csrc/loss_sisnr.inc).
 * Replaces cal_si_snr + the permutation search + the batch mean of onssen/loss/loss_e2e.py:45-87 and what autograd derives
 * from them.  For estimates x_i and references s_j, i, j < k <= 4, each N rows of S samples, eps = 1e-8:
 *   x~ = x - mean(x), s~ = s - mean(s), a = <x~, s~> / (|s~|^2 + eps), t = a s~,
 *   v(i, j) = 20 log10(eps + |t| / (|x~ - t| + eps)),
 *   value[b] = max over the permutations p of (1/k) sum_i v(i, p(i))   (lexicographic order, the first maximum wins),
 *   perm[b]  = index of that permutation (nullable),  total[0] = -sum_b value[b] / N (nullable).
 * The signals are passed as k base pointers with a row stride each (host arrays of device pointers / of strides in floats,
 * stride >= S): k views of one (k, N, S_out) buffer and k separate tensors both work without a copy; any alignment is taken
 * (rows on 16-byte boundaries are fetched 16 bytes at a time; the result does not depend on it).
 * lengths (nullable, device int32 [N]): row b is its first lengths[b] samples for means, norms and products; its value and
 * gradient are bit for bit those of the one-row call on that prefix, the gradient beyond it is zero, N stays the divisor.
 * (A device value cannot be refused by the host: it is clamped to [1, S].)
 * Degenerate rows as ATen: an all-zero or constant estimate or reference gives v = -160 and a zero gradient (a zero norm has
 * subgradient zero); an estimate that is an exact multiple of its reference gives a finite value and gradient.
 * One pass over the signals forward (fp64 moments per chunk, merged in a fixed order: bit-repeatable, no atomics), one
 * elementwise pass backward:  d_est[i][b][t] = A x_i[b,t] + B s_p(i)[b,t] + C  evaluated in fp64 and rounded once, with
 * the three fp64 coefficients per (row, estimate) the forward left in ws.  d_est is (k, N, S) contiguous and written once.
 * g_value [N] and / or g_total [1] (device; one may be NULL): the incoming gradients of value and of total.
 * ws: caller-owned, 8-byte aligned, onssen_sisnr_pit_workspace_bytes(N, k) bytes, needs no zeroing; the backward reads what the
 * forward of the same batch left in it.  Refused before anything is launched or written: k < 1, k > 4, N < 1, N > 65535,
 * S < 1, a NULL pointer, a row stride < S (ONSSEN_E_ARG); a short ws (ONSSEN_E_WORKSPACE).
 */
size_t onssen_sisnr_pit_workspace_bytes(int N, int k);
int onssen_sisnr_pit_f32(const float* const* est_host, const int64_t* est_stride_host, const float* const* ref_host,
                         const int64_t* ref_stride_host, int k, int N, int S, const int32_t* lengths, float* value,
                         int32_t* perm, float* total, void* ws, size_t ws_bytes, void* stream);
int onssen_sisnr_pit_backward_f32(const float* const* est_host, const int64_t* est_stride_host, const float* const* ref_host,
                                  const int64_t* ref_stride_host, int k, int N, int S, const int32_t* lengths,
                                  const float* g_value, const float* g_total, float* d_est, const void* ws, size_t ws_bytes,
                                  void* stream);

/* ---------------------------------------------------------------------------------------------
 * K10  mask-apply + inverse STFT overlap-add.
 * Replaces `stft_est = stft_mix * mask; librosa.core.istft(stft_est[i].T, hop_length, length)` at
 * egs/wsj0-2mix/deep_clustering/evaluate.py:42-45 and egs/wsj0-2mix/chimera/evaluate.py:40-43.
 *   stft_ri  (B, T, F, 2) float32;  mask element (b,c,t,f) at mask + b*m_sb + c*m_sc + t*m_st + f*m_sf
 *            (mask = NULL means all-ones);  out (B, C, length) float32
 * n_fft = 2(F-1) in {256, 512, 1024}; periodic Hann; divide by the window sum-of-squares where > tiny.
 */
int onssen_mask_istft_f32(const float* stft_ri, const float* mask, int64_t m_sb, int64_t m_sc, int64_t m_st,
                          int64_t m_sf, int B, int C, int T, int n_fft, int hop, int length, float* out,
                          void* stream);
/* The same with a phase estimate per speaker (phase_net's reconstruction): speaker c's spectrum at a bin is
 *   mask_c * |X| * (p_c.re + i p_c.im),  |X| = hypotf(Re X, Im X) in float32,
 * instead of X * mask_c; p_c (B, T, F, 2) contiguous at phase + c*p_sc (8-byte aligned, p_sc even: two views of one buffer, or
 * two tensors whose distance is p_sc floats).  The imaginary parts at DC and Nyquist are dropped like those of X above.
 * Uniform batches only; n_fft in {256, 512, 1024}. */
int onssen_phase_istft_f32(const float* stft_ri, const float* mask, int64_t m_sb, int64_t m_sc, int64_t m_st, int64_t m_sf,
                           const float* phase, int64_t p_sc, int B, int C, int T, int n_fft, int hop, int length, float* out,
                           void* stream);
/* onssen_phase_istft_f32 on a ragged batch: `frames` and `lengths` exactly as onssen_mask_istft_ragged_f32 below (frames[b] <= T
 * frames in, lengths[b] <= length samples out, zeros after them); row b inside its own length is bit for bit the uniform call on
 * that utterance alone (B = 1, T = frames[b]).  NULL `phase`, `frames` or `lengths`: ONSSEN_E_ARG. */
int onssen_phase_istft_ragged_f32(const float* stft_ri, const float* mask, int64_t m_sb, int64_t m_sc, int64_t m_st, int64_t m_sf,
                                  const float* phase, int64_t p_sc, int B, int C, int T, const int32_t* frames, int n_fft, int hop,
                                  int length, const int32_t* lengths, float* out, void* stream);
/* MISI (multiple input spectrogram inversion) half-step: from the mixture and C time-domain estimates to the C phase maps that
 * the next onssen_phase_istft_f32 reads, in one launch.  Per sample, in fp64 on load,
 *   d = (mix[n] - sum_{j<C} est_j[n]) / C  (sum in index order),   u_c[n] = est_c[n] + d
 * -- the residual spread evenly, so that the estimates sum to the mixture; no waveform is written -- then Z_c = STFT(u_c) (centred
 * frames, periodic Hann, reflect padding: the framing of onssen_stft_logmag_f32, fp64 transform) and
 *   phase[c][b][t][f] = (Re Z_c / h, Im Z_c / h),  h = hypot(Re Z_c, Im Z_c) in fp64, rounded once to float32; (1, 0) where Z_c = 0.
 *   mix    row b at mix + b*mix_stride, n_samples float32;  est (b, c) at est + b*est_sb + c*est_sc, unit sample stride
 *   phase  (C, B, T, F, 2) float32, T = 1 + n_samples/hop, F = n_fft/2 + 1: onssen_phase_istft_f32's `phase` with p_sc = B*T*F*2
 * Two speakers share one complex transform; deterministic, no atomics, no workspace.
 * The ragged form: n_per_utt[b] samples of row b are valid (n_fft/2 < n_per_utt[b] <= n_max; a device value outside is clamped);
 * the row mirrors about its own last sample, nothing beyond it is read, its frames 0 .. n_per_utt[b]/hop are bit for bit those of
 * the uniform call on that row alone, and the frames after them, up to T = 1 + n_max/hop, are silence: (1, 0).
 * Refused before anything is launched: a NULL pointer, B < 1, C < 2, C > 8, hop < 1, hop > n_fft, n_samples <= n_fft/2, n_fft not
 * in {256, 512, 1024} (ONSSEN_E_ARG); `phase` not 8-byte aligned (ONSSEN_E_ALIGN: (re, im) pairs are stored as one word). */
int onssen_misi_phase_f32(const float* mix, int64_t mix_stride, const float* est, int64_t est_sb, int64_t est_sc, int B, int C,
                          int n_samples, int n_fft, int hop, float* phase, void* stream);
int onssen_misi_phase_ragged_f32(const float* mix, int64_t mix_stride, const float* est, int64_t est_sb, int64_t est_sc, int B,
                                 int C, int n_max, const int32_t* n_per_utt, int n_fft, int hop, float* phase, void* stream);
/* The same from an estimated MAGNITUDE with the mixture's phase (enhancement's reconstruction): `mag` (strided like `mask`, not
 * NULL) and the spectrum at a bin is
 *   mag * X / |X|,  |X| = hypotf(Re X, Im X) and both quotients in float32, the product in fp64; (1, 0) for X / |X| where X = 0
 * (np.angle(0) = 0).  Any C (one transform per channel); n_fft in {256, 512, 1024}.  The ragged form takes `frames` and
 * `lengths` exactly as onssen_mask_istft_ragged_f32 below. */
int onssen_mag_istft_f32(const float* stft_ri, const float* mag, int64_t m_sb, int64_t m_sc, int64_t m_st, int64_t m_sf, int B,
                         int C, int T, int n_fft, int hop, int length, float* out, void* stream);
int onssen_mag_istft_ragged_f32(const float* stft_ri, const float* mag, int64_t m_sb, int64_t m_sc, int64_t m_st, int64_t m_sf,
                                int B, int C, int T, const int32_t* frames, int n_fft, int hop, int length, const int32_t* lengths,
                                float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Waveform-approximation training (Wang, Le Roux, Wang & Hershey 2018): the gradient through one inverse transform and the L1
 * waveform loss under the best speaker permutation (csrc/istft_bwd.inc, csrc/loss_wa.inc).  No upstream counterpart.
 *
 * onssen_istft_backward_f32: the adjoint of onssen_mask_istft_f32 (mode 0), onssen_phase_istft_f32 (mode 1) and
 * onssen_mag_istft_f32 (mode 2), uniform (frames = lengths = NULL) or ragged (both given), in one launch.  With g_out the
 * gradient at the forward's `out` ((B, C, length) CONTIGUOUS float32; nothing of a row is read beyond lengths[b], so it counts
 * as zero there), w the periodic Hann window, rw[n] the forward's reciprocal window sum of squares and a_f = 1 at DC / Nyquist, else 2:
 *   G_c[t, f] = a_f * sum_i (w[i] / N) rw[n] g_out_c[n] e^{-2 pi i f i / N},   n = t hop + i - N/2
 *   mode 0:  g_operand_c = Re X Re G + Im X Im G
 *   mode 1:  g_operand_c = |X| (Re p_c Re G + Im p_c Im G),   g_phase_c = mask_c |X| (Re G, Im G)
 *   mode 2:  g_operand_c = Re u Re G + Im u Im G,  u = X / |X| as the forward forms it ((1, 0) where X = 0)
 * with the imaginary terms dropped at DC and Nyquist, as the forward ignores them; fp64 transform and products, one rounding.
 *   g_operand (B, T, F, C) contiguous float32: the gradient at the masks (modes 0, 1) or magnitudes (mode 2)
 *   g_phase   (C, B, T, F, 2) contiguous float32, 8-byte aligned, mode 1 only (NULL otherwise): the gradient at the phase maps
 *   operand   the forward's masks with their strides: read in mode 1 only (for g_phase), may be NULL otherwise
 *   phase, p_sc: as onssen_phase_istft_f32, mode 1 only
 * Frames t >= frames[b] get zeros; nothing of X, the masks or the phases is read there.  Row b inside its own frames is bit for bit
 * the uniform call on that utterance alone.  Deterministic, no atomics, no workspace.
 * Refused before anything is launched: a NULL required pointer, B < 1, C < 1, T < 1, length < 1, hop < 1, hop > n_fft, n_fft not in
 * {256, 512, 1024}, only one of frames / lengths, an unknown mode (ONSSEN_E_ARG); stft_ri, phase or g_phase off an 8-byte
 * boundary, an odd p_sc (ONSSEN_E_ALIGN).
 */
int onssen_istft_backward_f32(const float* stft_ri, const float* operand, int64_t m_sb, int64_t m_sc, int64_t m_st, int64_t m_sf,
                              const float* phase, int64_t p_sc, int mode, int B, int C, int T, const int32_t* frames, int n_fft, int hop,
                              int length, const int32_t* lengths, const float* g_out, float* g_operand, float* g_phase, void* stream);
/* onssen_misi_phase_backward_f32: the adjoint of onssen_misi_phase_f32 / onssen_misi_phase_ragged_f32 (csrc/misi_bwd.inc) -- with
 * onssen_istft_backward_f32 in mode 1, which returns the gradient at the phase maps, what training through K unfolded MISI
 * iterations needs.  mix, est and their strides as in the forward; n_per_utt NULL: a uniform batch.  g_phase (C, B, T, F, 2)
 * CONTIGUOUS float32, T = 1 + n_max/hop: the gradient at the forward's `phase`; g_est (B, C, n_max) CONTIGUOUS float32: the
 * gradient at `est` (the mixture is data and gets none).  With Z_c the forward's spectra, recomputed in fp64 from the same
 * float32 mix and est (the forward's float32 `phase` is not an input), and p = Z / |Z|:
 *   g_Z = (g_phase - p (p . g_phase)) / |Z|           0 wherever the forward wrote its (1, 0) fallback
 *   r_t = w[i] * sum_f H[f] e^{+2 pi i f i / N}       H[f] = g_Z[f] / 2 for 0 < f < N/2, Re g_Z[f] at f in {0, N/2}, Hermitian beyond
 *   g_u = overlap-add of r_t over the reflect-padded axis, the padding folded back about sample 0 and sample n_b - 1
 *   g_est_c = g_u_c - (1 / C) sum_j g_u_j
 * Two launches (transform per frame and speaker pair; gather per sample), fp64 throughout with one rounding on the store, sums
 * in a fixed order, no atomics: bit-repeatable, nothing read back by the host, capturable in a graph.  Ragged: row b inside
 * n_per_utt[b] is bit for bit the batch-1 call on that row, exactly 0 after it; nothing of mix / est beyond n_per_utt[b] and
 * nothing of g_phase at frames >= 1 + n_per_utt[b]/hop is read; a device length is kept inside (n_fft/2, n_max].
 * ws: caller-owned, 8-byte aligned, onssen_misi_phase_backward_workspace_bytes(B, C, n_max, n_fft, hop) bytes (0 for a refused
 * geometry), needs no zeroing.
 * Refused before anything is launched or written: a NULL pointer (n_per_utt may be NULL), B < 1, C < 2, C > 8, hop < 1,
 * hop > n_fft, n_max <= n_fft/2, n_fft not in {256, 512, 1024} (ONSSEN_E_ARG); a short ws (ONSSEN_E_WORKSPACE); g_phase or ws
 * off an 8-byte boundary (ONSSEN_E_ALIGN). */
size_t onssen_misi_phase_backward_workspace_bytes(int B, int C, int n, int n_fft, int hop);
int onssen_misi_phase_backward_f32(const float* mix, int64_t mix_stride, const float* est, int64_t est_sb, int64_t est_sc, int B,
                                   int C, int n_max, const int32_t* n_per_utt, int n_fft, int hop, const float* g_phase,
                                   float* g_est, void* ws, size_t ws_bytes, void* stream);
/* The waveform L1 loss with the best permutation.  est (B, C, n) contiguous (the inverse transform's output); ref (b, j) at
 * ref + b*r_sb + j*r_sc, unit sample stride, |stride| >= n; C <= 4.  Per row with n_b = lengths[b] valid samples (NULL: n; a device
 * value is clamped to [1, n]):
 *   D[i][j]  = sum_{t < n_b} |est_i[t] - ref_j[t]|   (fp64, fixed order)
 *   value[b] = min over permutations p of sum_i D[i][p(i)] / (C n_b)   (lexicographic order, the first minimum wins)
 *   perm[b]  = index of that permutation (nullable),   total[0] = sum_b value[b] / B (nullable)
 *   d_est[b][i][t] = (g_value[b] + g_total[0] / B) * sign(est_i[t] - ref_p(i)[t]) / (C n_b),  0 at equality and at t >= n_b
 * One pass over the signals forward (fp64 partial sums per chunk, merged in a fixed order: bit-repeatable, no atomics), one
 * elementwise pass backward that reads the assignment the forward of the same batch left in ws.  d_est (B, C, n) contiguous.
 * ws: caller-owned, 8-byte aligned, onssen_wa_pit_workspace_bytes(B, C) bytes (0 for a refused B or C), needs no zeroing.
 * Refused before anything is launched or written: C < 1, C > 4, B < 1, B > 65535, n < 1, a NULL pointer (g_value and g_total both
 * NULL), a row stride shorter than n (ONSSEN_E_ARG); a short ws (ONSSEN_E_WORKSPACE); a misaligned ws (ONSSEN_E_ALIGN).
 */
size_t onssen_wa_pit_workspace_bytes(int B, int C);
int onssen_wa_pit_f32(const float* est, const float* ref, int64_t r_sb, int64_t r_sc, int B, int C, int n, const int32_t* lengths,
                      float* value, int32_t* perm, float* total, void* ws, size_t ws_bytes, void* stream);
int onssen_wa_pit_backward_f32(const float* est, const float* ref, int64_t r_sb, int64_t r_sc, int B, int C, int n,
                               const int32_t* lengths, const float* g_value, const float* g_total, float* d_est, const void* ws,
                               size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Ragged batches (round 4): the reference evaluates WHOLE utterances one at a time (onssen/utils/test.py:29-41 with the
 * batch-1 loader of onssen/data/wsj0_2mix.py:231-245), a shape that leaves most of the chip idle.  These entry points
 * run K utterances of different lengths in one launch sequence: every buffer keeps the padded batch shape (T = the longest
 * utterance's frames, n = the longest sample count) and a device array gives each row's own extent.  Row b's results
 * inside its own extent are bit-identical to what the uniform entry point returns for that utterance alone (B = 1,
 * T = frames[b]); outside it they are defined as stated below.
 *
 * onssen_stft_logmag_ragged_f32: n_per_utt[b] samples of row b are valid (n_fft/2 < n_per_utt[b] <= n_max; the reflect
 *   padding mirrors about the row's own last sample); T = 1 + n_max/hop frames are written per row, the frames past
 *   1 + n_per_utt[b]/hop as the transform of silence (log-magnitude log10(eps), spectrum 0 -- to rounding, ~1e-16).
 * onssen_blstm_forward_ragged_f32: frames[b] <= T live frames of row b; at t >= frames[b] the row holds h = c = 0 in both
 *   directions (the reverse direction therefore starts from zero state at the row's own last frame) and its output rows are
 *   0 -- whatever the input holds there (a NaN of the padding does not spread).  ONSSEN_BLSTM_XCD | ONSSEN_BLSTM_BF16X3
 *   without ONSSEN_BLSTM_FUSE_IN0 / ONSSEN_BLSTM_BF16 runs the persistent form; the launch-per-step form takes ragged
 *   batches in both precisions; other flag combinations return ONSSEN_E_ARG.
 * onssen_dc_cluster_ragged_f32: utterance b owns the first frames[b]*F bins of its slab; its padding is never active
 *   (masks 0) and takes no part in the maximum, the initialisation or the sums.
 * onssen_mask_istft_ragged_f32: frames[b] frames and lengths[b] <= length output samples per row (librosa.istft(...,
 *   length = lengths[b]) semantics); out (B, C, length), zeros past lengths[b].
 * onssen_batch_sdr_ragged_f32: row b holds lengths[b] <= n samples (est, org, mask keep the row stride n).
 */
int onssen_stft_logmag_ragged_f32(const float* wav, int B, int n_max, int64_t wav_stride, const int32_t* n_per_utt, int n_fft,
                                  int hop, float eps, float* logmag, float* stft_ri, void* stream);
int onssen_blstm_forward_ragged_f32(const float* x, int64_t xs_b, int64_t xs_t, int B, int T, const int32_t* frames,
                                    int in_dim, int H, int L, int ug, const float* const* wih_p_host,
                                    const float* const* whh_p_host, const float* const* bias_p_host, float* y, void* ws,
                                    size_t ws_bytes, int flags, void* stream);
int onssen_dc_cluster_ragged_f32(const float* emb, const float* feature, int B, int T, const int32_t* frames, int F, int D,
                                 float db_threshold, int iters, float tol, float* masks, void* ws, size_t ws_bytes, int flags,
                                 void* stream);
int onssen_mask_istft_ragged_f32(const float* stft_ri, const float* mask, int64_t m_sb, int64_t m_sc, int64_t m_st,
                                 int64_t m_sf, int B, int C, int T, const int32_t* frames, int n_fft, int hop, int length,
                                 const int32_t* lengths, float* out, void* stream);
int onssen_batch_sdr_ragged_f32(const float* est, const float* org, const float* mask, int B, int C, int n,
                                const int32_t* lengths, float* sdr_out, int* perm_out, void* ws, size_t ws_bytes,
                                void* stream);

/* ---------------------------------------------------------------------------------------------
 * Deep-clustering separation without the embedding round trip (round 4).  Which bins are clustered is decided by the
 * mixture's log-magnitude alone (`m = np.max(feature_mix) - 40/20; emb = embedding[feature_mix >= m, :]`,
 * egs/wsj0-2mix/deep_clustering/evaluate.py:36-37) and is known before the network has run; the silent bins' embeddings
 * are never read (their masks are 0).  So:
 *   1. onssen_dc_index_f32 (after the STFT): per utterance the threshold, the number of active bins and a target map
 *      dest[b][t*F + f] = row of bin (t, f) in the utterance's compacted array, -1 for a silent bin (int32, inside ws);
 *   2. onssen_linear_x3p_compact: the fc_dc GEMM of onssen_linear_x3p with ONSSEN_EPI_L2NORM whose epilogue stores only the
 *      normalised rows of the active bins, each straight into its row of the compacted array (comp, inside ws);
 *   3. onssen_dc_cluster_compact_f32: farthest-point initialisation, all Lloyd iterations in one persistent launch and the
 *      mask pass on the compacted array -- the same arithmetic as onssen_dc_cluster_f32 in its default form, bit-identical
 *      masks, without the 10 320 B/frame embedding write, its re-read and the compaction pass.
 * ws: onssen_dc_compact_workspace_bytes() bytes, 256-byte aligned, the part in front of the compacted array zeroed by its
 * owner like onssen_dc_cluster_f32's (same status word: onssen_dc_cluster_status_offset); onssen_dc_compact_layout gives the
 * byte offsets of `comp` ([B][T*F][D] floats, rows past an utterance's active count unused) and `dest` ([B][T*F] int32).
 * frames: NULL, or per-utterance frame counts of a ragged batch (see the ragged entry points).
 * onssen_linear_x3p_compact: a_img / w_img / bias / N / group / eps as onssen_linear_x3p (N = F * group); row m of the GEMM is
 * (utterance m % R, frame m / R); dest_bs = ints per utterance in dest, comp_bs = floats per utterance in comp; dest must be
 * readable for 12 bytes past its last entry (the map is fetched in 16-byte words; the workspace layout above pads it). */
size_t onssen_dc_compact_workspace_bytes(int B, int T, int F, int D);
int onssen_dc_compact_layout(int B, int T, int F, int D, size_t* comp_offset, size_t* dest_offset);
int onssen_dc_index_f32(const float* feature, int B, int T, const int32_t* frames, int F, int D, float db_threshold, void* ws,
                        size_t ws_bytes, void* stream);
int onssen_linear_x3p_compact(const uint16_t* a_img, int M, int K, const uint16_t* w_img, const float* bias, int N, int group,
                              float eps, const int32_t* dest, int64_t dest_bs, int F, float* comp, int R, int64_t comp_bs,
                              int bf16_only, void* stream);
int onssen_dc_cluster_compact_f32(int B, int T, int F, int D, int iters, float tol, float* masks, void* ws, size_t ws_bytes,
                                  int flags, void* stream);

/* ---------------------------------------------------------------------------------------------
 * N2, K speakers: the deep-clustering back end for K = 2 .. 4 clusters (`num_spk = sig_ref.shape[1]`,
 * `KMeans(n_clusters=num_spk)` and num_spk masks at egs/wsj0-2mix/deep_clustering/evaluate.py:33-44).  Threshold as above;
 * masks (B,T,F,K): channel k is 1 where the bin is active and belongs to cluster k, every channel 0 on silent bins and on the
 * padding of a ragged batch (frames: NULL, or frames[b] <= T frames per utterance, as onssen_dc_cluster_ragged_f32).
 * The arithmetic is fixed, so the cluster numbering is deterministic and two calls give the same bits:
 *   initialisation  c_0 = the embedding of the loudest bin (first maximum); c_k, k = 1 .. K-1, = the active bin that
 *                   minimises max_{j<k} e.c_j (farthest point on unit vectors; ties to the smallest bin index; c_0 when
 *                   there is no candidate).  K = 2: the initialisation of onssen_dc_cluster_f32.
 *   iteration       label = argmin_k |c_k|^2 - 2 e.c_k (ties to the smallest k); new centroid = mean of its bins (an empty
 *                   cluster keeps its centroid); stops at the bitwise fixed point, by the tol rule of onssen_dc_cluster_f32,
 *                   or after `iters` iterations
 *   masks           labels under the final centroids; cluster k is the one grown from c_k
 * One form only: one assignment launch and one update launch per iteration (2 K + 2 iters + 1 launches per call), no
 * inter-workgroup waits, no atomics.  D <= 32; emb and masks 16-byte aligned, ws 256-byte aligned (ONSSEN_E_ALIGN).
 * ONSSEN_E_ARG: K outside 2 .. 4, D outside 1 .. 32, B, T or F < 1, iters < 0, tol < 0, a NULL pointer, or ws_bytes below
 * what the size query returns (which is 0 for an unsupported shape); nothing is launched or written then.
 * Workspace, written by every call (no zeroing by the owner): int32 words [4 b + 0] = Lloyd iterations run for utterance b
 * and [4 b + 1] = 1 when it stopped by the fixed point or the tol rule, 0 when `iters` ran out ([4 b + 2], [4 b + 3]: the
 * loudest bin, reserved); the float part (feature maximum, centroids, partial sums) follows 256-byte aligned. */
size_t onssen_dc_cluster_k_workspace_bytes(int B, int T, int F, int D, int K);
int onssen_dc_cluster_k_f32(const float* emb, const float* feature, int B, int T, const int32_t* frames /* may be NULL */,
                            int F, int D, int K, float db_threshold, int iters, float tol, float* masks, void* ws,
                            size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * H1  host side of the data front end (round 5): a batch of RIFF/WAVE files -> float32 mono rows of one host buffer.
 * Replaces `librosa.load(fn, sr=None)` (onssen/data/feature_utils.py:15), called three times per training sample from
 * Dataset.__getitem__ on the training thread (onssen/data/wsj0_2mix.py:114-116, num_workers 0: :28-32).  HOST pointers
 * only; no device work, no stream.  onssen_wav_read_batch_f32 reads `count` files on up to `threads` host threads into
 * out_host + i * row_stride (floats; a pinned buffer makes the following H2D copy one asynchronous transfer):
 *   frames_host[i] = frames written (<= row_stride), rates_host[i] = the file's sample rate (resampling, if the rate is not
 *   the recipe's, stays with the caller as in feature_utils.py:17-20), status_host[i] = 0 | ONSSEN_WAV_TRUNCATED | ONSSEN_WAV_E_*.
 * Samples: PCM 8-bit (x - 128) / 128, 16-bit x / 2^15, 24-bit (left-justified in 32) and 32-bit x / 2^31, IEEE float 32 / 64
 * -> float32; several channels -> their float32 mean (what librosa.load(mono=True) returns for these files).
 * Returns ONSSEN_OK, ONSSEN_E_ARG, or ONSSEN_WAV_E_SOME_FAILED when a file failed (the others were still read).
 * onssen_wav_info: the header only; bits_host < 0 marks IEEE float. */
int onssen_wav_info(const char* path_host, int64_t* frames_host, int32_t* rate_host, int32_t* channels_host, int32_t* bits_host);
int onssen_wav_read_batch_f32(const char* const* paths_host, int count, float* out_host, int64_t row_stride, int32_t* frames_host,
                              int32_t* rates_host, int32_t* status_host, int threads);

/* Calibration probe (not part of the separation path): n dependent launches of a near-empty kernel with
 * `workgroups` x 256 threads on `stream`; bracket it with events to measure this box's launch-boundary floor. */
int onssen_debug_launch_chain(float* scratch, int n, int workgroups, void* stream);

/* Co-tenant probe (not part of the separation path; tools/cotenant_probe.py): `workgroups` x `threads` threads that only
 * hold their compute units for `ticks` ticks of the 100 MHz wall clock on `stream` -- a stand-in for RCCL's channel
 * kernels running beside the persistent recurrences (a recurrence group needs 30 of its XCD's 32 CUs at the same time).
 * heavy != 0: >= 112 live VGPRs per lane and 32 KB of LDS (cannot share a CU with a recurrence workgroup). */
int onssen_debug_cotenant_spin(int workgroups, int threads, long long ticks, int heavy, void* stream);

/* Bound of every wait inside the persistent kernels (ONSSEN_BLSTM_XCD forward, training forward / backward), in polling
 * passes: default 400000 (~0.2 s), initial value from ONSSEN_XCD_SPIN_LIMIT.  new_limit >= 0 sets it (0: every wait gives
 * up at once -- abort-path tests; data-parallel training raises it, see onssen_amd/dist.py), new_limit < 0 only queries.
 * Returns the previous value.  Process-wide; takes effect at the next launch. */
long long onssen_xcd_spin_limit(long long new_limit);

/* ---------------------------------------------------------------------------------------------
 * Conv-TasNet separation forward (onssen/nn/tasnet.py:166-264), eval semantics.
 * cfg_host: 12 HOST int32 values {N, L, B, H, P, X, R, norm, num_spks, activate, causal, precision}; norm / activate /
 *   precision take the ONSSEN_TASNET_* values below.  Limits: L even, 2 <= L <= 64, N <= 1024, P <= 32 (odd unless causal),
 *   X <= 30, num_spks <= 8.
 * params: the flat fp32 parameters (device), in this order: encoder.weight [N][L], encoder.bias [N], LayerN_S.weight [N],
 *   LayerN_S.bias [N], BottleN_S.weight [B][N], BottleN_S.bias [B]; for each block r * X + x: conv1x1.weight [H][B],
 *   conv1x1.bias [H], PReLU_1.weight [1], norm_1 (gln / cln: weight [H], bias [H]; bn: weight, bias, running_mean,
 *   running_var [H] each), dwconv.weight [H][P], dwconv.bias [H], Sc_conv.weight [B][H], Sc_conv.bias [B]; then
 *   gen_masks.weight [num_spks N][B], gen_masks.bias [num_spks N], decoder.weight [N][L], decoder.bias [1]
 *   (onssen_tasnet_param_floats values).  PReLU_2 / norm_2 are not used by the reference's forward and are not passed.
 * image: onssen_tasnet_image_bytes() bytes, 256-byte aligned, written by onssen_tasnet_pack_f32 (stream-ordered); one image
 *   serves every precision.
 * forward: x (n, S) with row stride x_stride >= S floats; T = (S - L) / (L/2) + 1 frames, S_out = (T - 1) L/2 + L;
 *   out = num_spks x n x S_out (contiguous); ws = onssen_tasnet_workspace_bytes(cfg, n, S) bytes, 256-byte aligned, no
 *   zeroing needed.  The 1x1 convolutions run on onssen_linear_f32 (precision F32) or an x3 image + onssen_linear_x3p
 *   (BF16X3, BF16).  Deterministic: no atomics; gLN statistics are fp64 partial sums merged in a fixed order.
 */
#define ONSSEN_TASNET_GLN 0
#define ONSSEN_TASNET_CLN 1
#define ONSSEN_TASNET_BN 2
#define ONSSEN_TASNET_RELU 0
#define ONSSEN_TASNET_SIGMOID 1
#define ONSSEN_TASNET_SOFTMAX 2
#define ONSSEN_TASNET_F32 0
#define ONSSEN_TASNET_BF16X3 1
#define ONSSEN_TASNET_BF16 2
/* OR-ed into precision, shifted left by 8: these 1x1 convolutions run on exact fp32 whatever the precision */
#define ONSSEN_TASNET_EXACT_BOTTLENECK 1
#define ONSSEN_TASNET_EXACT_CONV1X1 2
#define ONSSEN_TASNET_EXACT_SC_CONV 4
#define ONSSEN_TASNET_EXACT_MASKS 8
int64_t onssen_tasnet_param_floats(const int32_t* cfg_host);
size_t onssen_tasnet_image_bytes(const int32_t* cfg_host);
int onssen_tasnet_pack_f32(const int32_t* cfg_host, const float* params, void* image, size_t image_bytes, void* stream);
size_t onssen_tasnet_workspace_bytes(const int32_t* cfg_host, int n, int S);
int onssen_tasnet_forward_f32(const int32_t* cfg_host, const void* image, const float* x, int n, int S, int64_t x_stride,
                              float* out, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Conv-TasNet forward over a RAGGED batch: n whole utterances of different lengths in one call.  cfg / image as above (the
 * same image, every norm, activation and precision).
 * lengths_host: n HOST int32 sample counts S_b, 1 <= n <= ONSSEN_TASNET_RAGGED_MAX.  x: row b holds utterance b at
 *   x + b * x_stride; samples at and beyond S_b are never read (nothing beyond S_out_b is).  Utterance b has
 *   T_b = (S_b - L) / (L/2) + 1 frames and S_out_b = (T_b - 1) L/2 + L output samples.
 * out: num_spks x n rows of out_stride floats, out_stride >= max S_out_b; row (s, b) holds the estimate in [0, S_out_b) and
 *   zeros in [S_out_b, out_stride): every float of out is written.
 * ws: onssen_tasnet_ragged_workspace_bytes(cfg, n, lengths_host) bytes, 256-byte aligned, no zeroing needed.  Activations are
 *   compact rows (M = sum T_b, no padded rows), so the size is that of the rectangular forward at the same number of rows and
 *   statistics chunks: for n = 1 it EQUALS onssen_tasnet_workspace_bytes(cfg, 1, S_0).
 * Row (s, b) is bit for bit what onssen_tasnet_forward_f32 gives for utterance b alone (n = 1, S = S_b): gLN statistics,
 *   the depthwise convolution's zero padding and the overlap-add stop at the utterance's own last frame.  The per-utterance
 *   table travels to the kernels by value as a kernel argument (hence the bound on n): no host synchronisation, no copy, no
 *   atomics; ordinary launches on `stream`.  A captured graph holds the table, so it is tied to the lengths it was captured with.
 * ONSSEN_E_ARG: n out of range, an S_b < L or > x_stride, out_stride < max S_out_b, sum T_b > 2^31 / 4. */
#define ONSSEN_TASNET_RAGGED_MAX 64
size_t onssen_tasnet_ragged_workspace_bytes(const int32_t* cfg_host, int n, const int32_t* lengths_host);
int onssen_tasnet_forward_ragged_f32(const int32_t* cfg_host, const void* image, const float* x, int n,
                                     const int32_t* lengths_host, int64_t x_stride, float* out, int64_t out_stride, void* ws,
                                     size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Conv-TasNet training: a forward that keeps what the backward needs, and the backward of the network (the gradient of every
 * packed parameter; none with respect to the waveform).  cfg / image / x / n / S / x_stride as above.  norm = BN (batch
 * statistics, running-statistics updates) is not offered: every entry point here answers it with ONSSEN_E_ARG (sizes: 0).
 * train_forward: the kernels and the arithmetic of onssen_tasnet_forward_f32 -- `out` is bit-identical to it at the same
 *   precision -- writing the block inputs, the conv1x1 outputs before PReLU, the norm statistics, the depthwise outputs, the
 *   encoder output, its LayerNorm, the mask logits and the masked encoder output into `saved`
 *   (onssen_tasnet_saved_bytes(cfg, n, S) bytes, 256-byte aligned, no zeroing needed); ws as for the forward.
 * backward: d_out = d(loss)/d(out), num_spks x n x S_out contiguous; d_params = onssen_tasnet_param_floats(cfg) floats in the
 *   order of `params`, every one of them written (not accumulated).  ws = onssen_tasnet_backward_workspace_bytes(cfg, n, S)
 *   bytes, 256-byte aligned, no zeroing needed; `saved` and `image` are what the training forward of the same x read and
 *   wrote.  Every contraction is exact fp32 whatever cfg's precision says (no bf16 product touches a gradient): input
 *   gradients are onssen_linear_f32 on the transposed weights, weight and bias gradients per-row-chunk partial sums merged in
 *   fp64 in a fixed order.  No atomics: two runs give the same bits.  Ordinary launches on `stream`, no allocation.
 * A too-small saved / ws returns ONSSEN_E_WORKSPACE before anything is launched or written. */
size_t onssen_tasnet_saved_bytes(const int32_t* cfg_host, int n, int S);
int onssen_tasnet_train_forward_f32(const int32_t* cfg_host, const void* image, const float* x, int n, int S, int64_t x_stride,
                                    float* out, void* saved, size_t saved_bytes, void* ws, size_t ws_bytes, void* stream);
size_t onssen_tasnet_backward_workspace_bytes(const int32_t* cfg_host, int n, int S);
int onssen_tasnet_backward_f32(const int32_t* cfg_host, const void* image, const float* x, int n, int S, int64_t x_stride,
                               const void* saved, size_t saved_bytes, const float* d_out, float* d_params, void* ws, size_t ws_bytes,
                               void* stream);

/* ---------------------------------------------------------------------------------------------
 * Conv-TasNet STREAMING inference: n concurrent streams of a causal model that advance in lockstep, all state on the device.
 * cfg / image as above.  Only causal = 1 with norm = CLN or BN can stream (gLN statistics span the utterance, a non-causal block
 * looks ahead), and the deepest block's history (P - 1) 2^(X - 1) must not exceed ONSSEN_TASNET_STREAM_MAX_HISTORY frames: any
 * other configuration gets ONSSEN_E_ARG (size queries: 0) and nothing is launched.  hop = L/2.
 * step: x_new = n rows of frames * hop NEW samples (row stride x_stride >= frames * hop floats); out = num_spks x n x
 *   (frames * hop), contiguous.  frames >= 1 may differ from call to call.  ws = onssen_tasnet_stream_workspace_bytes(cfg, n,
 *   frames) bytes, 256-byte aligned, no zeroing needed, free between steps.
 * Delay: exactly ONE hop.  A hop of samples completes the frame that began one hop earlier, so after a reset the first hop of
 *   output is exactly zero, and from there the concatenated step outputs hold the offline output blocks 0, 1, ...: for a stream
 *   that was reset, fed M hops in steps of any sizes and flushed, concat(steps)[hop:] followed by flush's hop is BIT FOR BIT
 *   onssen_tasnet_forward_f32 of the whole M * hop samples (S_out = S there), at every precision.  flush = the last block (the
 *   decoder bias + the second half of the last frame's taps; zeros while the stream holds no complete frame); it changes nothing,
 *   so the stream may go on.  Taps and overlap-add terms that reach before a stream's frame 0 contribute nothing (skipped, as the
 *   forward skips them: NOT a zero row through the normalisation).
 * state: onssen_tasnet_stream_state_bytes(cfg, n) bytes (0: n < 1, n > 65535 or the size overflows), 256-byte aligned, each
 *   region 256-aligned, in this order:
 *     int64 next_frame[n]                 index of the next frame of each stream; -1 after reset; advanced by the step itself
 *     float carry_x[n][hop]               the last hop of samples (first half of the next frame)
 *     float carry_dec[num_spks][n][hop]   second half of the last frame's decoder taps (before the bias)
 *     per block j = r * X + x, history = (P - 1) 2^x frames:
 *       float ring[n][history][H]         conv1x1 + PReLU output of the last `history` frames; frame g in slot (g + 1) mod history
 *       float stat[n][history][2]         their cLN (mean, rstd) (unused under BN)
 *   (recipe N 512, H 512, P 3, X 8, R 3: 3 * 510 rows of 512 + 2 floats per stream, 3.1 MB.)
 *   reset: slots_host = n_slots HOST stream indices in [0, n) (NULL, 0: all); zeroes every byte of those streams' state and sets
 *   their counters to -1, whatever the buffer held; the other streams are untouched.  A new state buffer must be reset once.
 * The frame counters live on the device and no argument but the pointers changes from step to step, so ONE captured graph of a
 *   step serves every later step of the same (n, frames).  No launch writes a state row that another workgroup of the same
 *   launch reads (the history ring is written by a launch of its own after its readers).  No atomics, no spinning, no
 *   allocation; ordinary launches on `stream`; two runs give the same bits.
 * ONSSEN_E_ARG: a configuration that cannot stream, n < 1, frames < 1, n * frames > 2^31 / 4, x_stride < frames * hop, a slot
 *   outside [0, n).  ONSSEN_E_WORKSPACE: state_bytes or ws_bytes too small.  Both before anything is launched or written. */
#define ONSSEN_TASNET_STREAM_RESET_MAX 64          /* slots per round of reset launches (internal batching; any n_slots works) */
#define ONSSEN_TASNET_STREAM_MAX_HISTORY 16777216  /* frames */
size_t onssen_tasnet_stream_state_bytes(const int32_t* cfg_host, int n);
int onssen_tasnet_stream_reset(const int32_t* cfg_host, void* state, size_t state_bytes, int n, const int32_t* slots_host,
                               int n_slots, void* stream);
size_t onssen_tasnet_stream_workspace_bytes(const int32_t* cfg_host, int n, int frames);
int onssen_tasnet_stream_step_f32(const int32_t* cfg_host, const void* image, const float* x_new, int n, int frames,
                                  int64_t x_stride, float* out, void* state, size_t state_bytes, void* ws, size_t ws_bytes,
                                  void* stream);
int onssen_tasnet_stream_flush_f32(const int32_t* cfg_host, const void* image, const void* state, size_t state_bytes, int n,
                                   float* out_tail, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Conv-TasNet LONG-FORM separation: a recording cut into K windows of W samples that start `step` samples apart (overlap
 * O = W - step), each separated on its own by the forward above, and the window estimates put back together on the device.
 * windows: x = S samples -> win = K rows of W floats (contiguous), row k = x[k step, k step + W) with zeros past S;
 *   (K - 1) step < S.  The forward takes rows at least S apart, so overlapping windows cannot be a strided view of x.
 * stitch: est = C x K x W window estimates (contiguous; speaker-major as the forward writes them), all windows full but the last,
 *   which holds v_last valid samples (what lies beyond is never read); out = C x S_out, S_out = (K - 1) step + v_last;
 *   perm_out = K x C int32, perm_out[k][c] = the row of window k that carries output channel c (perm_out[0] = identity).
 *   Geometry: 1 <= C <= 4, K >= 1, 1 <= O <= W / 2 (at most two windows cover a sample), O < v_last <= W (every consecutive
 *   pair overlaps in exactly O samples).  Per pair (k - 1, k): sim[i][j] = sum_t est[i][k-1][step + t] est[j][k][t] over
 *   t in [0, O), fp64, a fixed order; the permutation pi maximising sum_i sim[i][pi(i)], scanned in lexicographic order, first
 *   maximum wins (an all-silent overlap gives the identity); perm[k][c] = pi_k(perm[k-1][c]).  out[c][t] is a copy where one
 *   window covers t; on an overlap, j samples into it, w_old a + w_new b with w_new = (j + 0.5) / O, w_old = 1 - w_new, a / b
 *   the older / newer window's rows perm[k-1][c] / perm[k][c].
 *   ws = onssen_tasnet_stitch_workspace_bytes(C, K, W, step, v_last) bytes (0: a refused geometry), 16-byte aligned, no zeroing
 *   needed.  Nothing is read back by the host: three ordinary launches on `stream`, no atomics, two runs give the same bits.
 * ONSSEN_E_ARG: a null pointer or a violated geometry; ONSSEN_E_WORKSPACE: ws_bytes too small; ONSSEN_E_ALIGN: ws; all before
 *   anything is launched or written. */
int onssen_tasnet_windows_f32(const float* x, int64_t S, int K, int W, int step, float* win, void* stream);
size_t onssen_tasnet_stitch_workspace_bytes(int C, int K, int W, int step, int v_last);
int onssen_tasnet_stitch_f32(const float* est, int C, int K, int W, int step, int v_last, float* out, int32_t* perm_out, void* ws,
                             size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Sample-rate conversion of the file loaders, csrc/resample.inc: scipy.signal.resample_poly(x, up, down) with its default
 * window, over a ragged batch, in one launch.  up = rate_out / g, down = rate_in / g (g their gcd; every entry reduces the pair
 * it is given), M = max(up, down) <= 2048, half = 10 M, taps h[0 .. 2 half]:
 *   g[k] = sinc((k - half) / M) I0(5 sqrt(1 - ((k - half) / half)^2)) / I0(5),  h = up g / sum g,  sinc(t) = sin(pi t) / (pi t)
 *   n_out = ceil(n_in up / down),  y[m] = sum_n x[n] h[m down - n up + half] over the n in [0, n_in) whose tap index is in range.
 *   Equal rates are the identity: half = 0 and the one tap 1.0 (resample_poly returns a copy).
 * onssen_resample_geometry: the reduced pair, half and n_out of (rate_in, rate_out, n_in); outputs may be NULL.  Host only.
 * onssen_resample_taps_f64: the 2 half + 1 taps into HOST memory, fp64, computed by the library (no SciPy behind the C ABI).
 * onssen_resample_workspace_bytes / onssen_resample_prepare: the device image of the taps, phase-major -- up rows of
 *   L = ceil((2 half + 1) / up) fp64 values, row p = h[p], h[p + up], ... (0 beyond 2 half), so that one output reads its L taps
 *   contiguously -- into caller-owned, 16-byte aligned device memory.  prepare computes on the host and copies with a BLOCKING
 *   copy: once per ratio, outside any graph capture; `stream` is unused.
 * onssen_resample_f32: x = B rows stride_in floats apart, row b holding lengths_in[b] <= n_in samples (lengths_in NULL: n_in
 *   each; device int32 values, clamped to [0, n_in]); sub (nullable, laid out like x): the filter's input is x - sub, formed in
 *   fp64 on load (onssen/data/feature_utils.py:24-33, get_stft_from_subtraction, in the same pass).  y = B rows stride_out
 *   floats apart: row b gets ceil(lengths_in[b] up / down) samples and ZEROS from there to stride_out; lengths_out (nullable,
 *   device int32, B values) receives that count.  Nothing at or beyond lengths_in[b] is read.  Products and sum in fp64 in a
 *   fixed order, one rounding to fp32 at the store, no atomics: bit-repeatable, and a row's output is bit for bit that of a
 *   batch-1 call on it.  Index arithmetic is 64-bit (m down may pass 2^31).  One launch on `stream`: nothing is allocated, nothing
 *   synchronises, capturable into a graph.  ws: what onssen_resample_prepare filled for the same ratio.
 * ONSSEN_E_ARG, before anything is launched or written: up or down < 1, a reduced up or down above 2048, a NULL x / y / ws,
 *   B outside 1 .. 65535, n_in < 1, stride_in < n_in, stride_out < ceil(n_in up / down), ws_bytes below
 *   onssen_resample_workspace_bytes (which is 0 for a refused ratio).  ONSSEN_E_ALIGN: ws not 16-byte aligned. */
int onssen_resample_geometry(int rate_in, int rate_out, int64_t n_in, int* up, int* down, int* half, int64_t* n_out);
int onssen_resample_taps_f64(int up, int down, double* taps_host);
size_t onssen_resample_workspace_bytes(int up, int down);
int onssen_resample_prepare(int up, int down, void* ws, size_t ws_bytes, void* stream);
int onssen_resample_f32(const float* x, const float* sub, int64_t stride_in, const int32_t* lengths_in, int B, int n_in, int up,
                        int down, float* y, int64_t stride_out, int32_t* lengths_out, const void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ONSSEN_HIP_H */
