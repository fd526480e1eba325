// libonssen_hip.so -- hand-written HIP kernels for gfx950 (MI355X / CDNA4) behind the C ABI of
// include/onssen_hip.h.  See DESIGN.md for the data layouts and the per-kernel rooflines.
//
// Kernel inventory (one translation unit, the parts are the .inc files next to this one):
//   fft.inc             stft_logmag_kernel (K1+K2: fp64 radix-4 FFT in LDS, one wavefront per PAIR of frames, fused log10(|X|+eps)),
//                       mask_istft_kernel (K10: mask-apply + fp64 inverse FFT, two speakers per transform, gather overlap-add;
//                       with its phase flag the operand is mask * |X| * the network's phase estimate: onssen_phase_istft_f32)
//   misi.inc            misi_phase_kernel (MISI phase reconstruction: mixture + C estimates -> residual spread over the speakers, fp64
//                       STFT of two speakers per transform, Z / |Z|: the phase maps of the next onssen_phase_istft_f32)
//   istft_bwd.inc       istft_bwd_kernel (waveform-approximation training: the adjoint of mask_istft_kernel in its three modes -- windowed
//                       fp64 forward transform of the waveform gradient, two speakers per transform, gradients of masks / phases / magnitudes)
//   misi_bwd.inc        misi_bwd_frames_kernel / misi_bwd_gather_kernel (unfolded MISI training: the adjoint of misi_phase_kernel -- forward
//                       transform, Z / |Z| Jacobian and inverse transform per frame in one LDS buffer, then the overlap-add with the
//                       reflect padding folded back and the residual adjoint)
//   gemm.inc            linear_x3q_kernel (K3/K7/K8/K9 on pre-split bf16 images: 256|128 x 320|256 tiles staged by LDS-DMA into a swizzled
//                       layout, 8 waves, register epilogues), linear_x3p_kernel (round-1 form: 256x160 tiles; batched weight gradients;
//                       bias | sigmoid | grouped L2-norm), linear_x3_kernel / linear_kernel (fp32-A forms, exact-fp32 MFMA),
//                       x3_image(_t)_kernel (fp32 -> split-bf16 operand images)
//   gemm_run.inc        host code: the GEMMs' argument filler, tile chooser, dispatchers, environment switches and C ABI entries
//   lstm.inc            lstm_xcd_kernel (K4, default: XCD-local persistent recurrence, ONE launch per layer, data-tagged h
//                       exchange through the XCD's L2; split-bf16 / bf16 / exact-fp32 instantiations), lstm_step_kernel (one
//                       launch per time step: H > 640 and the re-run of an aborted call)
//   lstm_bwd.inc        lstm_xcd_bwd_kernel / lstm_bwd_step_kernel (training: backward recurrence)
//   lstm_run.inc        host code: the BLSTM's geometry, workspace layouts, launchers and C ABI entries (forward, pipelined pair, training)
//   labels_cluster.inc  labels_kernel (training labels), kmeans2_* (deep-clustering back end: compaction of the active bins, all
//                       Lloyd iterations in one persistent launch with register-resident rows; launch-per-iteration fallback)
//   kmeans_k.inc        kmeansk_* (the same back end for 2 .. 4 speakers: farthest-point initialisation, launch-per-iteration Lloyd,
//                       K-channel masks)
//   pit.inc             shared by the time-domain PIT losses: row chunks, 4-float loads, the permutation enumerator, pit_total_kernel
//   loss_dc.inc         loss_dc_* (deep-clustering loss: value and gradient), dc_head_grad_images_kernel (that gradient as fc_dc's operands)
//   batch_sdr.inc       sdr_* (batch SI-SDR with best permutation, fp64 sums)
//   loss_mask.inc      loss_mask_* (chimera mask term: value, winning assignment, gradient)
//   loss_sisnr.inc      sisnr_* (Conv-TasNet's SI-SNR permutation-invariant training loss: value, assignment, gradient; fp64 moments)
//   loss_phase.inc      loss_phase_* (phase_net's training loss: mask term and cosine phase term in one pass, assignment, gradient)
//   enhance.inc         labels_enhance_kernel (|X|, |S|, cos of the phase difference in one pass), loss_enhance_* (the MSA / PSA
//                       enhancement losses: value and gradient); the reconstruction is mask_istft_kernel's magnitude mode (fft.inc)
//   loss_upit.inc       loss_upit_* (the uPIT mask network's loss for 2 .. 4 speakers: pair sums in one pass, assignment scan, gradient)
//   loss_wa.inc         wa_* (waveform-approximation training: L1 waveform distance under the best speaker permutation, fp64 sums in
//                       one pass, assignment scan, sign gradient)
//   resample.inc        resample_kernel (the loaders' sample-rate conversion: scipy's resample_poly as a polyphase filter over a ragged batch,
//                       the tile's input span staged in the LDS as fp64, optional subtraction of a second signal on load)
//   pack.inc            one-off weight re-layout (gate permutation, MFMA fragment order, BatchNorm fold); training glue: dropout,
//                       row-wise L2 normalisation and train-mode BatchNorm with their backward passes
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "../../include/onssen_hip.h"

typedef float f32x4 __attribute__((vector_size(16)));
typedef unsigned int u32x4 __attribute__((vector_size(16)));
typedef unsigned int u32x2 __attribute__((vector_size(8)));
typedef short s16x8 __attribute__((vector_size(16)));       // 8 bf16 bit patterns = one MFMA A/B fragment
typedef __bf16 bf16x8_t __attribute__((vector_size(16)));

// Opaque to the optimiser: the first use of `x` cannot be scheduled (or folded into another block) before `after` exists.
// (The host-side emulation of tests/emu defines ONSSEN_HOST_EMULATION: no such reordering there, and no VGPR constraints.)
#ifdef ONSSEN_HOST_EMULATION
#define ONSSEN_USE_AFTER(x, after) ((void)0)
#define ONSSEN_LDS_PTR(p) ((void*)(p))
#else
#define ONSSEN_USE_AFTER(x, after) asm volatile("" : "+v"(x) : "v"(after))
#define ONSSEN_LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))     // LDS pointer for buffer_load ... lds
#endif

// ---- split-bf16 ("bf16x3") arithmetic ---------------------------------------------------------------
// An fp32 value x is carried as hi = bf16(x), lo = bf16(x - hi) (|x - hi - lo| <= 2^-17 |x|).  A product
// a*b is evaluated as a_hi*b_hi + a_hi*b_lo + a_lo*b_hi on the bf16 MFMA pipe (each bf16 x bf16 product
// is exact in fp32; accumulation is fp32), dropping only a_lo*b_lo ~ 2^-16 |ab|.  That keeps dot products
// at ~1e-5 relative -- inside the 1e-4 parity budget -- at 3/16 of the exact-fp32 MFMA time.
__device__ __forceinline__ void split_bf16(float x, unsigned short& hi, unsigned short& lo) {
  const __hip_bfloat16 h = __float2bfloat16(x);
  const __hip_bfloat16 l = __float2bfloat16(x - __bfloat162float(h));
  hi = __builtin_bit_cast(unsigned short, h);
  lo = __builtin_bit_cast(unsigned short, l);
}
__device__ __forceinline__ f32x4 mfma_bf16(s16x8 a, s16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0,
                                                 0, 0);
}

// gfx950's transposing LDS read (ds_read_b64_tr_b16): every lane supplies the address of FOUR consecutive 16-bit elements; inside a
// 16-lane group, lane c receives element c % 4 of the rows addressed by lanes 4 j + c / 4, j = 0..3 (measured:
// tools/micro/tr16_probe.hip).  With the lanes of a group addressing a [4 k][16 m] block row by row, lane c gets column c of
// the block: four consecutive k of one m -- half an MFMA fragment from a tile that was stored as it came from memory.
typedef short s16x4 __attribute__((vector_size(8)));
#ifdef ONSSEN_HOST_EMULATION
__device__ __forceinline__ s16x4 lds_read_tr16(const unsigned short* p) { return emu_ds_read_tr16_b64(p); }
#else
__device__ __forceinline__ s16x4 lds_read_tr16(const unsigned short* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)p);
}
#endif

// the sum of v over the 64 lanes of a wave, in every lane
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// hipGetLastError() is sticky per thread: other libraries' failed probes (e.g. a device query before
// the runtime is initialised) linger.  Every ABI entry clears it first, then checks its own launches.
#define ONSSEN_CLEAR_ERROR() ((void)hipGetLastError())
#define ONSSEN_LAUNCH_CHECK()                   \
  do {                                          \
    hipError_t e__ = hipGetLastError();         \
    if (e__ != hipSuccess) return (int)e__;     \
  } while (0)

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
// grid of an element-wise kernel: one 256-thread workgroup per 256 elements, 8192 at the most (the kernels stride over the rest)
static unsigned ew_blocks(long total) { const long nb = (total + 255) / 256; return (unsigned)(nb > 8192 ? 8192 : nb); }
// Experiment / ablation switches exist only in builds made with -DONSSEN_DEBUG_KNOBS (tools/ab_variants.py): the product
// library reads no environment variable for them and carries their defaults as constants.
#ifdef ONSSEN_DEBUG_KNOBS
#define ONSSEN_KNOB_INT(name, dflt) (getenv(name) ? atoi(getenv(name)) : (dflt))
#else
#define ONSSEN_KNOB_INT(name, dflt) (dflt)
#endif
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static inline bool aligned256(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 255u) == 0; }

// Bounded waits of the persistent kernels: ~0.2 s of polling on the GPU by default.  A run-time setting of the library
// (onssen_xcd_spin_limit), initialised from ONSSEN_XCD_SPIN_LIMIT: the host-side emulation -- where a 'workgroup' is a
// process at the mercy of the OS scheduler -- and data-parallel training -- where a co-tenant RCCL kernel may hold CUs
// while it waits for a slower rank -- raise it; 0 makes every wait give up at once (abort-path tests).
static unsigned& xcd_spin_limit() {
  static unsigned v = getenv("ONSSEN_XCD_SPIN_LIMIT") ? (unsigned)strtoul(getenv("ONSSEN_XCD_SPIN_LIMIT"), nullptr, 10) : 400000u;
  return v;
}

// ---- device code, one translation unit (the host-side emulation compiles exactly this file too)
#include "pack.inc"
#include "gemm.inc"
#include "gemm_run.inc"    // GEMM host side: argument filler, tile chooser, dispatchers, environment switches and the C ABI entries over gemm.inc
#include "labels_cluster.inc"
#include "kmeans_k.inc"     // deep-clustering back end for 2 .. 4 speakers: its kernels and its C ABI entries
#include "dc_run.inc"       // deep-clustering 2-means host side: one workspace layout, one Lloyd launcher, the C ABI entries over labels_cluster.inc
#include "lstm.inc"
#include "lstm_bwd.inc"
#include "lstm_run.inc"    // BLSTM host side: geometry, workspace layouts, launchers and the C ABI entries over lstm.inc / lstm_bwd.inc
#include "fft.inc"
#include "misi.inc"       // MISI phase reconstruction: the half-step between two inverse transforms (estimates -> phase maps)
#include "istft_bwd.inc"  // waveform-approximation training: the adjoint of mask_istft_kernel, all three modes
#include "misi_bwd.inc"   // unfolded MISI training: the adjoint of misi_phase_kernel (phase-map gradients -> estimate gradients)
#include "pit.inc"        // permutation-invariant losses: the shared geometry, loads, permutation enumerator, sums and host helpers
#include "loss_dc.inc"    // deep-clustering loss and its gradient: its kernels and its C ABI entries
#include "batch_sdr.inc"  // batch SI-SDR with best permutation: its kernels and its C ABI entries
#include "loss_mask.inc"  // chimera training: the mask-inference term (better of the two speaker assignments) and its gradient
#include "wav_io.inc"      // host code: the batch RIFF reader of the file loader
#include "optim.inc"
#include "tasnet.inc"     // Conv-TasNet forward: its kernels and its C ABI entries
#include "tasnet_bwd.inc" // Conv-TasNet training: the saving forward and the backward
#include "tasnet_stream.inc" // Conv-TasNet streaming inference: stateful steps of causal models
#include "tasnet_stitch.inc" // Conv-TasNet long-form separation: window gather, permutation alignment, cross-fade
#include "tasnet_run.inc" // Conv-TasNet: the one launch sequence behind the eval, ragged, training and stream entries
#include "loss_sisnr.inc" // Conv-TasNet training: the SI-SNR permutation-invariant loss and its gradient
#include "loss_phase.inc" // phase_net training: mask term + phase term of loss_phase in one pass, and their gradient
#include "enhance.inc"    // speech enhancement: training labels, the MSA / PSA losses and their gradient
#include "loss_upit.inc"  // uPIT training: the utterance-level permutation-invariant mask loss for 2 .. 4 speakers and its gradient
#include "resample.inc"   // file loaders: polyphase sample-rate conversion (scipy.signal.resample_poly) of a ragged batch
#include "loss_wa.inc"    // waveform-approximation training: the L1 permutation-invariant waveform loss and its gradient

// Co-tenant probe (tools/cotenant_probe.py): `workgroups` workgroups of `threads` threads that do nothing but hold their
// CU for `ticks` ticks of the 100 MHz wall clock -- a stand-in for RCCL's channel kernels next to the persistent recurrences.
// NV live VGPRs per lane and LDS bytes decide whether such a workgroup can share a CU with a recurrence
// workgroup (2 waves x ~216 VGPRs per SIMD and ~114 KB of LDS leave ~80 VGPRs per SIMD and ~46 KB): the light form can,
// the heavy form (>= 100 VGPRs, like a collective's unrolled copy loops) needs a CU of its own.
template <int NV, int LDS>
__global__ __launch_bounds__(1024) void cotenant_spin_kernel(long long ticks, float* sink) {
  __shared__ char cotenant_lds[LDS];
  float v[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = (float)(threadIdx.x + i);
  const long long t0 = wall_clock64();
  for (long long it = 0; it < ticks && wall_clock64() - t0 < ticks; ++it) {   // (bounded by count too)
    __builtin_amdgcn_s_sleep(32);
#ifndef ONSSEN_HOST_EMULATION
#pragma unroll
    for (int i = 0; i < NV; ++i) asm volatile("" : "+v"(v[i]));                // keeps every value in a register across the loop
#endif
  }
  if (sink) {                                                                    // never taken by the probe: keeps v and the LDS alive
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) acc += v[i];
    cotenant_lds[threadIdx.x * 31 % LDS] = (char)acc;
    sink[threadIdx.x] = acc + (float)cotenant_lds[(threadIdx.x + 1) * 31 % LDS];
  }
}

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" {

long long onssen_xcd_spin_limit(long long new_limit) {
  const long long old = (long long)xcd_spin_limit();
  if (new_limit >= 0) xcd_spin_limit() = new_limit > 0xffffffffLL ? 0xffffffffu : (unsigned)new_limit;
  return old;
}

int onssen_debug_cotenant_spin(int workgroups, int threads, long long ticks, int heavy, void* stream) {
  if (workgroups <= 0 || threads <= 0 || threads > 1024 || ticks < 0) return ONSSEN_E_ARG;
  ONSSEN_CLEAR_ERROR();
  if (heavy)
    hipLaunchKernelGGL((cotenant_spin_kernel<112, 32768>), dim3((unsigned)workgroups), dim3((unsigned)threads), 0,
                       (hipStream_t)stream, ticks, (float*)nullptr);
  else
    hipLaunchKernelGGL((cotenant_spin_kernel<2, 64>), dim3((unsigned)workgroups), dim3((unsigned)threads), 0,
                       (hipStream_t)stream, ticks, (float*)nullptr);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_debug_launch_chain(float* scratch, int n, int workgroups, void* stream) {
  if (!scratch || n <= 0 || workgroups <= 0) return ONSSEN_E_ARG;
  ONSSEN_CLEAR_ERROR();
  for (int i = 0; i < n; ++i)
    hipLaunchKernelGGL(probe_kernel, dim3((unsigned)workgroups), dim3(256), 0, (hipStream_t)stream, scratch);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_abi_version(void) { return ONSSEN_ABI_VERSION; }

const char* onssen_error_string(int code) {
  switch (code) {
    case ONSSEN_OK: return "ok";
    case ONSSEN_E_ARG: return "onssen: invalid argument or unsupported shape";
    case ONSSEN_E_WORKSPACE: return "onssen: workspace too small";
    case ONSSEN_E_ALIGN: return "onssen: pointer or stride alignment requirement violated";
    case ONSSEN_WAV_E_OPEN: return "onssen: wav file could not be opened";
    case ONSSEN_WAV_E_FORMAT: return "onssen: not a RIFF/WAVE file, or malformed";
    case ONSSEN_WAV_E_UNSUPPORTED: return "onssen: wav sample format not supported (PCM 8/16/24/32-bit, IEEE float 32/64)";
    case ONSSEN_WAV_E_SOME_FAILED: return "onssen: at least one file of the batch failed (see the per-file status)";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "onssen: unknown error";
  }
}

static int stft_logmag_impl(const float* wav, int B, int n_samples, int64_t wav_stride, int n_fft, int hop, float eps,
                            float* logmag, float* stft_ri, void* stream, const int32_t* n_per_utt) {
  if (!wav || !logmag || B <= 0 || hop <= 0 || n_samples <= n_fft / 2) return ONSSEN_E_ARG;
  ONSSEN_CLEAR_ERROR();
  const int T = 1 + n_samples / hop;
  if (stft_ri && (reinterpret_cast<uintptr_t>(stft_ri) & 7u)) return ONSSEN_E_ALIGN;     // (re, im) pairs are stored as one 8-byte word
  // one wave per PAIR of consecutive frames of an utterance (one complex transform), `ppw` consecutive pairs per wave: the
  // per-lane constants of the transform are built once per wave and the next pair's samples are fetched under this pair's
  // butterflies; fewer pairs per wave when that leaves CUs without a workgroup
  static const int ppw_knob = ONSSEN_KNOB_INT("ONSSEN_STFT_PPW", 4);      // debug builds: tools/ab_variants.py
  const int npair = (T + 1) / 2;
  int ppw = ppw_knob < 1 ? 1 : ppw_knob;
  while (ppw > 1 && (long)B * ceil_div(npair, 4 * ppw) < 512) --ppw;
  const dim3 grid((unsigned)((long)B * ceil_div(npair, 4 * ppw))), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (n_fft == 256)
    hipLaunchKernelGGL((stft_logmag_kernel<256>), grid, block, 0, st, wav, n_samples, (long)wav_stride, hop, T, eps, ppw,
                       logmag, stft_ri, n_per_utt);
  else if (n_fft == 512)
    hipLaunchKernelGGL((stft_logmag_kernel<512>), grid, block, 0, st, wav, n_samples, (long)wav_stride, hop, T, eps, ppw,
                       logmag, stft_ri, n_per_utt);
  else if (n_fft == 1024)
    hipLaunchKernelGGL((stft_logmag_kernel<1024>), grid, block, 0, st, wav, n_samples, (long)wav_stride, hop, T, eps, ppw,
                       logmag, stft_ri, n_per_utt);
  else
    return ONSSEN_E_ARG;
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_stft_logmag_f32(const float* wav, int B, int n_samples, int64_t wav_stride, int n_fft, int hop, float eps,
                           float* logmag, float* stft_ri, void* stream) {
  return stft_logmag_impl(wav, B, n_samples, wav_stride, n_fft, hop, eps, logmag, stft_ri, stream, nullptr);
}

int onssen_stft_logmag_ragged_f32(const float* wav, int B, int n_max, int64_t wav_stride, const int32_t* n_per_utt, int n_fft,
                                  int hop, float eps, float* logmag, float* stft_ri, void* stream) {
  if (!n_per_utt) return ONSSEN_E_ARG;
  return stft_logmag_impl(wav, B, n_max, wav_stride, n_fft, hop, eps, logmag, stft_ri, stream, n_per_utt);
}

int onssen_lstm_pack_whh_bf16x3(const float* w_hh, int H, int ug, uint16_t* whh_x3, void* stream) {
  int Hp, KQ2;
  int64_t we;
  if (!w_hh || !whh_x3 || onssen_lstm_geometry(H, ug, &Hp, nullptr, nullptr, nullptr) != ONSSEN_OK ||
      onssen_lstm_geometry_x3(H, ug, &KQ2, nullptr, &we) != ONSSEN_OK)
    return ONSSEN_E_ARG;
  if (!aligned16(whh_x3)) return ONSSEN_E_ALIGN;      // 16-byte stores (one fragment lane's 8 values per half)
  ONSSEN_CLEAR_ERROR();
  const long n = we / 16;
  hipLaunchKernelGGL(pack_whh_bf16x3_kernel, dim3((unsigned)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256)),
                     dim3(256), 0, (hipStream_t)stream, w_hh, H, Hp, ug, KQ2, H, whh_x3);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}
int onssen_lstm_pack_wih_bf16x3(const float* w_ih, int in_dim, int H, int ug, uint16_t* wih_x3, void* stream) {
  int Hp;
  if (!w_ih || !wih_x3 || in_dim <= 0 || onssen_lstm_geometry(H, ug, &Hp, nullptr, nullptr, nullptr) != ONSSEN_OK)
    return ONSSEN_E_ARG;
  if (!aligned16(wih_x3)) return ONSSEN_E_ALIGN;
  ONSSEN_CLEAR_ERROR();
  const int KC = ceil_div(in_dim, 32);
  const long n = (long)(Hp / ug) * KC * (ug / 4) * 64;
  hipLaunchKernelGGL(pack_whh_bf16x3_kernel, dim3((unsigned)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256)),
                     dim3(256), 0, (hipStream_t)stream, w_ih, H, Hp, ug, KC, in_dim, wih_x3);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_lstm_pack_f32(const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int in_dim,
                         int bidir_in, int H, int ug, float* wih_p, float* whh_p, float* bias_p, void* stream) {
  int Hp, NP, KQ;
  int64_t we;
  if (onssen_lstm_geometry(H, ug, &Hp, &NP, &KQ, &we) != ONSSEN_OK) return ONSSEN_E_ARG;
  if (!w_ih || !w_hh || !b_ih || !b_hh || !wih_p || !whh_p || !bias_p || in_dim <= 0) return ONSSEN_E_ARG;
  if (bidir_in && in_dim != 2 * H) return ONSSEN_E_ARG;
  const int Kp = bidir_in ? 2 * Hp : ceil_div(in_dim, 4) * 4;
  hipStream_t st = (hipStream_t)stream;
  ONSSEN_CLEAR_ERROR();
  const long n1 = (long)NP * Kp;
  hipLaunchKernelGGL(pack_wih_kernel, dim3((unsigned)((n1 + 255) / 256 > 4096 ? 4096 : (n1 + 255) / 256)), dim3(256),
                     0, st, w_ih, b_ih, b_hh, in_dim, bidir_in, H, Hp, ug, Kp, wih_p, bias_p);
  ONSSEN_LAUNCH_CHECK();
  hipLaunchKernelGGL(pack_whh_kernel, dim3((unsigned)((we + 255) / 256 > 4096 ? 4096 : (we + 255) / 256)), dim3(256),
                     0, st, w_hh, H, Hp, ug, KQ, whh_p);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_lstm_pack_wih_image_f32(const float* w_ih, const float* b_ih, const float* b_hh, int in_dim, int bidir_in, int H, int ug,
                                   float* wih_p, float* bias_p, uint16_t* wih_img, void* stream) {
  int Hp, NP;
  if (onssen_lstm_geometry(H, ug, &Hp, &NP, nullptr, nullptr) != ONSSEN_OK) return ONSSEN_E_ARG;
  if (!w_ih || !b_ih || !b_hh || !wih_p || !bias_p || !wih_img || in_dim <= 0) return ONSSEN_E_ARG;
  if (bidir_in && in_dim != 2 * H) return ONSSEN_E_ARG;
  if (!aligned16(wih_img)) return ONSSEN_E_ALIGN;
  const int Kp = bidir_in ? 2 * Hp : ceil_div(in_dim, 4) * 4, K = bidir_in ? 2 * Hp : in_dim, KB = ceil_div(K, 32);
  ONSSEN_CLEAR_ERROR();
  const long n = (long)NP * KB * 4;
  hipLaunchKernelGGL(pack_wih_image_kernel, dim3((unsigned)((n + 255) / 256 > 16384 ? 16384 : (n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, w_ih, b_ih, b_hh, in_dim, bidir_in, H, Hp, ug, Kp, K, KB, wih_p, bias_p, wih_img);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_head_pack_f32(const float* w, const float* b, int N, int H, int Hp, const float* bn_gamma,
                         const float* bn_beta, const float* bn_mean, const float* bn_var, float bn_eps, float* w_p,
                         float* b_p, void* stream) {
  if (!w || !b || !w_p || !b_p || N <= 0 || H <= 0 || Hp < H || (Hp % 4) != 0) return ONSSEN_E_ARG;
  if (bn_gamma && (!bn_beta || !bn_mean || !bn_var)) return ONSSEN_E_ARG;
  ONSSEN_CLEAR_ERROR();
  hipLaunchKernelGGL(pack_head_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, w, b, N, H, Hp,
                     bn_gamma, bn_beta, bn_mean, bn_var, bn_eps, w_p, b_p);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

// ---- training: weight images for the backward recurrence (the training forward and the backward itself: lstm_run.inc) ----
int64_t onssen_lstm_whhT_elems(int H, int ug) {
  int Hp, NP, KQB, NUB;
  if (!lstm_bwd_geometry(H, ug, &Hp, &NP, &KQB, &NUB)) return 0;
  return (int64_t)NUB * KQB * 1024;
}

int onssen_lstm_pack_whhT_bf16x3(const float* w_hh, int H, int ug, uint16_t* out, void* stream) {
  int Hp, NP, KQB, NUB;
  if (!w_hh || !out || !lstm_bwd_geometry(H, ug, &Hp, &NP, &KQB, &NUB)) return ONSSEN_E_ARG;
  ONSSEN_CLEAR_ERROR();
  const long n = (long)NUB * KQB * 512;
  hipLaunchKernelGGL(pack_whhT_bf16x3_kernel, dim3((unsigned)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, w_hh, H, Hp, ug, KQB, NUB, out);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int64_t onssen_lstm_whhR_elems(int H, int ug) {
  int Hp, NP, KQB, NUB;
  if (!lstm_bwd_geometry(H, ug, &Hp, &NP, &KQB, &NUB)) return 0;
  return (int64_t)(Hp / ug) * ceil_div(4 * ug, 32) * NUB * 1024;
}

int onssen_lstm_pack_whhR_bf16x3(const float* w_hh, int H, int ug, uint16_t* out, void* stream) {
  int Hp, NP, KQB, NUB;
  if (!w_hh || !out || !lstm_bwd_geometry(H, ug, &Hp, &NP, &KQB, &NUB)) return ONSSEN_E_ARG;
  if (!aligned16(out)) return ONSSEN_E_ALIGN;
  ONSSEN_CLEAR_ERROR();
  const int KC = ceil_div(4 * ug, 32);
  const long n = (long)(Hp / ug) * KC * NUB * 64;
  hipLaunchKernelGGL(pack_whhR_bf16x3_kernel, dim3((unsigned)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, w_hh, H, Hp, ug, KC, NUB, out);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_lstm_pack_train_f32(int L, int in_dim, int H, int ug, const float* const* w_ih_host, const float* const* w_hh_host,
                               const float* const* b_ih_host, const float* const* b_hh_host, float* const* wih_p_host,
                               float* const* bias_p_host, uint16_t* const* wih_img_host, uint16_t* const* whh_x3_host,
                               uint16_t* const* whhR_host, void* stream) {
  int Hp, NP, KQB, NUB, KQ2;
  if (L <= 0 || in_dim <= 0 || !w_ih_host || !w_hh_host || !b_ih_host || !b_hh_host || !wih_p_host || !bias_p_host || !wih_img_host ||
      !whh_x3_host || !lstm_bwd_geometry(H, ug, &Hp, &NP, &KQB, &NUB) || onssen_lstm_geometry_x3(H, ug, &KQ2, nullptr, nullptr) != ONSSEN_OK)
    return ONSSEN_E_ARG;
  for (int i = 0; i < 2 * L; ++i)
    if (!w_ih_host[i] || !w_hh_host[i] || !b_ih_host[i] || !b_hh_host[i] || !wih_p_host[i] || !bias_p_host[i] || !wih_img_host[i] ||
        !whh_x3_host[i] || !aligned16(wih_img_host[i]) || !aligned16(whh_x3_host[i]) ||
        (whhR_host && (!whhR_host[i] || !aligned16(whhR_host[i]))))
      return ONSSEN_E_ARG;
  ONSSEN_CLEAR_ERROR();
  const int per = whhR_host ? 3 : 2, group = packt::MAXJ / per;       // (layer, direction) pairs per launch
  auto blocks = [](long n) { const long b = (n + 255) / 256; return (int)(b > 2048 ? 2048 : b); };
  for (int i0 = 0; i0 < 2 * L; i0 += group) {
    PackTrainArgs a;
    a.H = H; a.Hp = Hp; a.UG = ug; a.KQ2 = KQ2; a.KC = ceil_div(4 * ug, 32); a.NTB = NUB; a.njobs = 0;
    int fb = 0;
    for (int i = i0; i < 2 * L && i < i0 + group; ++i) {
      const int l = i / 2, bidir = l > 0;
      const int ind = bidir ? 2 * H : in_dim, Kp = bidir ? 2 * Hp : ceil_div(in_dim, 4) * 4, K = bidir ? 2 * Hp : in_dim, KB = ceil_div(K, 32);
      PackJob j{};
      j.w = w_ih_host[i]; j.b_ih = b_ih_host[i]; j.b_hh = b_hh_host[i]; j.wih_p = wih_p_host[i]; j.bias_p = bias_p_host[i];
      j.out = wih_img_host[i]; j.type = 0; j.in_dim = ind; j.bidir = bidir; j.Kp = Kp; j.K = K; j.KB = KB;
      j.first_block = fb; j.nblocks = blocks((long)NP * KB * 4); fb += j.nblocks;
      a.job[a.njobs++] = j;
      PackJob h{};
      h.w = w_hh_host[i]; h.out = whh_x3_host[i]; h.type = 1;
      h.first_block = fb; h.nblocks = blocks((long)(Hp / ug) * KQ2 * (ug / 4) * 64); fb += h.nblocks;
      a.job[a.njobs++] = h;
      if (whhR_host) {
        PackJob r{};
        r.w = w_hh_host[i]; r.out = whhR_host[i]; r.type = 2;
        r.first_block = fb; r.nblocks = blocks((long)(Hp / ug) * a.KC * NUB * 64); fb += r.nblocks;
        a.job[a.njobs++] = r;
      }
    }
    hipLaunchKernelGGL(lstm_pack_train_kernel, dim3((unsigned)fb), dim3(256), 0, (hipStream_t)stream, a);
  }
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

size_t onssen_bn_rows_workspace_bytes(int64_t M, int C) {
  return M > 0 && C > 0 ? (size_t)((M + bnr::STRIP - 1) / bnr::STRIP) * 3 * (size_t)C * sizeof(float) : 0;   // (count-free strip sums + shift)
}

int onssen_bn_rows_train_f32(const float* x, int64_t M, int C, const float* gamma, const float* beta, float eps, float* y,
                             float* mean, float* invstd, void* ws, size_t ws_bytes, void* stream) {
  if (!x || !gamma || !beta || !y || !mean || !invstd || !ws || M <= 1 || C <= 0 || M > 0x7fffffffL * bnr::STRIP) return ONSSEN_E_ARG;
  if (ws_bytes < onssen_bn_rows_workspace_bytes(M, C)) return ONSSEN_E_WORKSPACE;
  ONSSEN_CLEAR_ERROR();
  hipStream_t st = (hipStream_t)stream;
  const int nblk = (int)((M + bnr::STRIP - 1) / bnr::STRIP);
  const dim3 gp((unsigned)nblk, (unsigned)ceil_div(C, 256));
  hipLaunchKernelGGL((bn_rows_partial_kernel<0>), gp, dim3(256), 0, st, x, (const float*)nullptr, (const float*)nullptr,
                     (const float*)nullptr, (long)M, C, (float*)ws);
  hipLaunchKernelGGL((bn_rows_final_kernel<0>), dim3((unsigned)ceil_div(C, 16)), dim3(256), 0, st, (const float*)ws, nblk, (long)M, C,
                     eps, mean, invstd);
  const long nb = ((long)M * C + 255) / 256;
  hipLaunchKernelGGL((bn_rows_apply_kernel<0>), dim3((unsigned)(nb > 16384 ? 16384 : nb)), dim3(256), 0, st, x, (const float*)nullptr,
                     (const float*)mean, (const float*)invstd, gamma, beta, (const float*)nullptr, (long)M, C, y);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_bn_rows_grad_f32(const float* x, const float* dy, int64_t M, int C, const float* gamma, const float* mean,
                            const float* invstd, float* dx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream) {
  if (!x || !dy || !gamma || !mean || !invstd || !dx || !dgamma || !dbeta || !ws || M <= 1 || C <= 0) return ONSSEN_E_ARG;
  if (ws_bytes < onssen_bn_rows_workspace_bytes(M, C)) return ONSSEN_E_WORKSPACE;
  ONSSEN_CLEAR_ERROR();
  hipStream_t st = (hipStream_t)stream;
  const int nblk = (int)((M + bnr::STRIP - 1) / bnr::STRIP);
  const dim3 gp((unsigned)nblk, (unsigned)ceil_div(C, 256));
  hipLaunchKernelGGL((bn_rows_partial_kernel<1>), gp, dim3(256), 0, st, x, dy, mean, invstd, (long)M, C, (float*)ws);
  hipLaunchKernelGGL((bn_rows_final_kernel<1>), dim3((unsigned)ceil_div(C, 16)), dim3(256), 0, st, (const float*)ws, nblk, (long)M, C,
                     0.0f, dbeta, dgamma);
  const long nb = ((long)M * C + 255) / 256;
  hipLaunchKernelGGL((bn_rows_apply_kernel<1>), dim3((unsigned)(nb > 16384 ? 16384 : nb)), dim3(256), 0, st, x, dy, mean, invstd, gamma,
                     (const float*)dbeta, (const float*)dgamma, (long)M, C, dx);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_l2norm_rows_f32(const float* x, int64_t rows, int D, float eps, float* y, void* stream) {
  if (!x || !y || rows <= 0 || D <= 0 || D > 64 || (D % 4) != 0 || !(eps > 0.0f)) return ONSSEN_E_ARG;
  if (!aligned16(x) || !aligned16(y)) return ONSSEN_E_ALIGN;
  ONSSEN_CLEAR_ERROR();
  const int dq = D <= 20 ? 5 : D <= 32 ? 8 : 16;
  const long nb = (rows + 4 * (64 / dq) - 1) / (4 * (64 / dq));      // 4 waves per workgroup, 64 / dq rows per wave and pass
#define ONSSEN_L2N(DQ_) hipLaunchKernelGGL((l2norm_rows_kernel<false, DQ_>), dim3((unsigned)(nb > 8192 ? 8192 : nb)), dim3(256), 0, (hipStream_t)stream, x, \
                                           (const float*)nullptr, (long)rows, D, eps, y)
  if (dq == 5) ONSSEN_L2N(5); else if (dq == 8) ONSSEN_L2N(8); else ONSSEN_L2N(16);
#undef ONSSEN_L2N
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_l2norm_rows_grad_f32(const float* x, const float* g, int64_t rows, int D, float eps, float* dx, void* stream) {
  if (!x || !g || !dx || rows <= 0 || D <= 0 || D > 64 || (D % 4) != 0 || !(eps > 0.0f)) return ONSSEN_E_ARG;
  if (!aligned16(x) || !aligned16(g) || !aligned16(dx)) return ONSSEN_E_ALIGN;
  ONSSEN_CLEAR_ERROR();
  const int dq = D <= 20 ? 5 : D <= 32 ? 8 : 16;
  const long nb = (rows + 4 * (64 / dq) - 1) / (4 * (64 / dq));      // 4 waves per workgroup, 64 / dq rows per wave and pass
#define ONSSEN_L2N(DQ_) hipLaunchKernelGGL((l2norm_rows_kernel<true, DQ_>), dim3((unsigned)(nb > 8192 ? 8192 : nb)), dim3(256), 0, (hipStream_t)stream, x, g, \
                                           (long)rows, D, eps, dx)
  if (dq == 5) ONSSEN_L2N(5); else if (dq == 8) ONSSEN_L2N(8); else ONSSEN_L2N(16);
#undef ONSSEN_L2N
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_l2norm_rows_grad_y_f32(const float* y, const float* inv_norm, const float* g, int64_t rows, int D, float eps, float* dx,
                                  void* stream) {
  if (!y || !inv_norm || !g || !dx || rows <= 0 || D <= 0 || D > 64 || (D % 4) != 0 || !(eps > 0.0f)) return ONSSEN_E_ARG;
  if (!aligned16(y) || !aligned16(g) || !aligned16(dx)) return ONSSEN_E_ALIGN;
  ONSSEN_CLEAR_ERROR();
  const int dq = D <= 20 ? 5 : D <= 32 ? 8 : 16;
  const long nb = (rows + 4 * (64 / dq) - 1) / (4 * (64 / dq));      // 4 waves per workgroup, 64 / dq rows per wave and pass
#define ONSSEN_L2N(DQ_) hipLaunchKernelGGL((l2norm_rows_grad_y_kernel<DQ_>), dim3((unsigned)(nb > 8192 ? 8192 : nb)), dim3(256), 0, (hipStream_t)stream, y, \
                                           inv_norm, g, (long)rows, D, eps, dx)
  if (dq == 5) ONSSEN_L2N(5); else if (dq == 8) ONSSEN_L2N(8); else ONSSEN_L2N(16);
#undef ONSSEN_L2N
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_dropout_f32(const float* x, int64_t n, float p, uint64_t seed, float* out, void* stream) {
  if (!x || !out || n <= 0 || !(p >= 0.0f) || !(p < 1.0f)) return ONSSEN_E_ARG;
  const int vec = (n % 4) == 0 && aligned16(x) && aligned16(out);
  const double t = (double)p * 4294967296.0;
  const unsigned thr = t >= 4294967295.0 ? 4294967295u : (unsigned)t;     // hash < thr: dropped
  const long work = vec ? n / 4 : n;
  const long nb = (work + 255) / 256;
  ONSSEN_CLEAR_ERROR();
  hipLaunchKernelGGL(dropout_kernel, dim3((unsigned)(nb > 16384 ? 16384 : nb)), dim3(256), 0, (hipStream_t)stream, x, (long)n, thr,
                     1.0f / (1.0f - p), (unsigned long long)seed, out, vec);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

static long adam_blocks(const int64_t* numel, int n) {
  long b = 0;
  for (int i = 0; i < n; ++i) b += (numel[i] + opt::CHUNK - 1) / opt::CHUNK;
  return b;
}

size_t onssen_clip_adam_workspace_bytes(const int64_t* numel_host, int n) {
  if (!numel_host || n <= 0) return 0;
  for (int i = 0; i < n; ++i)
    if (numel_host[i] <= 0) return 0;
  return align256((size_t)(1 + adam_blocks(numel_host, n)) * sizeof(float));
}

int onssen_clip_adam_f32(int n, float* const* p_host, float* const* g_host, float* const* m_host, float* const* v_host,
                         const int64_t* numel_host, float max_norm, double lr, double beta1, double beta2, double eps, int step,
                         int write_grads, void* ws, size_t ws_bytes, void* stream) {
  if (n <= 0 || !p_host || !g_host || !m_host || !v_host || !numel_host || step < 1 || !(lr >= 0.) || !(beta1 >= 0. && beta1 < 1.) ||
      !(beta2 >= 0. && beta2 < 1.) || !(eps >= 0.))
    return ONSSEN_E_ARG;
  for (int i = 0; i < n; ++i)
    if (!p_host[i] || !g_host[i] || !m_host[i] || !v_host[i] || numel_host[i] <= 0) return ONSSEN_E_ARG;
  const bool clip = max_norm > 0.f && max_norm < INFINITY;
  const long nblk = adam_blocks(numel_host, n);
  if (nblk > 0x7fffffffL) return ONSSEN_E_ARG;
  if (clip && (!ws || ws_bytes < onssen_clip_adam_workspace_bytes(numel_host, n))) return ONSSEN_E_WORKSPACE;
  if (clip && (reinterpret_cast<uintptr_t>(ws) & 15u)) return ONSSEN_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  float* wsf = (float*)ws;
  // hyper-parameters arrive as doubles (Python floats) and are rounded ONCE, after 1 - beta has been formed: 1 - float(0.999) is
  // off by 1.3e-5 relative, which is what torch avoids by the same route
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  ONSSEN_CLEAR_ERROR();
  for (int pass = clip ? 0 : 1; pass < 2; ++pass) {
    long done_blocks = 0;
    for (int i0 = 0; i0 < n; i0 += opt::MAXT) {
      AdamArgs a;
      a.n = n - i0 < opt::MAXT ? n - i0 : opt::MAXT;
      int b = 0;
      for (int i = 0; i < a.n; ++i) {
        a.p[i] = p_host[i0 + i]; a.g[i] = g_host[i0 + i]; a.m[i] = m_host[i0 + i]; a.v[i] = v_host[i0 + i];
        a.numel[i] = (long)numel_host[i0 + i];
        a.first_block[i] = b;
        b += (int)((numel_host[i0 + i] + opt::CHUNK - 1) / opt::CHUNK);
      }
      a.first_block[a.n] = b;
      a.lr_bc1 = (float)(lr / bc1); a.omb1 = (float)(1.0 - beta1); a.beta2 = (float)beta2; a.omb2 = (float)(1.0 - beta2);
      a.eps = (float)eps; a.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
      a.max_norm = max_norm; a.write_grads = write_grads;
      a.partials = clip ? wsf + 1 + done_blocks : nullptr;
      a.norm = clip ? wsf : nullptr;
      if (pass == 0) hipLaunchKernelGGL(grad_sqnorm_partial_kernel, dim3((unsigned)b), dim3(256), 0, st, a);
      else hipLaunchKernelGGL(clip_adam_kernel, dim3((unsigned)b), dim3(256), 0, st, a);
      done_blocks += b;
    }
    if (pass == 0) hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(256), 0, st, (const float*)(wsf + 1), (int)nblk, wsf);
  }
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_phase_input_f32(const float* x_mag, const float* mask, int64_t m_sb, int64_t m_sc, int64_t m_st,
                           int64_t m_sf, const float* x_phase, int B, int C, int T, int F, float* out, void* stream) {
  if (!x_mag || !mask || !x_phase || !out || B <= 0 || C <= 0 || T <= 0 || F <= 0) return ONSSEN_E_ARG;
  const long total = (long)C * B * T * 3 * F;
  ONSSEN_CLEAR_ERROR();
  hipLaunchKernelGGL(phase_input_kernel, dim3(ew_blocks(total)), dim3(256), 0, (hipStream_t)stream,
                     x_mag, mask, (long)m_sb, (long)m_sc, (long)m_st, (long)m_sf, x_phase, B, C, T, F, out);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_labels_f32(const float* stft_mix, const float* stft_s1, const float* stft_s2, const float* feature_mix, int B,
                      int T, int F, float db_threshold, float* utt_max, float* one_hot, float* mag_mix, float* mag_s1,
                      float* mag_s2, float* cos_s1, float* cos_s2, void* stream) {
  if (!stft_mix || !stft_s1 || !stft_s2 || !feature_mix || !utt_max || !one_hot || !mag_mix || !mag_s1 || !mag_s2 ||
      B <= 0 || T <= 0 || F <= 0 || ((cos_s1 == nullptr) != (cos_s2 == nullptr)))
    return ONSSEN_E_ARG;
  ONSSEN_CLEAR_ERROR();
  hipStream_t st = (hipStream_t)stream;
  const long per_utt = (long)T * F, total = per_utt * B;
  hipLaunchKernelGGL(utt_max_kernel, dim3((unsigned)B), dim3(256), 0, st, feature_mix, per_utt, utt_max);
  hipLaunchKernelGGL(labels_kernel, dim3(ew_blocks(total)), dim3(256), 0, st, stft_mix, stft_s1, stft_s2,
                     feature_mix, utt_max, per_utt, total, db_threshold, one_hot, mag_mix, mag_s1, mag_s2, cos_s1, cos_s2);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_param_guard_u32(const void* const* ptrs, const int64_t* numel, int n, int samples, int mode, uint32_t* ref, uint32_t* flag,
                           void* stream) {
  if (!ptrs || !numel || !ref || !flag || n <= 0 || samples <= 0 || (mode != 0 && mode != 1)) return ONSSEN_E_ARG;
  ONSSEN_CLEAR_ERROR();
  hipLaunchKernelGGL(param_guard_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float* const*>(ptrs),
                     reinterpret_cast<const long long*>(numel), samples, mode, ref, flag);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_log_magnitude_f32(const float* stft_ri, int64_t n, float epsilon, float* out, void* stream) {
  if (!stft_ri || !out || n <= 0) return ONSSEN_E_ARG;
  ONSSEN_CLEAR_ERROR();
  hipLaunchKernelGGL(log_magnitude_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, stft_ri, (long)n, epsilon, out);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_cos_difference_f32(const float* stft_1, const float* stft_2, int64_t n, float* out, void* stream) {
  if (!stft_1 || !stft_2 || !out || n <= 0) return ONSSEN_E_ARG;
  ONSSEN_CLEAR_ERROR();
  hipLaunchKernelGGL(cos_difference_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, stft_1, stft_2, (long)n, out);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_one_hot_f32(const float* feature_mix, const float* mag_s1, const float* mag_s2, int B, int64_t per_utt,
                       float db_threshold, float* utt_max, float* one_hot, void* stream) {
  if (!feature_mix || !mag_s1 || !mag_s2 || !utt_max || !one_hot || B <= 0 || per_utt <= 0) return ONSSEN_E_ARG;
  ONSSEN_CLEAR_ERROR();
  hipStream_t st = (hipStream_t)stream;
  const long total = (long)per_utt * B;
  hipLaunchKernelGGL(utt_max_kernel, dim3((unsigned)B), dim3(256), 0, st, feature_mix, (long)per_utt, utt_max);
  hipLaunchKernelGGL(one_hot_kernel, dim3(ew_blocks(total)), dim3(256), 0, st, feature_mix, mag_s1, mag_s2, utt_max, (long)per_utt,
                     total, db_threshold, one_hot);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

#ifdef ONSSEN_FFT_PROFILE
int onssen_debug_fft_stamps(long long* host_out, int n) {      // profile builds only; not part of the ABI
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_fft_stamps), (size_t)n * sizeof(long long), 0, hipMemcpyDeviceToHost);
}
#endif

static int mask_istft_impl(const float* stft_ri, const float* mask, int64_t m_sb, int64_t m_sc, int64_t m_st,
                           int64_t m_sf, int B, int C, int T, int n_fft, int hop, int length, float* out,
                           void* stream, const int32_t* frames, const int32_t* lengths, const float* phase = nullptr,
                           int64_t p_sc = 0, bool magnitude = false) {
  if (!stft_ri || !out || B <= 0 || C <= 0 || T <= 0 || hop <= 0 || length <= 0 || hop > n_fft) return ONSSEN_E_ARG;
  if (reinterpret_cast<uintptr_t>(stft_ri) & 7u) return ONSSEN_E_ALIGN;               // (re, im) pairs are read as one 8-byte word
  if (phase && ((reinterpret_cast<uintptr_t>(phase) & 7u) || (p_sc & 1))) return ONSSEN_E_ALIGN;   // so are the phase vectors
  // a chunk of FR hops of output needs FR + ceil(n_fft/hop) - 1 frames (one more when the chunk
  // origin n_fft/2 is not hop-aligned); FB frames fit in LDS
  // speakers go through the inverse FFT in pairs (one complex transform for two real frames) when there are at least
  // two; FB frames of both speakers then share the LDS, so the longer transforms keep fewer frames per workgroup
  const bool hop_aligned = (n_fft % hop) == 0 && ((n_fft / 2) % hop) == 0;
  const int halo = ceil_div(n_fft, hop) - 1 + (hop_aligned ? 0 : 1);
  bool pair = C >= 2 && n_fft <= 512 && !magnitude;      // (the magnitude form has one estimate per input: unpaired only)
  int FB = pair ? (n_fft <= 256 ? 16 : 8) : (n_fft <= 512 ? 16 : 8);
  if (pair && FB - halo <= 0) {      // very small hops: the unpaired form keeps more frames per workgroup
    pair = false;
    FB = 16;
  }
  // the wsj0-2mix transform (256, two speakers) exists with 8, 12 and 16 frames per workgroup.  A grid that fits the chip in one
  // go (3 workgroups per CU) is latency-bound -- its time is the rounds of ONE workgroup, so the fewest frames per workgroup
  // win (one utterance of 1 000 frames: 7.7 / 9.5 / 11.4 us with 8 / 12 / 16); a larger grid is throughput-bound and the
  // halo frames that every chunk transforms again cost more than the shorter workgroups save (32 x 400: 35.1 / 31.6 / 28.4 us)
  static const int fb_knob = ONSSEN_KNOB_INT("ONSSEN_ISTFT_FB", 0);      // debug builds: tools/ab_variants.py
  if (pair && n_fft == 256 && FB - halo > 0) {
    if (fb_knob == 8 || fb_knob == 12 || fb_knob == 16) {
      if (fb_knob - halo > 0) FB = fb_knob;
    } else {
      for (int fb = 8; fb < 16; fb += 4) {
        if (fb - halo <= 0) continue;
        if ((long)ceil_div(length, (fb - halo) * hop) * ceil_div(C, 2) * B <= 256L * 3) { FB = fb; break; }
      }
    }
  }
  const int FR = FB - halo;
  if (FR <= 0) return ONSSEN_E_ARG;
  ONSSEN_CLEAR_ERROR();
  const dim3 grid((unsigned)ceil_div(length, FR * hop), (unsigned)(pair ? ceil_div(C, 2) : C), (unsigned)B), block(256);
  hipStream_t st = (hipStream_t)stream;
  // (phase: the phase-aware operand of onssen_phase_istft_f32 -- the same geometry, its own instantiation of every form;
  // magnitude: the operand of onssen_mag_istft_f32, the unpaired forms only)
#define ONSSEN_ISTFT(N_, FB_, PAIR_)                                                                                    \
  do {                                                                                                                  \
    if (phase)                                                                                                          \
      hipLaunchKernelGGL((mask_istft_kernel<N_, FB_, PAIR_, ISTFT_PHASE>), grid, block, 0, st, stft_ri, mask, (long)m_sb, \
                         (long)m_sc, (long)m_st, (long)m_sf, C, T, hop, length, FR, out, frames, lengths, phase, (long)p_sc); \
    else                                                                                                                \
      hipLaunchKernelGGL((mask_istft_kernel<N_, FB_, PAIR_, ISTFT_MASK>), grid, block, 0, st, stft_ri, mask, (long)m_sb, \
                         (long)m_sc, (long)m_st, (long)m_sf, C, T, hop, length, FR, out, frames, lengths, phase, (long)p_sc); \
  } while (0)
#define ONSSEN_ISTFT_MAG(N_, FB_)                                                                                       \
  hipLaunchKernelGGL((mask_istft_kernel<N_, FB_, false, ISTFT_MAG>), grid, block, 0, st, stft_ri, mask, (long)m_sb,     \
                     (long)m_sc, (long)m_st, (long)m_sf, C, T, hop, length, FR, out, frames, lengths, phase, (long)p_sc)
  if (magnitude) {
    if (n_fft == 256) ONSSEN_ISTFT_MAG(256, 16);
    else if (n_fft == 512) ONSSEN_ISTFT_MAG(512, 16);
    else if (n_fft == 1024) ONSSEN_ISTFT_MAG(1024, 8);
    else return ONSSEN_E_ARG;
  } else
  if (n_fft == 256) {
    if (!pair) ONSSEN_ISTFT(256, 16, false);
    else if (FB == 8) ONSSEN_ISTFT(256, 8, true);
    else if (FB == 12) ONSSEN_ISTFT(256, 12, true);
    else ONSSEN_ISTFT(256, 16, true);
  }
  else if (n_fft == 512) { if (pair) ONSSEN_ISTFT(512, 8, true); else ONSSEN_ISTFT(512, 16, false); }
  else if (n_fft == 1024) ONSSEN_ISTFT(1024, 8, false);
  else
    return ONSSEN_E_ARG;
#undef ONSSEN_ISTFT_MAG
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_mask_istft_f32(const float* stft_ri, const float* mask, int64_t m_sb, int64_t m_sc, int64_t m_st,
                          int64_t m_sf, int B, int C, int T, int n_fft, int hop, int length, float* out,
                          void* stream) {
  return mask_istft_impl(stft_ri, mask, m_sb, m_sc, m_st, m_sf, B, C, T, n_fft, hop, length, out, stream, nullptr, nullptr);
}

int onssen_mask_istft_ragged_f32(const float* stft_ri, const float* mask, int64_t m_sb, int64_t m_sc, int64_t m_st,
                                 int64_t m_sf, int B, int C, int T, const int32_t* frames, int n_fft, int hop, int length,
                                 const int32_t* lengths, float* out, void* stream) {
  if (!frames || !lengths) return ONSSEN_E_ARG;
  return mask_istft_impl(stft_ri, mask, m_sb, m_sc, m_st, m_sf, B, C, T, n_fft, hop, length, out, stream, frames, lengths);
}

int onssen_phase_istft_f32(const float* stft_ri, const float* mask, int64_t m_sb, int64_t m_sc, int64_t m_st, int64_t m_sf,
                           const float* phase, int64_t p_sc, int B, int C, int T, int n_fft, int hop, int length, float* out,
                           void* stream) {
  if (!phase) return ONSSEN_E_ARG;
  return mask_istft_impl(stft_ri, mask, m_sb, m_sc, m_st, m_sf, B, C, T, n_fft, hop, length, out, stream, nullptr, nullptr, phase,
                         p_sc);
}

int onssen_phase_istft_ragged_f32(const float* stft_ri, const float* mask, int64_t m_sb, int64_t m_sc, int64_t m_st, int64_t m_sf,
                                  const float* phase, int64_t p_sc, int B, int C, int T, const int32_t* frames, int n_fft, int hop,
                                  int length, const int32_t* lengths, float* out, void* stream) {
  if (!phase || !frames || !lengths) return ONSSEN_E_ARG;
  return mask_istft_impl(stft_ri, mask, m_sb, m_sc, m_st, m_sf, B, C, T, n_fft, hop, length, out, stream, frames, lengths, phase,
                         p_sc);
}

int onssen_misi_phase_f32(const float* mix, int64_t mix_stride, const float* est, int64_t est_sb, int64_t est_sc, int B, int C,
                          int n_samples, int n_fft, int hop, float* phase, void* stream) {
  return misi_phase_impl(mix, mix_stride, est, est_sb, est_sc, B, C, n_samples, n_fft, hop, phase, stream, nullptr);
}

int onssen_misi_phase_ragged_f32(const float* mix, int64_t mix_stride, const float* est, int64_t est_sb, int64_t est_sc, int B,
                                 int C, int n_max, const int32_t* n_per_utt, int n_fft, int hop, float* phase, void* stream) {
  if (!n_per_utt) return ONSSEN_E_ARG;
  return misi_phase_impl(mix, mix_stride, est, est_sb, est_sc, B, C, n_max, n_fft, hop, phase, stream, n_per_utt);
}

int onssen_istft_backward_f32(const float* stft_ri, const float* operand, int64_t m_sb, int64_t m_sc, int64_t m_st, int64_t m_sf,
                              const float* phase, int64_t p_sc, int mode, int B, int C, int T, const int32_t* frames, int n_fft, int hop,
                              int length, const int32_t* lengths, const float* g_out, float* g_operand, float* g_phase, void* stream) {
  return istft_backward_impl(stft_ri, operand, m_sb, m_sc, m_st, m_sf, phase, p_sc, mode, B, C, T, frames, n_fft, hop, length, lengths,
                             g_out, g_operand, g_phase, stream);
}

int onssen_mag_istft_f32(const float* stft_ri, const float* mag, int64_t m_sb, int64_t m_sc, int64_t m_st, int64_t m_sf, int B,
                         int C, int T, int n_fft, int hop, int length, float* out, void* stream) {
  if (!mag) return ONSSEN_E_ARG;
  return mask_istft_impl(stft_ri, mag, m_sb, m_sc, m_st, m_sf, B, C, T, n_fft, hop, length, out, stream, nullptr, nullptr, nullptr, 0,
                         true);
}

int onssen_mag_istft_ragged_f32(const float* stft_ri, const float* mag, int64_t m_sb, int64_t m_sc, int64_t m_st, int64_t m_sf,
                                int B, int C, int T, const int32_t* frames, int n_fft, int hop, int length, const int32_t* lengths,
                                float* out, void* stream) {
  if (!mag || !frames || !lengths) return ONSSEN_E_ARG;
  return mask_istft_impl(stft_ri, mag, m_sb, m_sc, m_st, m_sf, B, C, T, n_fft, hop, length, out, stream, frames, lengths, nullptr, 0,
                         true);
}

}  // extern "C"
