// Speech enhancement (egs/daps): training labels and the two masked-magnitude losses, value and gradient (part of onssen_hip.hip).
// =================================================================================================
// onssen/data/daps_enhance.py:104-106 -- from the (re, im) spectra of a noisy chunk and of its clean counterpart
//   mag_noisy = |X|, mag_clean = |S| (np.abs: hypotf, as labels_kernel) and cos_diff = cos(angle(X) - angle(S))
//   (get_cos_difference: the expression of cos_difference_kernel, so the same bits).
//   labels_enhance_kernel   one pass, 16 bytes in and 12 bytes out per bin (8 out without cos_diff): (re, im) as one 8-byte load
// onssen/loss/loss_mask.py:6-40 -- one estimate, one target, no assignment to choose:
//   MSA  per_utt[b] = sum_bins (est - clean)^2                                     (MSELoss's mean: the caller's scale = 1 / (B T F))
//   PSA  per_utt[b] = sum_bins |mask x - t|,  t = min(x, relu(s c))                (norm_1d; x = mag_noisy, s = mag_clean, c = cos_diff)
//   total = scale * sum_b per_utt[b]
//   loss_enhance_kernel        grid (NBLK, B): a workgroup reads its slice of the maps ONCE (8 bytes per bin MSA, 16 PSA) and writes one
//                              fp64 partial sum
//   loss_enhance_final_kernel  one workgroup, one thread per utterance (strided past 256): adds the slices in order, then thread 0
//                              adds the utterances in order of b
//   loss_enhance_grad_kernel   one elementwise pass (12 bytes per bin MSA, 20 PSA):
//     MSA  d est  = g[0] 2 scale (est - clean)
//     PSA  d mask = g[b] x sign(mask x - t)                                        (sign(0) = 0, as loss_mask_grad_kernel)
// Per-bin arithmetic is fp32 -- the PSA residual is one fused multiply-add, so its sign is the exact one -- every sum fp64 in a
// fixed order: no atomics, a workspace that needs no zeroing, two runs give the same bits.
// =================================================================================================
namespace lossenh {
constexpr int NBLK = 32;        // slices per utterance
}  // namespace lossenh

__global__ void labels_enhance_kernel(const float2* __restrict__ noisy, const float2* __restrict__ clean, long total,
                                      float* __restrict__ mag_noisy, float* __restrict__ mag_clean, float* __restrict__ cos_diff) {
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const float2 a = noisy[e];
    mag_noisy[e] = hypotf(a.x, a.y);
    if (!clean) continue;                          // (separation has the noisy spectrum only: 8 bytes in, 4 out)
    const float2 b = clean[e];
    mag_clean[e] = hypotf(b.x, b.y);
    if (cos_diff) cos_diff[e] = cosf(atan2f(a.y, a.x) - atan2f(b.y, b.x));
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void loss_enhance_kernel(const float* __restrict__ est, const float* __restrict__ mag_noisy,
                                                           const float* __restrict__ mag_clean, const float* __restrict__ cos_diff,
                                                           int TF, double* __restrict__ partial) {
  using namespace lossenh;
  __shared__ double red[256];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int per = (TF + NBLK - 1) / NBLK, e0 = blockIdx.x * per, e1 = e0 + per < TF ? e0 + per : TF;
  double acc = 0.0;                                  // (an empty slice -- fewer bins than slices -- keeps it)
  for (int e = e0 + tid; e < e1; e += 256) {
    const long i = (long)b * TF + e;
    if constexpr (MODE == ONSSEN_ENHANCE_MSA) {
      const float d = est[i] - mag_clean[i];
      acc += d * d;
    } else {
      const float x = mag_noisy[i];
      const float t = fminf(x, fmaxf(mag_clean[i] * cos_diff[i], 0.0f));
      acc += fabsf(fmaf(est[i], x, -t));
    }
  }
  red[tid] = acc;
  __syncthreads();
  for (int sft = 128; sft > 0; sft >>= 1) {
    if (tid < sft) red[tid] += red[tid + sft];
    __syncthreads();
  }
  if (tid == 0) partial[(long)b * NBLK + blockIdx.x] = red[0];
}

__global__ __launch_bounds__(256) void loss_enhance_final_kernel(const double* __restrict__ partial, double* __restrict__ utt, int B,
                                                                 float scale, float* __restrict__ per_utt, float* __restrict__ total) {
  using namespace lossenh;
  for (int b = threadIdx.x; b < B; b += 256) {
    double s = 0.0;
    for (int k = 0; k < NBLK; ++k) s += partial[(long)b * NBLK + k];
    utt[b] = s;
    per_utt[b] = (float)s;
  }
  __syncthreads();
  if (threadIdx.x == 0 && total) {
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += utt[b];
    total[0] = (float)((double)scale * s);
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void loss_enhance_grad_kernel(const float* __restrict__ est, const float* __restrict__ mag_noisy,
                                                                const float* __restrict__ mag_clean,
                                                                const float* __restrict__ cos_diff, int TF, float scale,
                                                                const float* __restrict__ g, float* __restrict__ d_est) {
  const int b = blockIdx.y;
  const float gb = MODE == ONSSEN_ENHANCE_MSA ? g[0] * 2.0f * scale : g[b];
  for (int e = blockIdx.x * 256 + threadIdx.x; e < TF; e += gridDim.x * 256) {
    const long i = (long)b * TF + e;
    if constexpr (MODE == ONSSEN_ENHANCE_MSA) {
      d_est[i] = gb * (est[i] - mag_clean[i]);
    } else {
      const float x = mag_noisy[i];
      const float r = fmaf(est[i], x, -fminf(x, fmaxf(mag_clean[i] * cos_diff[i], 0.0f)));
      d_est[i] = gb * x * (r > 0.0f ? 1.0f : r < 0.0f ? -1.0f : 0.0f);
    }
  }
}

extern "C" {

int onssen_labels_enhance_f32(const float* stft_noisy, const float* stft_clean, int64_t n_bins, float* mag_noisy, float* mag_clean,
                              float* cos_diff, void* stream) {
  if (!stft_noisy || !mag_noisy || n_bins <= 0) return ONSSEN_E_ARG;
  if (!stft_clean != !mag_clean || (!stft_clean && cos_diff)) return ONSSEN_E_ARG;      // no clean spectrum: |X| alone
  if ((reinterpret_cast<uintptr_t>(stft_noisy) | reinterpret_cast<uintptr_t>(stft_clean)) & 7u)
    return ONSSEN_E_ALIGN;                          // (re, im) pairs are read as one 8-byte word
  ONSSEN_CLEAR_ERROR();
  const long nb = ((long)n_bins + 255) / 256;
  hipLaunchKernelGGL(labels_enhance_kernel, dim3((unsigned)(nb > 8192 ? 8192 : nb)), dim3(256), 0, (hipStream_t)stream,
                     (const float2*)stft_noisy, (const float2*)stft_clean, (long)n_bins, mag_noisy, mag_clean, cos_diff);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

size_t onssen_loss_enhance_workspace_bytes(int B) {
  return B > 0 ? (size_t)B * (lossenh::NBLK + 1) * sizeof(double) : 0;      // the slices' sums, then the utterances'
}

int onssen_loss_enhance_f32(int mode, const float* est, const float* mag_noisy, const float* mag_clean, const float* cos_diff, int B,
                            int TF, float scale, float* per_utt, float* total, void* ws, size_t ws_bytes, void* stream) {
  using namespace lossenh;
  if ((mode != ONSSEN_ENHANCE_MSA && mode != ONSSEN_ENHANCE_PSA) || !est || !mag_clean || !per_utt || !ws || B <= 0 || B > 65535 ||
      TF <= 0)
    return ONSSEN_E_ARG;
  if (mode == ONSSEN_ENHANCE_PSA && (!mag_noisy || !cos_diff)) return ONSSEN_E_ARG;
  if (reinterpret_cast<uintptr_t>(ws) & 7u) return ONSSEN_E_ALIGN;          // the partial sums are fp64
  if (ws_bytes < onssen_loss_enhance_workspace_bytes(B)) return ONSSEN_E_WORKSPACE;
  ONSSEN_CLEAR_ERROR();
  hipStream_t st = (hipStream_t)stream;
  double* partial = (double*)ws;
  if (mode == ONSSEN_ENHANCE_MSA)
    hipLaunchKernelGGL((loss_enhance_kernel<ONSSEN_ENHANCE_MSA>), dim3(NBLK, (unsigned)B), dim3(256), 0, st, est, mag_noisy, mag_clean,
                       cos_diff, TF, partial);
  else
    hipLaunchKernelGGL((loss_enhance_kernel<ONSSEN_ENHANCE_PSA>), dim3(NBLK, (unsigned)B), dim3(256), 0, st, est, mag_noisy, mag_clean,
                       cos_diff, TF, partial);
  hipLaunchKernelGGL(loss_enhance_final_kernel, dim3(1), dim3(256), 0, st, (const double*)partial, partial + (size_t)B * NBLK, B, scale,
                     per_utt, total);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_loss_enhance_grad_f32(int mode, const float* est, const float* mag_noisy, const float* mag_clean, const float* cos_diff,
                                 int B, int TF, float scale, const float* g, float* d_est, void* stream) {
  if ((mode != ONSSEN_ENHANCE_MSA && mode != ONSSEN_ENHANCE_PSA) || !est || !mag_clean || !g || !d_est || B <= 0 || B > 65535 ||
      TF <= 0)
    return ONSSEN_E_ARG;
  if (mode == ONSSEN_ENHANCE_PSA && (!mag_noisy || !cos_diff)) return ONSSEN_E_ARG;
  ONSSEN_CLEAR_ERROR();
  const int nblk = ceil_div(TF, 256) < 64 ? ceil_div(TF, 256) : 64;
  const dim3 grid((unsigned)nblk, (unsigned)B);
  if (mode == ONSSEN_ENHANCE_MSA)
    hipLaunchKernelGGL((loss_enhance_grad_kernel<ONSSEN_ENHANCE_MSA>), grid, dim3(256), 0, (hipStream_t)stream, est, mag_noisy,
                       mag_clean, cos_diff, TF, scale, g, d_est);
  else
    hipLaunchKernelGGL((loss_enhance_grad_kernel<ONSSEN_ENHANCE_PSA>), grid, dim3(256), 0, (hipStream_t)stream, est, mag_noisy,
                       mag_clean, cos_diff, TF, scale, g, d_est);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

}  // extern "C"
