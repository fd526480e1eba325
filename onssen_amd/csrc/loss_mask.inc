// Mask-inference term of the chimera losses, value and gradient: the kernels and their C ABI entries (part of onssen_hip.hip).
// =================================================================================================
// N1 (forward half): mask-inference term of the chimera losses, onssen/loss/loss_chimera.py:25-29 (MSA) and :53-57 (PSA):
//   l_AB = sum |mA*x - t1| + sum |mB*x - t2|,  l_BA = sum |mB*x - t1| + sum |mA*x - t2|,  out = min(l_AB, l_BA)
//   t_s = mag_s (MSA)  or  min(x, relu(mag_s * cos_s)) (PSA, cos given).  One pass over the five / seven maps.
// =================================================================================================
__global__ __launch_bounds__(256) void loss_mask_kernel(const float* __restrict__ mask_a, const float* __restrict__ mask_b,
                                                        long m_sb, long m_se, const float* __restrict__ mag,
                                                        const float* __restrict__ s1, const float* __restrict__ s2,
                                                        const float* __restrict__ c1, const float* __restrict__ c2, int TF,
                                                        float* __restrict__ partial) {
  // grid (NBLK, B): every workgroup sums a slice of the utterance; loss_mask_final_kernel adds the slices in order
  __shared__ double red[4][256];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int per = (TF + (int)gridDim.x - 1) / (int)gridDim.x, e0 = blockIdx.x * per, e1 = e0 + per < TF ? e0 + per : TF;
  double a1 = 0.0, b2 = 0.0, b1 = 0.0, a2 = 0.0;
  for (int e = e0 + tid; e < e1; e += 256) {
    const long i = (long)b * TF + e;
    const float x = mag[i];
    float t1 = s1[i], t2 = s2[i];
    if (c1) {
      t1 = fminf(x, fmaxf(t1 * c1[i], 0.0f));
      t2 = fminf(x, fmaxf(t2 * c2[i], 0.0f));
    }
    const float ma = mask_a[(long)b * m_sb + (long)e * m_se] * x, mb = mask_b[(long)b * m_sb + (long)e * m_se] * x;
    a1 += fabsf(ma - t1); b2 += fabsf(mb - t2); b1 += fabsf(mb - t1); a2 += fabsf(ma - t2);
  }
  red[0][tid] = a1; red[1][tid] = b2; red[2][tid] = b1; red[3][tid] = a2;
  __syncthreads();
  for (int sft = 128; sft > 0; sft >>= 1) {
    if (tid < sft)
      for (int k = 0; k < 4; ++k) red[k][tid] += red[k][tid + sft];
    __syncthreads();
  }
  if (tid < 4) partial[((long)b * gridDim.x + blockIdx.x) * 4 + tid] = (float)red[tid][0];
}

__global__ void loss_mask_final_kernel(const float* __restrict__ partial, int nblk, float* __restrict__ out,
                                       int* __restrict__ perm_out) {
  const int b = blockIdx.x;
  if (threadIdx.x == 0) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < nblk; ++k)
      for (int j = 0; j < 4; ++j) s[j] += (double)partial[((long)b * nblk + k) * 4 + j];
    out[b] = (float)fmin(s[0] + s[1], s[2] + s[3]);
    // the assignment the gradient follows (ties go to A->1, B->2: a measure-zero choice)
    if (perm_out) perm_out[b] = (float)(s[0] + s[1]) <= (float)(s[2] + s[3]) ? 0 : 1;
  }
}

// N1: gradient of the mask-inference term w.r.t. the two mask maps, one pass (the permutation was picked by the forward
// kernels): d out[b] / d mask_A[e] = x sign(mask_A x - t_A), t_A = the target the chosen assignment gives speaker A
// (sign(0) = 0, as torch.abs' backward), times the incoming gradient g[b].  Both maps are written (strided like the inputs).
__global__ __launch_bounds__(256) void loss_mask_grad_kernel(const float* __restrict__ mask_a, const float* __restrict__ mask_b,
                                                             long m_sb, long m_se, const float* __restrict__ mag,
                                                             const float* __restrict__ s1, const float* __restrict__ s2,
                                                             const float* __restrict__ c1, const float* __restrict__ c2, int TF,
                                                             const float* __restrict__ g, const int* __restrict__ perm,
                                                             float* __restrict__ d_a, float* __restrict__ d_b, long d_sb, long d_se) {
  const int b = blockIdx.y;
  const float gb = g[b];
  const bool swap = perm[b] != 0;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < TF; e += gridDim.x * 256) {
    const long i = (long)b * TF + e;
    const float x = mag[i];
    float t1 = s1[i], t2 = s2[i];
    if (c1) {
      t1 = fminf(x, fmaxf(t1 * c1[i], 0.0f));
      t2 = fminf(x, fmaxf(t2 * c2[i], 0.0f));
    }
    const float ra = mask_a[(long)b * m_sb + (long)e * m_se] * x - (swap ? t2 : t1);
    const float rb = mask_b[(long)b * m_sb + (long)e * m_se] * x - (swap ? t1 : t2);
    d_a[(long)b * d_sb + (long)e * d_se] = gb * x * (ra > 0.0f ? 1.0f : ra < 0.0f ? -1.0f : 0.0f);
    d_b[(long)b * d_sb + (long)e * d_se] = gb * x * (rb > 0.0f ? 1.0f : rb < 0.0f ? -1.0f : 0.0f);
  }
}

extern "C" {

size_t onssen_loss_mask_workspace_bytes(int B) { return B > 0 ? (size_t)B * 32 * 4 * sizeof(float) : 0; }

int onssen_loss_mask_f32(const float* mask_a, const float* mask_b, int64_t m_sb, int64_t m_se, const float* mag_mix,
                         const float* mag_s1, const float* mag_s2, const float* cos_s1, const float* cos_s2, int B, int TF,
                         float* out, int32_t* perm_out, void* ws, size_t ws_bytes, void* stream) {
  if (!mask_a || !mask_b || !mag_mix || !mag_s1 || !mag_s2 || !out || !ws || B <= 0 || TF <= 0 ||
      ((cos_s1 == nullptr) != (cos_s2 == nullptr)))
    return ONSSEN_E_ARG;
  if (ws_bytes < onssen_loss_mask_workspace_bytes(B)) return ONSSEN_E_WORKSPACE;
  ONSSEN_CLEAR_ERROR();
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(loss_mask_kernel, dim3(32, (unsigned)B), dim3(256), 0, st, mask_a, mask_b, (long)m_sb, (long)m_se, mag_mix,
                     mag_s1, mag_s2, cos_s1, cos_s2, TF, (float*)ws);
  hipLaunchKernelGGL(loss_mask_final_kernel, dim3((unsigned)B), dim3(64), 0, st, (const float*)ws, 32, out, (int*)perm_out);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_loss_mask_grad_f32(const float* mask_a, const float* mask_b, int64_t m_sb, int64_t m_se, const float* mag_mix,
                              const float* mag_s1, const float* mag_s2, const float* cos_s1, const float* cos_s2, int B, int TF,
                              const float* g, const int32_t* perm, float* d_mask_a, float* d_mask_b, int64_t d_sb, int64_t d_se,
                              void* stream) {
  if (!mask_a || !mask_b || !mag_mix || !mag_s1 || !mag_s2 || !g || !perm || !d_mask_a || !d_mask_b || B <= 0 || TF <= 0 ||
      ((cos_s1 == nullptr) != (cos_s2 == nullptr)))
    return ONSSEN_E_ARG;
  ONSSEN_CLEAR_ERROR();
  const int nblk = ceil_div(TF, 256) < 64 ? ceil_div(TF, 256) : 64;
  hipLaunchKernelGGL(loss_mask_grad_kernel, dim3((unsigned)nblk, (unsigned)B), dim3(256), 0, (hipStream_t)stream, mask_a, mask_b,
                     (long)m_sb, (long)m_se, mag_mix, mag_s1, mag_s2, cos_s1, cos_s2, TF, g, (const int*)perm, d_mask_a, d_mask_b,
                     (long)d_sb, (long)d_se);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

}  // extern "C"
