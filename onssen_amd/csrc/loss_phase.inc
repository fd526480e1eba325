// Mask term and phase term of phase_net's training loss, value and gradient (part of onssen_hip.hip).
// =================================================================================================
// onssen/loss/loss_phase.py:15-35 (restated in onssen_amd/loss.py: loss_phase).  Per utterance, over its TF bins, with the
// mixture magnitude x, the mask estimates mA, mB, the magnitude targets s1, s2, the phase estimates pA, pB and the phase
// targets q1, q2 (two floats per bin; raw STFT values, exactly 0 in silent bins), eps = 1e-8:
//   l1 = sum |mA x - s1| + sum |mB x - s2|,   l2 = sum |mB x - s1| + sum |mA x - s2|
//   cos(p, q) = <p / max(|p|, eps), q / max(|q|, eps)>                    (F.cosine_similarity: each norm clamped)
//   straight (perm 0) if and only if l1 < l2, else swapped (perm 1: A <-> 2, B <-> 1; a tie is swapped, loss_phase.py:21)
//   out_mask = the chosen l,  out_phase = -sum x (cos(pA, q_A) + cos(pB, q_B)) under the same assignment
// (onssen_loss_mask_f32 sends a tie the other way: the chimera losses take a minimum, this loss an index.)
//   loss_phase_kernel        grid (NBLK, B): a workgroup reads its slice of the eleven maps ONCE (52 bytes per bin) and writes eight
//                            fp64 partial sums: the four |.| sums of loss_mask_kernel, then sum x cos for A<->1, B<->2, B<->1, A<->2
//   loss_phase_final_kernel  one thread per utterance adds the slices in order and picks the assignment
//   loss_phase_grad_kernel   one elementwise pass (76 bytes per bin), under perm:
//     d mask_A = g_mask x sign(mA x - s_A)                                  (sign(0) = 0, as loss_mask_grad_kernel)
//     d pA     = -g_phase x (q^ - c p^) / N,  N = max(|p|, eps), c = <p / N, q^>, p^ = p / |p| (0 at p = 0), q^ = q / max(|q|, eps)
//   -- what autograd derives: ATen clamps the norm's VALUE and still differentiates the norm (d|p| = p^), so a p shorter than
//   eps keeps the second term, scaled by the clamped N.  A zero target has q^ = 0: no value, no gradient.  The residual is one
//   fused multiply-add, so its sign is the exact one.
// Per-bin arithmetic is fp32 (a few roundings of quantities bounded by x), every sum fp64 in a fixed order: no atomics, two
// runs give the same bits.
// =================================================================================================
namespace lossphase {
constexpr int NBLK = 32;        // slices per utterance
constexpr int NS = 8;           // partial sums per slice
constexpr float EPS = 1e-8f;

__device__ __forceinline__ float2 unit_clamped(float2 v) {      // v / max(|v|, eps)
  const float d = fmaxf(sqrtf(v.x * v.x + v.y * v.y), EPS);
  return make_float2(v.x / d, v.y / d);
}
__device__ __forceinline__ float dot2(float2 a, float2 b) { return a.x * b.x + a.y * b.y; }
}  // namespace lossphase

__global__ __launch_bounds__(256) void loss_phase_kernel(const float* __restrict__ mask_a, const float* __restrict__ mask_b,
                                                         long m_sb, long m_se, const float* __restrict__ mag,
                                                         const float* __restrict__ s1, const float* __restrict__ s2,
                                                         const float2* __restrict__ pa, const float2* __restrict__ pb,
                                                         const float2* __restrict__ q1, const float2* __restrict__ q2, int TF,
                                                         double* __restrict__ partial) {
  using namespace lossphase;
  __shared__ double red[NS][256];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int per = (TF + NBLK - 1) / NBLK, e0 = blockIdx.x * per, e1 = e0 + per < TF ? e0 + per : TF;
  double acc[NS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int e = e0 + tid; e < e1; e += 256) {
    const long i = (long)b * TF + e;
    const float x = mag[i], t1 = s1[i], t2 = s2[i];
    const float ma = mask_a[(long)b * m_sb + (long)e * m_se], mb = mask_b[(long)b * m_sb + (long)e * m_se];
    const float2 ua = unit_clamped(pa[i]), ub = unit_clamped(pb[i]), u1 = unit_clamped(q1[i]), u2 = unit_clamped(q2[i]);
    acc[0] += fabsf(fmaf(ma, x, -t1)); acc[1] += fabsf(fmaf(mb, x, -t2));
    acc[2] += fabsf(fmaf(mb, x, -t1)); acc[3] += fabsf(fmaf(ma, x, -t2));
    acc[4] += x * dot2(ua, u1); acc[5] += x * dot2(ub, u2);
    acc[6] += x * dot2(ub, u1); acc[7] += x * dot2(ua, u2);
  }
#pragma unroll
  for (int k = 0; k < NS; ++k) red[k][tid] = acc[k];
  __syncthreads();
  for (int sft = 128; sft > 0; sft >>= 1) {
    if (tid < sft)
      for (int k = 0; k < NS; ++k) red[k][tid] += red[k][tid + sft];
    __syncthreads();
  }
  if (tid < NS) partial[((long)b * NBLK + blockIdx.x) * NS + tid] = red[tid][0];
}

__global__ void loss_phase_final_kernel(const double* __restrict__ partial, int B, float* __restrict__ out_mask,
                                        float* __restrict__ out_phase, int* __restrict__ perm_out) {
  using namespace lossphase;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double s[NS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < NBLK; ++k)
    for (int j = 0; j < NS; ++j) s[j] += partial[((long)b * NBLK + k) * NS + j];
  const double l1 = s[0] + s[1], l2 = s[2] + s[3];
  const bool straight = l1 < l2;                   // strictly: a tie takes the swapped assignment
  out_mask[b] = (float)(straight ? l1 : l2);
  out_phase[b] = (float)(straight ? -(s[4] + s[5]) : -(s[6] + s[7]));
  perm_out[b] = straight ? 0 : 1;
}

__global__ __launch_bounds__(256) void loss_phase_grad_kernel(const float* __restrict__ mask_a, const float* __restrict__ mask_b,
                                                              long m_sb, long m_se, const float* __restrict__ mag,
                                                              const float* __restrict__ s1, const float* __restrict__ s2,
                                                              const float2* __restrict__ pa, const float2* __restrict__ pb,
                                                              const float2* __restrict__ q1, const float2* __restrict__ q2, int TF,
                                                              const float* __restrict__ g_mask, const float* __restrict__ g_phase,
                                                              const int* __restrict__ perm, float* __restrict__ d_a,
                                                              float* __restrict__ d_b, long d_sb, long d_se,
                                                              float2* __restrict__ d_pa, float2* __restrict__ d_pb) {
  using namespace lossphase;
  const int b = blockIdx.y;
  const float gm = g_mask[b], gp = g_phase[b];
  const bool swap = perm[b] != 0;
  auto dphase = [](float2 p, float2 q, float k) {      // k * d cos(p, q) / dp
    const float2 u = unit_clamped(q);
    const float n = sqrtf(p.x * p.x + p.y * p.y), nc = fmaxf(n, EPS);
    const float2 ph = n > 0.0f ? make_float2(p.x / n, p.y / n) : make_float2(0.0f, 0.0f);
    const float c = dot2(make_float2(p.x / nc, p.y / nc), u);
    return make_float2(k * ((u.x - c * ph.x) / nc), k * ((u.y - c * ph.y) / nc));
  };
  for (int e = blockIdx.x * 256 + threadIdx.x; e < TF; e += gridDim.x * 256) {
    const long i = (long)b * TF + e;
    const float x = mag[i], t1 = s1[i], t2 = s2[i];
    const float2 v1 = q1[i], v2 = q2[i];
    const float ra = fmaf(mask_a[(long)b * m_sb + (long)e * m_se], x, -(swap ? t2 : t1));
    const float rb = fmaf(mask_b[(long)b * m_sb + (long)e * m_se], x, -(swap ? t1 : t2));
    d_a[(long)b * d_sb + (long)e * d_se] = gm * x * (ra > 0.0f ? 1.0f : ra < 0.0f ? -1.0f : 0.0f);
    d_b[(long)b * d_sb + (long)e * d_se] = gm * x * (rb > 0.0f ? 1.0f : rb < 0.0f ? -1.0f : 0.0f);
    d_pa[i] = dphase(pa[i], swap ? v2 : v1, -gp * x);
    d_pb[i] = dphase(pb[i], swap ? v1 : v2, -gp * x);
  }
}

extern "C" {

size_t onssen_loss_phase_workspace_bytes(int B) {
  return B > 0 ? (size_t)B * lossphase::NBLK * lossphase::NS * sizeof(double) : 0;
}

int onssen_loss_phase_f32(const float* mask_a, const float* mask_b, int64_t m_sb, int64_t m_se, const float* mag_mix,
                          const float* mag_s1, const float* mag_s2, const float* phase_a, const float* phase_b,
                          const float* phase_s1, const float* phase_s2, int B, int TF, float* out_mask, float* out_phase,
                          int32_t* perm, void* ws, size_t ws_bytes, void* stream) {
  using namespace lossphase;
  if (!mask_a || !mask_b || !mag_mix || !mag_s1 || !mag_s2 || !phase_a || !phase_b || !phase_s1 || !phase_s2 || !out_mask ||
      !out_phase || !perm || !ws || B <= 0 || B > 65535 || TF <= 0)
    return ONSSEN_E_ARG;
  if ((reinterpret_cast<uintptr_t>(phase_a) | reinterpret_cast<uintptr_t>(phase_b) | reinterpret_cast<uintptr_t>(phase_s1) |
       reinterpret_cast<uintptr_t>(phase_s2) | reinterpret_cast<uintptr_t>(ws)) & 7u)
    return ONSSEN_E_ALIGN;                          // (re, im) pairs are read as one 8-byte word; the partial sums are fp64
  if (ws_bytes < onssen_loss_phase_workspace_bytes(B)) return ONSSEN_E_WORKSPACE;
  ONSSEN_CLEAR_ERROR();
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(loss_phase_kernel, dim3(NBLK, (unsigned)B), dim3(256), 0, st, mask_a, mask_b, (long)m_sb, (long)m_se, mag_mix,
                     mag_s1, mag_s2, (const float2*)phase_a, (const float2*)phase_b, (const float2*)phase_s1,
                     (const float2*)phase_s2, TF, (double*)ws);
  hipLaunchKernelGGL(loss_phase_final_kernel, dim3((unsigned)ceil_div(B, 64)), dim3(64), 0, st, (const double*)ws, B, out_mask,
                     out_phase, (int*)perm);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_loss_phase_grad_f32(const float* mask_a, const float* mask_b, int64_t m_sb, int64_t m_se, const float* mag_mix,
                               const float* mag_s1, const float* mag_s2, const float* phase_a, const float* phase_b,
                               const float* phase_s1, const float* phase_s2, int B, int TF, const float* g_mask,
                               const float* g_phase, const int32_t* perm, float* d_mask_a, float* d_mask_b, int64_t d_sb,
                               int64_t d_se, float* d_phase_a, float* d_phase_b, void* stream) {
  if (!mask_a || !mask_b || !mag_mix || !mag_s1 || !mag_s2 || !phase_a || !phase_b || !phase_s1 || !phase_s2 || !g_mask ||
      !g_phase || !perm || !d_mask_a || !d_mask_b || !d_phase_a || !d_phase_b || B <= 0 || B > 65535 || TF <= 0)
    return ONSSEN_E_ARG;
  if ((reinterpret_cast<uintptr_t>(phase_a) | reinterpret_cast<uintptr_t>(phase_b) | reinterpret_cast<uintptr_t>(phase_s1) |
       reinterpret_cast<uintptr_t>(phase_s2) | reinterpret_cast<uintptr_t>(d_phase_a) | reinterpret_cast<uintptr_t>(d_phase_b)) & 7u)
    return ONSSEN_E_ALIGN;
  ONSSEN_CLEAR_ERROR();
  const int nblk = ceil_div(TF, 256) < 64 ? ceil_div(TF, 256) : 64;
  hipLaunchKernelGGL(loss_phase_grad_kernel, dim3((unsigned)nblk, (unsigned)B), dim3(256), 0, (hipStream_t)stream, mask_a, mask_b,
                     (long)m_sb, (long)m_se, mag_mix, mag_s1, mag_s2, (const float2*)phase_a, (const float2*)phase_b,
                     (const float2*)phase_s1, (const float2*)phase_s2, TF, g_mask, g_phase, (const int*)perm, d_mask_a, d_mask_b,
                     (long)d_sb, (long)d_se, (float2*)d_phase_a, (float2*)d_phase_b);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

}  // extern "C"
