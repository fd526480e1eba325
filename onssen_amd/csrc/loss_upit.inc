// Utterance-level permutation-invariant mask loss for 2 .. 4 speakers, value and gradient (part of onssen_hip.hip).
// =================================================================================================
// The loss of the uPIT mask network (onssen/nn/uPIT-LSTM.py has the network only; upstream has no loss for it).  Per utterance b,
// over its bins, with the mixture magnitude x, the S mask estimates m_k and the S targets
//   t_j = mag_s_j (MSA)   or   min(x, relu(mag_s_j cos_j)) (PSA: the transform of loss_mask_kernel):
//   pair[k][j] = sum_bins |m_k x - t_j|
//   total[p]   = sum_k pair[k][p[k]]   for the S! assignments p in the order of itertools.permutations(range(S))
//   out = min_p total[p],  perm = the index of that p; of equal totals the smallest index (a strict less-than in the scan)
// For S = 2 this is the chimera mask term (loss_mask_kernel) and its perm word.
//   loss_upit_kernel<S, PSA>       grid (NBLK, B): a workgroup reads its slice of the 1 + 2S (MSA) / 1 + 3S (PSA) maps ONCE and
//                                  writes S S fp64 partial sums.  A thread takes FOUR consecutive bins per pass: the contiguous
//                                  maps come as one 16-byte load each where the row is aligned, as four loads where it is not --
//                                  the same bins in the same order either way, so alignment never shows in the bits.  The masks are
//                                  read through strides (the network's interleaved (.., S) buffer where it lies, or S maps).
//                                  Sums: per thread, then across the wave by shuffles (all S S at once: wave_sum_spread), then
//                                  the four waves through 4 S S doubles of LDS (not S S x 256).
//   loss_upit_final_kernel         one workgroup per utterance: adds the slices in order, scans the S! assignments in fp64
//   loss_upit_grad_kernel<S, PSA>  one elementwise pass: d m_k = g[b] x sign(m_k x - t_p[k]), sign(0) = 0 (as loss_mask_grad_kernel)
// Per-bin arithmetic is fp32 -- the residual is one fused multiply-add, so its sign is the exact one -- every sum fp64 in a
// fixed order: no atomics, no waits between workgroups, a workspace that needs no zeroing, two runs give the same bits.
// Ragged rows: with `frames`, row b covers its first frames[b] F bins only; the slices are cut from THAT count, so the row's
// value is bit for bit the one of a batch-1 call on its own frames; the gradient beyond them is written as zero.
// =================================================================================================
namespace upit {
constexpr int NBLK = 32;        // slices per utterance
constexpr int SMAX = 4;

// bins of row b: all TF, or the first frames[b] * F of them (clamped to [0, TF]: frames is device data)
__device__ __forceinline__ int row_bins(const int* __restrict__ frames, int b, int F, int TF) {
  if (!frames) return TF;
  const long n = (long)frames[b] * F;
  return n < 0 ? 0 : n > TF ? TF : (int)n;
}
// bins per slice: a multiple of 4, so that every slice of an aligned row starts on a 16-byte boundary
__device__ __forceinline__ int slice_bins(int n) { return ((n + NBLK - 1) / NBLK + 3) & ~3; }

__host__ __device__ constexpr int factorial(int s) { return s <= 1 ? 1 : s * factorial(s - 1); }

// assignment number idx (the order of itertools.permutations(range(S)): lexicographic) as nibbles, p[k] = (r >> 4 k) & 15
__device__ __forceinline__ unsigned perm_nibbles(int S, int idx) {
  unsigned avail = 0x3210u, r = 0;
  int f = factorial(S - 1);
  for (int k = 0; k < S; ++k) {
    const int d = idx / f;
    idx -= d * f;
    r |= ((avail >> (4 * d)) & 15u) << (4 * k);
    avail = (avail & ((1u << (4 * d)) - 1u)) | ((avail >> (4 * d + 4)) << (4 * d));       // drop nibble d
    if (S - 1 - k > 1) f /= S - 1 - k;
  }
  return r;
}

// four consecutive floats from p + t (nv of them are inside the slice): one 16-byte load where the row allows it
__device__ __forceinline__ void load4(const float* __restrict__ p, long t, int nv, bool vec, float (&v)[4]) {
  if (vec && nv == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p + t);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = j < nv ? p[t + j] : 0.0f;
  }
}

// Wave sums of N = 2^L values per lane at once, in N - 1 + (6 - L) shuffles instead of 6 N: at each of the first L steps a lane
// keeps one half of its values and hands the other half to its partner, so the values spread over the lanes while they are
// summed.  Lane q * (64 / N) ends up with the wave's sum of value q (every other lane of its group of 64 / N with the same).
template <int N>
__device__ __forceinline__ double wave_sum_spread(double (&v)[N], int lane) {
  int m = 32;
#pragma unroll
  for (int half = N / 2; half >= 1; half >>= 1) {
    const bool hi = (lane & m) != 0;
#pragma unroll
    for (int i = 0; i < half; ++i) {
      const double keep = hi ? v[i + half] : v[i], send = hi ? v[i] : v[i + half];
      v[i] = keep + __shfl_xor(send, m);
    }
    m >>= 1;
  }
  for (; m >= 1; m >>= 1) v[0] += __shfl_xor(v[0], m);
  return v[0];
}
}  // namespace upit

template <int S, bool PSA>
__global__ __launch_bounds__(256) void loss_upit_kernel(const float* __restrict__ masks, long m_sb, long m_se, long m_ss,
                                                        const float* __restrict__ mag, const float* __restrict__ src, long s_sd,
                                                        const float* __restrict__ cs, long c_sd, const int* __restrict__ frames,
                                                        int F, int TF, double* __restrict__ partial) {
  using namespace upit;
  __shared__ double red[4][S * S];
  const int tid = threadIdx.x, b = blockIdx.y, wave = tid >> 6, lane = tid & 63;
  const int n = row_bins(frames, b, F, TF), per = slice_bins(n), e0 = (int)blockIdx.x * per;
  if (e0 >= n) return;                               // (the whole workgroup) an empty slice: the final kernel does not read it
  const int e1 = e0 + per < n ? e0 + per : n;
  const long row = (long)b * TF;
  // e0 is a multiple of 4: the 16-byte loads need the row's start and the distances between the maps aligned
  uintptr_t al = reinterpret_cast<uintptr_t>(mag + row) | reinterpret_cast<uintptr_t>(src + row) | (uintptr_t)(s_sd * 4);
  if (PSA) al |= reinterpret_cast<uintptr_t>(cs + row) | (uintptr_t)(c_sd * 4);
  const bool vec = (al & 15u) == 0;
  double acc[S][S];
#pragma unroll
  for (int k = 0; k < S; ++k)
#pragma unroll
    for (int j = 0; j < S; ++j) acc[k][j] = 0.0;
  for (int t = e0 + 4 * tid; t < e1; t += 4 * 256) {
    const int nv = e1 - t < 4 ? e1 - t : 4;
    float x[4], tg[S][4];
    load4(mag, row + t, nv, vec, x);
#pragma unroll
    for (int j = 0; j < S; ++j) {
      load4(src + j * s_sd, row + t, nv, vec, tg[j]);
      if (PSA) {
        float c[4];
        load4(cs + j * c_sd, row + t, nv, vec, c);
#pragma unroll
        for (int e = 0; e < 4; ++e) tg[j][e] = fminf(x[e], fmaxf(tg[j][e] * c[e], 0.0f));
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e < nv) {
        const float* mp = masks + (long)b * m_sb + (long)(t + e) * m_se;
#pragma unroll
        for (int k = 0; k < S; ++k) {
          const float m = mp[k * m_ss];
#pragma unroll
          for (int j = 0; j < S; ++j) acc[k][j] += (double)fabsf(fmaf(m, x[e], -tg[j][e]));
        }
      }
    }
  }
  constexpr int NV = S == 2 ? 4 : 16, GROUP = 64 / NV;     // the S S sums padded to a power of two
  double v[NV];
#pragma unroll
  for (int q = 0; q < NV; ++q) v[q] = q < S * S ? acc[q / S][q % S] : 0.0;
  const double a = wave_sum_spread<NV>(v, lane);
  if (lane % GROUP == 0 && lane / GROUP < S * S) red[wave][lane / GROUP] = a;
  __syncthreads();
  if (tid < S * S)
    partial[((long)b * NBLK + blockIdx.x) * (S * S) + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

__global__ __launch_bounds__(64) void loss_upit_final_kernel(const double* __restrict__ partial, const int* __restrict__ frames,
                                                             int F, int TF, int S, float* __restrict__ out,
                                                             int* __restrict__ perm_out, float* __restrict__ pair_out) {
  using namespace upit;
  __shared__ double pair[SMAX * SMAX];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int n = row_bins(frames, b, F, TF), per = slice_bins(n), nch = n > 0 ? (n + per - 1) / per : 0;
  if (tid < S * S) {
    double s = 0.0;
    for (int c = 0; c < nch; ++c) s += partial[((long)b * NBLK + c) * (S * S) + tid];          // slice order: fixed
    pair[tid] = s;
    if (pair_out) pair_out[(long)b * S * S + tid] = (float)s;
  }
  __syncthreads();
  if (tid == 0) {
    double best = 0.0;
    int best_idx = 0;
    const int np = factorial(S);
    for (int idx = 0; idx < np; ++idx) {
      const unsigned p = perm_nibbles(S, idx);
      double v = 0.0;
      for (int k = 0; k < S; ++k) v += pair[k * S + ((p >> (4 * k)) & 15u)];
      if (idx == 0 || v < best) { best = v; best_idx = idx; }                                   // strict: the first minimum wins
    }
    out[b] = (float)best;
    if (perm_out) perm_out[b] = best_idx;
  }
}

template <int S, bool PSA>
__global__ __launch_bounds__(256) void loss_upit_grad_kernel(const float* __restrict__ masks, long m_sb, long m_se, long m_ss,
                                                             const float* __restrict__ mag, const float* __restrict__ src, long s_sd,
                                                             const float* __restrict__ cs, long c_sd,
                                                             const int* __restrict__ frames, int F, int TF,
                                                             const float* __restrict__ g, const int* __restrict__ perm,
                                                             float* __restrict__ d_masks, long d_sb, long d_se, long d_ss) {
  using namespace upit;
  const int b = blockIdx.y;
  const int n = row_bins(frames, b, F, TF);
  const float gb = g[b];
  int idx = perm[b];
  idx = idx < 0 ? 0 : idx >= factorial(S) ? factorial(S) - 1 : idx;      // (device data: an index outside the table is clamped)
  const unsigned p = perm_nibbles(S, idx);
  for (int e = blockIdx.x * 256 + threadIdx.x; e < TF; e += gridDim.x * 256) {
    float* dp = d_masks + (long)b * d_sb + (long)e * d_se;
    if (e >= n) {
#pragma unroll
      for (int k = 0; k < S; ++k) dp[k * d_ss] = 0.0f;
      continue;
    }
    const long i = (long)b * TF + e;
    const float x = mag[i];
    float t[S];
#pragma unroll
    for (int j = 0; j < S; ++j) {
      t[j] = src[j * s_sd + i];
      if (PSA) t[j] = fminf(x, fmaxf(t[j] * cs[j * c_sd + i], 0.0f));
    }
    const float* mp = masks + (long)b * m_sb + (long)e * m_se;
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const int pk = (int)((p >> (4 * k)) & 15u);
      float tk = t[0];
#pragma unroll
      for (int j = 1; j < S; ++j) tk = pk == j ? t[j] : tk;
      const float r = fmaf(mp[k * m_ss], x, -tk);
      dp[k * d_ss] = gb * x * (r > 0.0f ? 1.0f : r < 0.0f ? -1.0f : 0.0f);
    }
  }
}

static int loss_upit_args_bad(const float* masks, const float* mag_mix, const float* mag_src, const int32_t* frames, int F, int B,
                              int TF, int S) {
  if (!masks || !mag_mix || !mag_src || B <= 0 || B > 65535 || TF < 1 || S < 2 || S > upit::SMAX) return 1;
  return frames && (F <= 0 || TF % F != 0);
}

extern "C" {

size_t onssen_loss_upit_workspace_bytes(int B, int S) {
  return B > 0 && S >= 2 && S <= upit::SMAX ? (size_t)B * upit::NBLK * S * S * sizeof(double) : 0;
}

int onssen_loss_upit_f32(const float* masks, int64_t m_sb, int64_t m_se, int64_t m_ss, const float* mag_mix, const float* mag_src,
                         int64_t s_sd, const float* cos_src, int64_t c_sd, const int32_t* frames, int F, int B, int TF, int S,
                         float* out, int32_t* perm, float* pair, void* ws, size_t ws_bytes, void* stream) {
  using namespace upit;
  if (loss_upit_args_bad(masks, mag_mix, mag_src, frames, F, B, TF, S) || !out || !ws) return ONSSEN_E_ARG;
  if (reinterpret_cast<uintptr_t>(ws) & 7u) return ONSSEN_E_ALIGN;          // the partial sums are fp64
  if (ws_bytes < onssen_loss_upit_workspace_bytes(B, S)) return ONSSEN_E_WORKSPACE;
  ONSSEN_CLEAR_ERROR();
  hipStream_t st = (hipStream_t)stream;
  double* partial = (double*)ws;
  const dim3 grid(NBLK, (unsigned)B);
#define ONSSEN_UPIT_FWD(S_, PSA_)                                                                                            \
  hipLaunchKernelGGL((loss_upit_kernel<S_, PSA_>), grid, dim3(256), 0, st, masks, (long)m_sb, (long)m_se, (long)m_ss, mag_mix, \
                     mag_src, (long)s_sd, cos_src, (long)c_sd, (const int*)frames, F, TF, partial)
  if (cos_src) {
    if (S == 2) ONSSEN_UPIT_FWD(2, true); else if (S == 3) ONSSEN_UPIT_FWD(3, true); else ONSSEN_UPIT_FWD(4, true);
  } else {
    if (S == 2) ONSSEN_UPIT_FWD(2, false); else if (S == 3) ONSSEN_UPIT_FWD(3, false); else ONSSEN_UPIT_FWD(4, false);
  }
#undef ONSSEN_UPIT_FWD
  hipLaunchKernelGGL(loss_upit_final_kernel, dim3((unsigned)B), dim3(64), 0, st, (const double*)partial, (const int*)frames, F, TF, S,
                     out, (int*)perm, pair);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_loss_upit_grad_f32(const float* masks, int64_t m_sb, int64_t m_se, int64_t m_ss, const float* mag_mix,
                              const float* mag_src, int64_t s_sd, const float* cos_src, int64_t c_sd, const int32_t* frames, int F,
                              int B, int TF, int S, const float* g, const int32_t* perm, float* d_masks, int64_t d_sb, int64_t d_se,
                              int64_t d_ss, void* stream) {
  if (loss_upit_args_bad(masks, mag_mix, mag_src, frames, F, B, TF, S) || !g || !perm || !d_masks) return ONSSEN_E_ARG;
  ONSSEN_CLEAR_ERROR();
  hipStream_t st = (hipStream_t)stream;
  const int nblk = ceil_div(TF, 256) < 64 ? ceil_div(TF, 256) : 64;
  const dim3 grid((unsigned)nblk, (unsigned)B);
#define ONSSEN_UPIT_BWD(S_, PSA_)                                                                                                  \
  hipLaunchKernelGGL((loss_upit_grad_kernel<S_, PSA_>), grid, dim3(256), 0, st, masks, (long)m_sb, (long)m_se, (long)m_ss, mag_mix, \
                     mag_src, (long)s_sd, cos_src, (long)c_sd, (const int*)frames, F, TF, g, (const int*)perm, d_masks, (long)d_sb,  \
                     (long)d_se, (long)d_ss)
  if (cos_src) {
    if (S == 2) ONSSEN_UPIT_BWD(2, true); else if (S == 3) ONSSEN_UPIT_BWD(3, true); else ONSSEN_UPIT_BWD(4, true);
  } else {
    if (S == 2) ONSSEN_UPIT_BWD(2, false); else if (S == 3) ONSSEN_UPIT_BWD(3, false); else ONSSEN_UPIT_BWD(4, false);
  }
#undef ONSSEN_UPIT_BWD
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

}  // extern "C"
