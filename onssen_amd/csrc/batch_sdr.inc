// N4 batch SI-SDR with best permutation: its kernels and its C ABI entries (part of onssen_hip.hip).
// =================================================================================================
// onssen/evaluate/sdr.py:11-87 (calc_sdr_torch + batch_SDR_torch).
// Everything the metric needs per utterance is the Gram matrix of the 2C zero-mean (optionally masked) signals
// [est_0..est_{C-1}, org_0..org_{C-1}]: pass 1 sums the signals (means), pass 2 the centred products, a last
// workgroup per utterance forms the C x C SDR table and scans the C! permutations in the reference's
// (lexicographic) order.  The separated waveforms never leave the device.
// The reference sums (est - scale*org)^2 directly; from a Gram matrix the residual power is ee - 2 s eo + s^2 oo, which
// cancels: with fp32 sums it is wrong by 0.1 dB at 50 dB SDR and negative (NaN) from ~70 dB.  The Gram matrix, the
// means and the table are therefore accumulated and evaluated in fp64 (good to ~140 dB, the resolution of the fp32 inputs).
// =================================================================================================
namespace sdr {
using pit::CMAX;
constexpr int NBLK = 32, SMAX = 2 * CMAX, TS = 256;
constexpr int PSTRIDE = SMAX * SMAX + SMAX;     // per (b, block): Gram then sums
}  // namespace sdr

template <int PASS>
__global__ __launch_bounds__(256) void sdr_partial_kernel(const float* __restrict__ est, const float* __restrict__ org,
                                                          const float* __restrict__ mask, int C, int n,
                                                          const double* __restrict__ means, double* __restrict__ partial,
                                                          const int* __restrict__ lengths) {
  using namespace sdr;
  __shared__ float tile[SMAX][TS + 1];
  const int tid = threadIdx.x, blk = blockIdx.x, b = blockIdx.y, S = 2 * C;
  // ragged batch: row b holds lengths[b] <= n samples of its own (rows keep the stride n; the padding takes no part)
  const int nb = lengths ? lengths[b] : n;
  const int per = (nb + NBLK - 1) / NBLK, s0 = blk * per, s1 = s0 + per < nb ? s0 + per : nb;
  float mu[SMAX];
#pragma unroll
  for (int k = 0; k < SMAX; ++k) mu[k] = (PASS == 1 && k < S) ? (float)means[b * SMAX + k] : 0.0f;   // the reference subtracts an fp32 mean
  double acc = 0.0;                              // PASS 0: thread k < S sums signal k; PASS 1: thread o < S*S -> G[o/S][o%S]
  for (int t0 = s0; t0 < s1; t0 += TS) {
    const int nt = s1 - t0 < TS ? s1 - t0 : TS;
    __syncthreads();
    for (int e = tid; e < S * TS; e += 256) {
      const int k = e / TS, i = e % TS;
      float v = 0.0f;
      if (i < nt) {
        const float* src = (k < C ? est + ((long)b * C + k) * n : org + ((long)b * C + (k - C)) * n);
        v = src[t0 + i];
        if (PASS == 1) {
          v -= mu[k];
          if (mask) v *= mask[(long)b * n + t0 + i];
        }
      }
      tile[k][i] = v;
    }
    __syncthreads();
    if (PASS == 0) {
      if (tid < S) for (int i = 0; i < nt; ++i) acc += tile[tid][i];
    } else if (tid < S * S) {
      const int k = tid / S, l = tid % S;
      for (int i = 0; i < nt; ++i) acc += (double)tile[k][i] * (double)tile[l][i];
    }
  }
  double* dst = partial + ((long)b * NBLK + blk) * PSTRIDE;
  if (PASS == 0) {
    if (tid < S) dst[SMAX * SMAX + tid] = acc;
  } else if (tid < S * S) {
    dst[tid] = acc;
  }
}

__global__ void sdr_means_kernel(const double* __restrict__ partial, int C, int n, double* __restrict__ means,
                                 const int* __restrict__ lengths) {
  using namespace sdr;
  const int b = blockIdx.x, k = threadIdx.x;
  if (lengths) n = lengths[b];
  if (k < 2 * C) {
    double s = 0.0;
    for (int blk = 0; blk < NBLK; ++blk) s += partial[((long)b * NBLK + blk) * PSTRIDE + SMAX * SMAX + k];
    means[b * SMAX + k] = s / n;
  }
}

__global__ void sdr_final_kernel(const double* __restrict__ partial, int C, float* __restrict__ sdr_out, int* __restrict__ perm_out) {
  using namespace sdr;
  __shared__ double G[SMAX][SMAX];
  __shared__ float tab[CMAX][CMAX];
  const int b = blockIdx.x, tid = threadIdx.x, S = 2 * C;
  if (tid < S * S) {
    double s = 0.0;
    for (int blk = 0; blk < NBLK; ++blk) s += partial[((long)b * NBLK + blk) * PSTRIDE + tid];
    G[tid / S][tid % S] = s;
  }
  __syncthreads();
  if (tid < C * C) {       // SDR[i][j] of estimate i against source j (sdr.py:23-33)
    const int i = tid / C, j = tid % C;
    const double oo = G[C + j][C + j], ee = G[i][i], eo = G[i][C + j];
    const double scale = eo / (oo + 1e-8);
    const double true_p = scale * scale * oo + 1e-8;
    const double res = ee - 2.0 * scale * eo + scale * scale * oo;        // >= 0 up to rounding
    const double res_p = (res > 0.0 ? res : 0.0) + 1e-8;
    tab[i][j] = (float)(10.0 * log10(true_p) - 10.0 * log10(res_p));
  }
  __syncthreads();
  if (tid == 0) {          // permutations in lexicographic order (sorted(set(permutations(range(C)))), sdr.py:74)
    pit::Perms e(C);
    int best_idx = 0;
    float best = -3.0e38f;                             // (no sum of a NaN table is accepted: -3e38 / C and index 0)
    do {
      float v = 0.0f;
      for (int k = 0; k < C; ++k) v += tab[k][e.p(k)];
      if (v > best) { best = v; best_idx = e.idx; }    // torch.max keeps the first maximum
    } while (e.next());
    sdr_out[b] = best / (float)C;
    if (perm_out) perm_out[b] = best_idx;
  }
}

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" {

size_t onssen_batch_sdr_workspace_bytes(int B) {
  return B > 0 ? ((size_t)B * sdr::NBLK * sdr::PSTRIDE + (size_t)B * sdr::SMAX) * sizeof(double) : 0;
}

static int batch_sdr_impl(const float* est, const float* org, const float* mask, int B, int C, int n, float* sdr_out,
                          int* perm_out, void* ws, size_t ws_bytes, void* stream, const int32_t* lengths) {
  if (!est || !org || !sdr_out || !ws || B <= 0 || C <= 0 || C > sdr::CMAX || n <= C) return ONSSEN_E_ARG;
  if (ws_bytes < onssen_batch_sdr_workspace_bytes(B)) return ONSSEN_E_WORKSPACE;
  ONSSEN_CLEAR_ERROR();
  hipStream_t st = (hipStream_t)stream;
  if ((reinterpret_cast<uintptr_t>(ws) & 7u) != 0) return ONSSEN_E_ALIGN;
  double* partial = (double*)ws;      // fp64 sums: see the note at the top
  double* means = partial + (size_t)B * sdr::NBLK * sdr::PSTRIDE;
  const dim3 grid(sdr::NBLK, (unsigned)B);
  hipLaunchKernelGGL((sdr_partial_kernel<0>), grid, dim3(256), 0, st, est, org, mask, C, n, (const double*)nullptr, partial, lengths);
  hipLaunchKernelGGL(sdr_means_kernel, dim3((unsigned)B), dim3(64), 0, st, (const double*)partial, C, n, means, lengths);
  hipLaunchKernelGGL((sdr_partial_kernel<1>), grid, dim3(256), 0, st, est, org, mask, C, n, (const double*)means, partial, lengths);
  hipLaunchKernelGGL(sdr_final_kernel, dim3((unsigned)B), dim3(64), 0, st, (const double*)partial, C, sdr_out, perm_out);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_batch_sdr_f32(const float* est, const float* org, const float* mask, int B, int C, int n, float* sdr_out,
                         int* perm_out, void* ws, size_t ws_bytes, void* stream) {
  return batch_sdr_impl(est, org, mask, B, C, n, sdr_out, perm_out, ws, ws_bytes, stream, nullptr);
}

int onssen_batch_sdr_ragged_f32(const float* est, const float* org, const float* mask, int B, int C, int n,
                                const int32_t* lengths, float* sdr_out, int* perm_out, void* ws, size_t ws_bytes,
                                void* stream) {
  if (!lengths) return ONSSEN_E_ARG;
  return batch_sdr_impl(est, org, mask, B, C, n, sdr_out, perm_out, ws, ws_bytes, stream, lengths);
}

}  // extern "C"
