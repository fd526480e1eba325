// Waveform-approximation loss: the L1 distance of C estimated waveforms to C references under the best speaker permutation, and
// its gradient (part of onssen_hip.hip).  Wang, Le Roux, Wang & Hershey 2018 ("waveform approximation"); no upstream counterpart.
// =================================================================================================
// Per row b with n_b valid samples and C <= 4 speakers:
//   D[b,i,j]   = sum_{n < n_b} |est_i[n] - ref_j[n]|                        fp64, fixed summation order
//   V[b]       = min over permutations p of sum_i D[b,i,p(i)] / (C n_b)     lexicographic order, the first minimum wins
//   d est_i[n] = w_b sign(est_i[n] - ref_p(i)[n]) / (C n_b)                 0 at equality and at n >= n_b
// with w_b = g_value[b] + g_total / B, total = sum_b V[b] / B.
//   wa_partial_kernel   grid (chunks, rows): a workgroup reads its chunk of all 2C signals ONCE and writes the C^2 fp64 partial sums
//   wa_final_kernel     one wave per row: partials merged in chunk order, the permutation scan, V_b, the assignment for the backward
//   wa_total_kernel     the batch mean, a fixed-order sum over the rows
//   wa_backward_kernel  one elementwise pass that reads the assignment the forward left in the workspace
// The structure is loss_sisnr.inc's: a row's chunking depends on its own length only, a thread's samples on nothing else, every sum
// has a fixed order (no atomics), the workspace needs no zeroing; aligned rows are fetched 16 bytes at a time, others 4, in the
// same order -- bit-repeatable and independent of the batch.
// est is (B, C, n) contiguous (the inverse transform's output); ref (b, j) starts at ref + b r_sb + j r_sc, unit sample stride.
// =================================================================================================
namespace wa {
constexpr int CMAX = 4;
constexpr int NCH = 64;                         // chunks of a row at most
constexpr int CHMIN = 1024;                     // samples of a chunk at least
constexpr int ND = CMAX * CMAX;                 // sums per (row, chunk)
__host__ __device__ inline int chunk_len(int len) {
  const int per = ((len + NCH - 1) / NCH + 3) & ~3;
  return per < CHMIN ? CHMIN : per;
}
__device__ __forceinline__ int row_len(const int* lengths, int b, int n) {
  const int l = lengths ? lengths[b] : n;
  return l < 1 ? 1 : l > n ? n : l;               // a device-side length cannot be refused by the host: it is clamped
}
}  // namespace wa

template <int K, bool VEC>
__global__ __launch_bounds__(256) void wa_partial_kernel(const float* __restrict__ est, const float* __restrict__ ref, long r_sb,
                                                         long r_sc, int n, const int* __restrict__ lengths,
                                                         double* __restrict__ partial) {
  using namespace wa;
  __shared__ double red[4][ND];
  const int tid = threadIdx.x, b = blockIdx.y, wave = tid >> 6, lane = tid & 63;
  const int len = row_len(lengths, b, n), per = chunk_len(len), c0 = (int)blockIdx.x * per;
  if (c0 >= len) return;                           // (the whole workgroup) this row has fewer chunks than the longest
  const int c1 = c0 + per < len ? c0 + per : len;
  const float* xp[K];
  const float* sp[K];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    xp[i] = est + ((long)b * K + i) * n;
    sp[i] = ref + (long)b * r_sb + (long)i * r_sc;
  }
  double d[K][K];
#pragma unroll
  for (int i = 0; i < K; ++i)
#pragma unroll
    for (int j = 0; j < K; ++j) d[i][j] = 0.0;
  for (int t = c0 + 4 * tid; t < c1; t += 4 * 256) {
    const int nv = c1 - t < 4 ? c1 - t : 4;
    float xv[K][4], sv[K][4];
#pragma unroll
    for (int i = 0; i < K; ++i) {
      sisnr_load4<VEC>(xp[i], t, nv, xv[i]);
      sisnr_load4<VEC>(sp[i], t, nv, sv[i]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e < nv) {
#pragma unroll
        for (int i = 0; i < K; ++i)
#pragma unroll
          for (int j = 0; j < K; ++j) d[i][j] += fabs((double)xv[i][e] - (double)sv[j][e]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < K; ++i)
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const double a = tas::wave_sum_d(d[i][j]);
      if (lane == 0) red[wave][i * CMAX + j] = a;
    }
  __syncthreads();
  if (tid < ND && tid / CMAX < K && tid % CMAX < K)
    partial[((long)b * NCH + blockIdx.x) * ND + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

__global__ __launch_bounds__(64) void wa_final_kernel(int K, int n, const int* __restrict__ lengths,
                                                      const double* __restrict__ partial, float* __restrict__ value,
                                                      int* __restrict__ perm_out, double* __restrict__ vals, int* __restrict__ pj) {
  using namespace wa;
  __shared__ double tab[ND];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int len = row_len(lengths, b, n), per = chunk_len(len), nch = (len + per - 1) / per;
  if (tid < ND) {
    double s = 0.0;
    if (tid / CMAX < K && tid % CMAX < K)
      for (int c = 0; c < nch; ++c) s += partial[((long)b * NCH + c) * ND + tid];      // chunk order: fixed
    tab[tid] = s;
  }
  __syncthreads();
  if (tid == 0) {          // permutations in lexicographic order, the first minimum wins
    int perm[CMAX], bperm[CMAX], best_idx = 0, idx = 0;
    for (int q = 0; q < CMAX; ++q) perm[q] = bperm[q] = q;
    double best = 0.0;
    for (;;) {
      double v = 0.0;
      for (int q = 0; q < K; ++q) v += tab[q * CMAX + perm[q]];
      if (idx == 0 || v < best) {
        best = v; best_idx = idx;
        for (int q = 0; q < K; ++q) bperm[q] = perm[q];
      }
      ++idx;
      int p = K - 2;                                   // next lexicographic permutation
      while (p >= 0 && perm[p] > perm[p + 1]) --p;
      if (p < 0) break;
      int c = K - 1;
      while (perm[c] < perm[p]) --c;
      int t = perm[p]; perm[p] = perm[c]; perm[c] = t;
      for (int l = p + 1, r = K - 1; l < r; ++l, --r) { t = perm[l]; perm[l] = perm[r]; perm[r] = t; }
    }
    best /= (double)K * (double)len;
    value[b] = (float)best;
    vals[b] = best;
    if (perm_out) perm_out[b] = best_idx;
    for (int q = 0; q < CMAX; ++q) pj[b * CMAX + q] = q < K ? bperm[q] : 0;
  }
}

__global__ __launch_bounds__(64) void wa_total_kernel(const double* __restrict__ vals, int B, float* __restrict__ total) {
  double s = 0.0;
  for (int b = threadIdx.x; b < B; b += 64) s += vals[b];
  s = tas::wave_sum_d(s);
  if (threadIdx.x == 0) total[0] = (float)(s / (double)B);
}

// d_est (B, C, n) contiguous, written once: the chosen assignment's sign inside the row's length, zero beyond it.
template <bool VIN, bool VOUT>
__global__ __launch_bounds__(256) void wa_backward_kernel(const float* __restrict__ est, const float* __restrict__ ref, long r_sb,
                                                          long r_sc, int B, int K, int n, const int* __restrict__ lengths,
                                                          const float* __restrict__ g_value, const float* __restrict__ g_total,
                                                          const int* __restrict__ pj, float* __restrict__ d_est) {
  using namespace wa;
  const int b = blockIdx.y, i = blockIdx.z;
  const long t = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (t >= n) return;
  const int len = row_len(lengths, b, n), j = pj[b * CMAX + i];
  const double w = (g_value ? (double)g_value[b] : 0.0) + (g_total ? (double)g_total[0] / (double)B : 0.0);
  const float pos = (float)(w / ((double)K * (double)len)), neg = (float)(-w / ((double)K * (double)len));
  const float* x = est + ((long)b * K + i) * n;
  const float* s = ref + (long)b * r_sb + (long)j * r_sc;
  float* out = d_est + ((long)b * K + i) * n;
  const int nv = len - t >= 4 ? 4 : len - t > 0 ? (int)(len - t) : 0;       // samples inside the row's length
  float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (nv > 0) {
    float xv[4], sv[4];
    sisnr_load4<VIN>(x, (int)t, nv, xv);
    sisnr_load4<VIN>(s, (int)t, nv, sv);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < nv) o[e] = xv[e] > sv[e] ? pos : xv[e] < sv[e] ? neg : 0.0f;     // (a NaN difference has no sign: 0)
  }
  if (VOUT) {
    *reinterpret_cast<float4*>(out + t) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (t + e < n) out[t + e] = o[e];
  }
}

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" size_t onssen_wa_pit_workspace_bytes(int B, int C);

namespace wa {
struct Plan {
  bool vec;             // every row of every signal starts on a 16-byte boundary
  double *partial, *vals;
  int* pj;
};
// everything both entries refuse, before anything is launched or written
static int plan(const float* est, const float* ref, int64_t r_sb, int64_t r_sc, int B, int C, int n, void* ws, size_t ws_bytes, Plan* p) {
  if (C < 1 || C > CMAX || B < 1 || B > 65535 || n < 1 || n > 0x7ffff000 || !est || !ref || !ws) return ONSSEN_E_ARG;
  if ((C > 1 && (r_sc < n && r_sc > -n)) || (B > 1 && (r_sb < n && r_sb > -n))) return ONSSEN_E_ARG;     // overlapping rows
  if (ws_bytes < onssen_wa_pit_workspace_bytes(B, C)) return ONSSEN_E_WORKSPACE;
  if ((reinterpret_cast<uintptr_t>(ws) & 7u) != 0) return ONSSEN_E_ALIGN;
  p->vec = aligned16(est) && aligned16(ref) && n % 4 == 0 && r_sb % 4 == 0 && r_sc % 4 == 0;
  p->partial = (double*)ws;
  p->vals = p->partial + (size_t)B * NCH * ND;
  p->pj = (int*)(p->vals + B);
  return ONSSEN_OK;
}
}  // namespace wa

extern "C" {

size_t onssen_wa_pit_workspace_bytes(int B, int C) {
  using namespace wa;
  if (B < 1 || B > 65535 || C < 1 || C > CMAX) return 0;
  return ((size_t)B * NCH * ND + (size_t)B) * sizeof(double) + (size_t)B * CMAX * sizeof(int32_t);
}

int onssen_wa_pit_f32(const float* est, const float* ref, int64_t r_sb, int64_t r_sc, int B, int C, int n, const int32_t* lengths,
                      float* value, int32_t* perm, float* total, void* ws, size_t ws_bytes, void* stream) {
  using namespace wa;
  Plan p;
  if (!value) return ONSSEN_E_ARG;
  const int rc = plan(est, ref, r_sb, r_sc, B, C, n, ws, ws_bytes, &p);
  if (rc != ONSSEN_OK) return rc;
  ONSSEN_CLEAR_ERROR();
  hipStream_t st = (hipStream_t)stream;
  // chunks of the longest possible row; a shorter row has no more of them (chunk_len)
  const int nch = n >= NCH * CHMIN ? NCH : ceil_div(n, CHMIN);
  const dim3 grid((unsigned)nch, (unsigned)B);
#define ONSSEN_WA_PARTIAL(K_)                                                                                              \
  do {                                                                                                                     \
    if (p.vec) hipLaunchKernelGGL((wa_partial_kernel<K_, true>), grid, dim3(256), 0, st, est, ref, (long)r_sb, (long)r_sc, n, \
                                  (const int*)lengths, p.partial);                                                         \
    else hipLaunchKernelGGL((wa_partial_kernel<K_, false>), grid, dim3(256), 0, st, est, ref, (long)r_sb, (long)r_sc, n,   \
                            (const int*)lengths, p.partial);                                                               \
  } while (0)
  switch (C) {
    case 1: ONSSEN_WA_PARTIAL(1); break;
    case 2: ONSSEN_WA_PARTIAL(2); break;
    case 3: ONSSEN_WA_PARTIAL(3); break;
    default: ONSSEN_WA_PARTIAL(4); break;
  }
#undef ONSSEN_WA_PARTIAL
  hipLaunchKernelGGL(wa_final_kernel, dim3((unsigned)B), dim3(64), 0, st, C, n, (const int*)lengths, (const double*)p.partial, value,
                     (int*)perm, p.vals, p.pj);
  if (total) hipLaunchKernelGGL(wa_total_kernel, dim3(1), dim3(64), 0, st, (const double*)p.vals, B, total);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_wa_pit_backward_f32(const float* est, const float* ref, int64_t r_sb, int64_t r_sc, int B, int C, int n,
                               const int32_t* lengths, const float* g_value, const float* g_total, float* d_est, const void* ws,
                               size_t ws_bytes, void* stream) {
  using namespace wa;
  Plan p;
  if (!d_est || (!g_value && !g_total)) return ONSSEN_E_ARG;
  const int rc = plan(est, ref, r_sb, r_sc, B, C, n, const_cast<void*>(ws), ws_bytes, &p);
  if (rc != ONSSEN_OK) return rc;
  ONSSEN_CLEAR_ERROR();
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)ceil_div(n, 1024), (unsigned)B, (unsigned)C);
  const bool vout = aligned16(d_est) && n % 4 == 0;
#define ONSSEN_WA_BWD(VIN, VOUT)                                                                                             \
  hipLaunchKernelGGL((wa_backward_kernel<VIN, VOUT>), grid, dim3(256), 0, st, est, ref, (long)r_sb, (long)r_sc, B, C, n,    \
                     (const int*)lengths, g_value, g_total, (const int*)p.pj, d_est)
  if (p.vec && vout) ONSSEN_WA_BWD(true, true);
  else if (p.vec) ONSSEN_WA_BWD(true, false);
  else if (vout) ONSSEN_WA_BWD(false, true);
  else ONSSEN_WA_BWD(false, false);
#undef ONSSEN_WA_BWD
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

}  // extern "C"
