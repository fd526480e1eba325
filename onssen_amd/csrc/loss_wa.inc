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
//   pit_total_kernel    the batch mean, a fixed-order sum over the rows (pit.inc)
//   wa_backward_kernel  one elementwise pass that reads the assignment the forward left in the workspace
// The structure is loss_sisnr.inc's, the shared parts are pit.inc's: bit-repeatable, independent of the batch, no workspace zeroing.
// est is (B, C, n) contiguous (the inverse transform's output); ref (b, j) starts at ref + b r_sb + j r_sc, unit sample stride.
// =================================================================================================
namespace wa {
using pit::CMAX;
using pit::NCH;
using pit::row_len;
constexpr int CHMIN = 1024;                     // samples of a chunk at least (pit::chunk_len)
constexpr int ND = CMAX * CMAX;                 // sums per (row, chunk)
}  // namespace wa

template <int K, bool VEC>
__global__ __launch_bounds__(256) void wa_partial_kernel(const float* __restrict__ est, const float* __restrict__ ref, long r_sb,
                                                         long r_sc, int n, const int* __restrict__ lengths,
                                                         double* __restrict__ partial) {
  using namespace wa;
  __shared__ double red[4][ND];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int len = row_len(lengths, b, n), per = pit::chunk_len(len, CHMIN), c0 = (int)blockIdx.x * per;
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
      pit::load4(xp[i], t, nv, VEC, xv[i]);
      pit::load4(sp[i], t, nv, VEC, sv[i]);
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
    for (int j = 0; j < K; ++j) pit::wave_put(red, i * CMAX + j, d[i][j]);
  __syncthreads();
  if (tid < ND && tid / CMAX < K && tid % CMAX < K) partial[((long)b * NCH + blockIdx.x) * ND + tid] = pit::block_sum(red, tid);
}

__global__ __launch_bounds__(64) void wa_final_kernel(int K, int n, const int* __restrict__ lengths,
                                                      const double* __restrict__ partial, float* __restrict__ value,
                                                      int* __restrict__ perm_out, double* __restrict__ vals, int* __restrict__ pj) {
  using namespace wa;
  __shared__ double tab[ND];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int len = row_len(lengths, b, n), per = pit::chunk_len(len, CHMIN), nch = (len + per - 1) / per;
  if (tid < ND) {
    double s = 0.0;
    if (tid / CMAX < K && tid % CMAX < K)
      for (int c = 0; c < nch; ++c) s += partial[((long)b * NCH + c) * ND + tid];      // chunk order: fixed
    tab[tid] = s;
  }
  __syncthreads();
  if (tid == 0) {          // the first minimum of the raw sum wins; the division comes after the scan
    pit::Perms e(K), win = e;
    double best = 0.0;
    do {
      double v = 0.0;
      for (int q = 0; q < K; ++q) v += tab[q * CMAX + e.p(q)];
      if (e.idx == 0 || v < best) { best = v; win = e; }
    } while (e.next());
    best /= (double)K * (double)len;
    value[b] = (float)best;
    vals[b] = best;
    if (perm_out) perm_out[b] = win.idx;
    for (int q = 0; q < CMAX; ++q) pj[b * CMAX + q] = q < K ? win.p(q) : 0;
  }
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
  const double w = pit::row_weight(g_value, g_total, b, B, 1.0);
  const float pos = (float)(w / ((double)K * (double)len)), neg = (float)(-w / ((double)K * (double)len));
  const float* x = est + ((long)b * K + i) * n;
  const float* s = ref + (long)b * r_sb + (long)j * r_sc;
  float* out = d_est + ((long)b * K + i) * n;
  const int nv = pit::inside4(len, t);
  float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (nv > 0) {
    float xv[4], sv[4];
    pit::load4(x, (int)t, nv, VIN, xv);
    pit::load4(s, (int)t, nv, VIN, sv);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < nv) o[e] = xv[e] > sv[e] ? pos : xv[e] < sv[e] ? neg : 0.0f;     // (a NaN difference has no sign: 0)
  }
  pit::store4(out, t, n, VOUT, o);
}

// =================================================================================================
// C ABI
// =================================================================================================
namespace wa {
// everything both entries refuse, before anything is launched or written; vec: every row of every signal starts on a 16-byte boundary
static int plan(const float* est, const float* ref, int64_t r_sb, int64_t r_sc, int B, int C, int n, void* ws, size_t ws_bytes,
                bool* vec, pit::Ws* w) {
  if (C < 1 || C > CMAX || B < 1 || B > 65535 || n < 1 || n > 0x7ffff000 || !est || !ref || !ws) return ONSSEN_E_ARG;
  if ((C > 1 && (r_sc < n && r_sc > -n)) || (B > 1 && (r_sb < n && r_sb > -n))) return ONSSEN_E_ARG;     // overlapping rows
  *vec = aligned16(est) && aligned16(ref) && n % 4 == 0 && r_sb % 4 == 0 && r_sc % 4 == 0;
  return pit::carve(ws, ws_bytes, B, ND, 0, w);
}
}  // namespace wa

extern "C" {

size_t onssen_wa_pit_workspace_bytes(int B, int C) {
  using namespace wa;
  if (B < 1 || B > 65535 || C < 1 || C > CMAX) return 0;
  return pit::ws_bytes(B, ND, 0);
}

int onssen_wa_pit_f32(const float* est, const float* ref, int64_t r_sb, int64_t r_sc, int B, int C, int n, const int32_t* lengths,
                      float* value, int32_t* perm, float* total, void* ws, size_t ws_bytes, void* stream) {
  using namespace wa;
  bool vec;
  pit::Ws w;
  if (!value) return ONSSEN_E_ARG;
  const int rc = plan(est, ref, r_sb, r_sc, B, C, n, ws, ws_bytes, &vec, &w);
  if (rc != ONSSEN_OK) return rc;
  ONSSEN_CLEAR_ERROR();
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)pit::chunks(n, CHMIN), (unsigned)B);
  pit::with_k(C, [&](auto K) { pit::with_flag(vec, [&](auto VEC) {
    hipLaunchKernelGGL((wa_partial_kernel<decltype(K)::value, decltype(VEC)::value>), grid, dim3(256), 0, st, est, ref, (long)r_sb,
                       (long)r_sc, n, (const int*)lengths, w.partial);
  }); });
  hipLaunchKernelGGL(wa_final_kernel, dim3((unsigned)B), dim3(64), 0, st, C, n, (const int*)lengths, (const double*)w.partial, value,
                     (int*)perm, w.vals, w.pj);
  if (total) hipLaunchKernelGGL(pit_total_kernel, dim3(1), dim3(64), 0, st, (const double*)w.vals, B, 1.0, total);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_wa_pit_backward_f32(const float* est, const float* ref, int64_t r_sb, int64_t r_sc, int B, int C, int n,
                               const int32_t* lengths, const float* g_value, const float* g_total, float* d_est, const void* ws,
                               size_t ws_bytes, void* stream) {
  using namespace wa;
  bool vec;
  pit::Ws w;
  if (!d_est || (!g_value && !g_total)) return ONSSEN_E_ARG;
  const int rc = plan(est, ref, r_sb, r_sc, B, C, n, const_cast<void*>(ws), ws_bytes, &vec, &w);
  if (rc != ONSSEN_OK) return rc;
  ONSSEN_CLEAR_ERROR();
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)ceil_div(n, 1024), (unsigned)B, (unsigned)C);
  pit::with_flags(vec, aligned16(d_est) && n % 4 == 0, [&](auto VIN, auto VOUT) {
    hipLaunchKernelGGL((wa_backward_kernel<decltype(VIN)::value, decltype(VOUT)::value>), grid, dim3(256), 0, st, est, ref, (long)r_sb,
                       (long)r_sc, B, C, n, (const int*)lengths, g_value, g_total, (const int*)w.pj, d_est);
  });
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

}  // extern "C"
