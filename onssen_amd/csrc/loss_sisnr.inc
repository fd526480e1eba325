// SI-SNR permutation-invariant training loss of Conv-TasNet and its gradient (part of onssen_hip.hip).
// =================================================================================================
// onssen/loss/loss_e2e.py:45-87 (restated in onssen_amd/loss.py: sisnr, si_snr_loss).  For estimates x_i and references s_j,
// each (N, S), i, j < k <= 4, eps = 1e-8, per row over its first len samples:
//   x~ = x - mean(x), s~ = s - mean(s), D = <x~, s~>, E = |s~|^2 + eps, a = D / E, t = a s~, n = |x~ - t|
//   v(i, j) = 20 log10(eps + |t| / (n + eps)),  V = max over permutations p (lexicographic, first maximum) of (1/k) sum_i v(i, p(i))
//   loss = -sum_b V_b / N
// Everything v needs is a handful of moments of the 2k signals: their sums, squared norms and the k^2 products est . ref.
//   sisnr_partial_kernel  grid (chunks, rows): a workgroup reads its chunk of all 2k signals ONCE and writes fp64 partial moments
//   sisnr_final_kernel    one workgroup per row: partials merged in chunk order, the k x k table, the permutation scan, V_b, and
//                         per (row, estimate) the three coefficients of the gradient -- all fp64
//   pit_total_kernel      the scalar loss, a fixed-order sum over the rows (pit.inc)
//   sisnr_backward_kernel d_est[i][b][t] = A x_i[b,t] + B s_p(i)[b,t] + C, evaluated in fp64 and rounded once
// The cancellation note of batch_sdr.inc applies: n^2 = |x~|^2 - (D^2 / E)(1 + eps / E) from a Gram matrix
// cancels, so sums, table and coefficients are fp64 and there is no fp32 log10f.  The moments are taken of x - x[0] and
// s - s[0] (the row's first sample as pivot; centred moments do not depend on it): a constant signal has exactly zero moments
// whatever its value, and a DC offset costs no digits.
// Bit-repeatable and independent of the batch: a row's chunking depends on its own length only, a thread's samples on
// nothing else, every sum has a fixed order (no atomics); aligned rows are fetched 16 bytes at a time, others 4, in the same order.
//
// Gradient of v with respect to x (DESIGN section 16).  With T = |t| = |a| sqrt(S2), S2 = |s~|^2, n as above, u = eps + T / (n + eps):
//   dT/dx = sign(a) sqrt(S2) / E * s~                          (sign(0) = 0; a zero norm has subgradient zero, as ATen's)
//   dn/dx = (x~ - a (1 + eps / E) s~) / n                      (<x~ - a s~, s~> = a eps; 0 where n = 0)
//   dv/dx = K (cT s~ - cN (x~ - a (1 + eps / E) s~)),  K = 20 / (ln 10 * u),  cT = sign(a) sqrt(S2) / (E (n + eps)),
//                                                        cN = T / ((n + eps)^2 n)
// which lies in span{x, s, 1}:  A = -K cN,  B = K (cT + cN a (1 + eps / E)),  C = -(A mean(x) + B mean(s)).
// =================================================================================================
namespace sisnr {
using pit::CMAX;
using pit::NCH;
using pit::row_len;
constexpr int CHMIN = 512;                      // samples of a chunk at least (pit::chunk_len)
constexpr int NM = 4 * CMAX + CMAX * CMAX;      // moments per (row, chunk): sums (est | ref), squared norms (est | ref), products
constexpr int NCOEF = 4;                        // A, B, C per (row, estimate), one spare
constexpr double EPS = 1e-8;
struct Sig {                                    // the 2k signals: row b of estimate i starts at est[i] + b * es[i]
  const float* est[CMAX];
  const float* ref[CMAX];
  long es[CMAX], rs[CMAX];
};
// p[i] without indexing the kernel-argument block with a run-time value
template <class T>
__device__ __forceinline__ T pick(const T (&p)[CMAX], int i) {
  T r = p[0];
#pragma unroll
  for (int q = 1; q < CMAX; ++q)
    if (i == q) r = p[q];
  return r;
}
__device__ __forceinline__ bool slot_used(int slot, int K) {
  if (slot < 4 * CMAX) return (slot % CMAX) < K;
  const int o = slot - 4 * CMAX;
  return o / CMAX < K && o % CMAX < K;
}
}  // namespace sisnr

template <int K, bool VEC>
__global__ __launch_bounds__(256) void sisnr_partial_kernel(sisnr::Sig sg, int S, const int* __restrict__ lengths,
                                                            double* __restrict__ partial) {
  using namespace sisnr;
  __shared__ double red[4][NM];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int len = row_len(lengths, b, S), per = pit::chunk_len(len, CHMIN), c0 = (int)blockIdx.x * per;
  if (c0 >= len) return;                           // (the whole workgroup) this row has fewer chunks than the longest
  const int c1 = c0 + per < len ? c0 + per : len;
  const float* xp[K];
  const float* sp[K];
  double px[K], ps[K];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    xp[i] = sg.est[i] + (long)b * sg.es[i];
    sp[i] = sg.ref[i] + (long)b * sg.rs[i];
    px[i] = (double)xp[i][0];
    ps[i] = (double)sp[i][0];
  }
  double sx[K], ss[K], qx[K], qs[K], xs[K][K];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    sx[i] = ss[i] = qx[i] = qs[i] = 0.0;
#pragma unroll
    for (int j = 0; j < K; ++j) xs[i][j] = 0.0;
  }
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
        double xd[K], sd[K];
#pragma unroll
        for (int i = 0; i < K; ++i) {
          xd[i] = (double)xv[i][e] - px[i];
          sd[i] = (double)sv[i][e] - ps[i];
          sx[i] += xd[i]; ss[i] += sd[i];
          qx[i] += xd[i] * xd[i]; qs[i] += sd[i] * sd[i];
        }
#pragma unroll
        for (int i = 0; i < K; ++i)
#pragma unroll
          for (int j = 0; j < K; ++j) xs[i][j] += xd[i] * sd[j];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < K; ++i) {
    pit::wave_put(red, i, sx[i]); pit::wave_put(red, CMAX + i, ss[i]);                         // sums
    pit::wave_put(red, 2 * CMAX + i, qx[i]); pit::wave_put(red, 3 * CMAX + i, qs[i]);         // squared norms
#pragma unroll
    for (int j = 0; j < K; ++j) pit::wave_put(red, 4 * CMAX + i * CMAX + j, xs[i][j]);
  }
  __syncthreads();
  if (tid < NM && slot_used(tid, K)) partial[((long)b * NCH + blockIdx.x) * NM + tid] = pit::block_sum(red, tid);
}

// One workgroup per row: the moments, the k x k table with the gradient's coefficients, the permutation scan.
__global__ __launch_bounds__(64) void sisnr_final_kernel(sisnr::Sig sg, int K, int S, const int* __restrict__ lengths,
                                                         const double* __restrict__ partial, float* __restrict__ value,
                                                         int* __restrict__ perm_out, double* __restrict__ vals,
                                                         double* __restrict__ coef, int* __restrict__ pj) {
  using namespace sisnr;
  __shared__ double m[NM];
  __shared__ double tab[CMAX][CMAX], cA[CMAX][CMAX], cB[CMAX][CMAX], cC[CMAX][CMAX];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int len = row_len(lengths, b, S), per = pit::chunk_len(len, CHMIN), nch = (len + per - 1) / per;
  if (tid < NM) {
    double s = 0.0;
    if (slot_used(tid, K))
      for (int c = 0; c < nch; ++c) s += partial[((long)b * NCH + c) * NM + tid];      // chunk order: fixed
    m[tid] = s;
  }
  __syncthreads();
  if (tid < K * K) {
    const int i = tid / K, j = tid % K;
    const double n = (double)len;
    const double px = (double)pick(sg.est, i)[(long)b * pick(sg.es, i)], ps = (double)pick(sg.ref, j)[(long)b * pick(sg.rs, j)];
    const double mx = m[i] / n, ms = m[CMAX + j] / n;                  // means of the shifted signals
    double X2 = m[2 * CMAX + i] - mx * m[i], S2 = m[3 * CMAX + j] - ms * m[CMAX + j];
    const double D = m[4 * CMAX + i * CMAX + j] - mx * m[CMAX + j];
    X2 = X2 > 0.0 ? X2 : 0.0;
    S2 = S2 > 0.0 ? S2 : 0.0;
    const double E = S2 + EPS, a = D / E, f = 1.0 + EPS / E;
    double n2 = X2 - (D * a) * f;                                      // |x~ - a s~|^2 >= 0 up to rounding
    n2 = n2 > 0.0 ? n2 : 0.0;
    const double nn = sqrt(n2), rS = sqrt(S2), T = fabs(a) * rS;
    const double u = EPS + T / (nn + EPS);
    tab[i][j] = 20.0 * log10(u);
    const double Kd = (20.0 / 2.302585092994045684) / u;
    const double sgn = a > 0.0 ? 1.0 : a < 0.0 ? -1.0 : 0.0;
    const double cT = sgn * rS / (E * (nn + EPS));
    const double cN = nn > 0.0 ? T / ((nn + EPS) * (nn + EPS) * nn) : 0.0;
    const double A = -Kd * cN, B = Kd * (cT + cN * a * f);
    cA[i][j] = A;
    cB[i][j] = B;
    cC[i][j] = -(A * (px + mx) + B * (ps + ms));
  }
  __syncthreads();
  if (tid == 0) {          // the first maximum of the MEAN wins: sums that round to one quotient tie
    pit::Perms e(K), win = e;
    double best = 0.0;
    do {
      double v = 0.0;
      for (int q = 0; q < K; ++q) v += tab[q][e.p(q)];
      v /= (double)K;
      if (e.idx == 0 || v > best) { best = v; win = e; }
    } while (e.next());
    value[b] = (float)best;
    vals[b] = best;
    if (perm_out) perm_out[b] = win.idx;
    for (int q = 0; q < K; ++q) {
      const int j = win.p(q);
      double* dst = coef + ((long)b * CMAX + q) * NCOEF;
      dst[0] = cA[q][j] / (double)K; dst[1] = cB[q][j] / (double)K; dst[2] = cC[q][j] / (double)K; dst[3] = 0.0;
      pj[b * CMAX + q] = j;
    }
  }
}

// d_est (k, N, S) contiguous, written once: the chosen assignment's A x + B s + C inside the row's length, zero beyond it.
// The incoming gradients are device data: w_b = g_value[b] - g_total / N.
template <bool VIN, bool VOUT>
__global__ __launch_bounds__(256) void sisnr_backward_kernel(sisnr::Sig sg, int N, int S, const int* __restrict__ lengths,
                                                             const float* __restrict__ g_value, const float* __restrict__ g_total,
                                                             const double* __restrict__ coef, const int* __restrict__ pj,
                                                             float* __restrict__ d_est) {
  using namespace sisnr;
  const int b = blockIdx.y, i = blockIdx.z;
  const long t = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (t >= S) return;
  const int len = row_len(lengths, b, S), j = pj[b * CMAX + i];
  const double w = pit::row_weight(g_value, g_total, b, N, -1.0);
  const double* cf = coef + ((long)b * CMAX + i) * NCOEF;
  const double A = w * cf[0], B = w * cf[1], C = w * cf[2];
  const float* x = pick(sg.est, i) + (long)b * pick(sg.es, i);
  const float* s = pick(sg.ref, j) + (long)b * pick(sg.rs, j);
  float* out = d_est + ((long)i * N + b) * S;
  const int nv = pit::inside4(len, t);
  float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (nv > 0) {
    float xv[4], sv[4];
    pit::load4(x, (int)t, nv, VIN, xv);
    pit::load4(s, (int)t, nv, VIN, sv);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < nv) o[e] = (float)(A * (double)xv[e] + B * (double)sv[e] + C);
  }
  pit::store4(out, t, S, VOUT, o);
}

// =================================================================================================
// C ABI
// =================================================================================================
namespace sisnr {
struct Plan {
  Sig sg;
  bool vec;             // every row of every signal starts on a 16-byte boundary
  pit::Ws w;            // extra: the coefficients
};
// everything both entries refuse, before anything is launched or written
static int plan(const float* const* est_host, const int64_t* est_stride_host, const float* const* ref_host,
                const int64_t* ref_stride_host, int k, int N, int S, void* ws, size_t ws_bytes, Plan* p) {
  if (k < 1 || k > CMAX || N < 1 || N > 65535 || S < 1 || S > 0x7ffff000 || !est_host || !est_stride_host || !ref_host ||
      !ref_stride_host || !ws)
    return ONSSEN_E_ARG;
  p->vec = true;
  for (int i = 0; i < CMAX; ++i) {
    const int q = i < k ? i : 0;
    if (!est_host[q] || !ref_host[q] || est_stride_host[q] < S || ref_stride_host[q] < S) return ONSSEN_E_ARG;
    p->sg.est[i] = est_host[q]; p->sg.ref[i] = ref_host[q];
    p->sg.es[i] = (long)est_stride_host[q]; p->sg.rs[i] = (long)ref_stride_host[q];
    p->vec = p->vec && aligned16(est_host[q]) && aligned16(ref_host[q]) &&
             (N == 1 || (est_stride_host[q] % 4 == 0 && ref_stride_host[q] % 4 == 0));
  }
  return pit::carve(ws, ws_bytes, N, NM, CMAX * NCOEF, &p->w);
}
}  // namespace sisnr

extern "C" {

size_t onssen_sisnr_pit_workspace_bytes(int N, int k) {
  using namespace sisnr;
  if (N < 1 || N > 65535 || k < 1 || k > CMAX) return 0;
  return pit::ws_bytes(N, NM, CMAX * NCOEF);
}

int onssen_sisnr_pit_f32(const float* const* est_host, const int64_t* est_stride_host, const float* const* ref_host,
                         const int64_t* ref_stride_host, int k, int N, int S, const int32_t* lengths, float* value,
                         int32_t* perm, float* total, void* ws, size_t ws_bytes, void* stream) {
  using namespace sisnr;
  Plan p;
  if (!value) return ONSSEN_E_ARG;
  const int rc = plan(est_host, est_stride_host, ref_host, ref_stride_host, k, N, S, ws, ws_bytes, &p);
  if (rc != ONSSEN_OK) return rc;
  ONSSEN_CLEAR_ERROR();
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)pit::chunks(S, CHMIN), (unsigned)N);
  pit::with_k(k, [&](auto K) { pit::with_flag(p.vec, [&](auto VEC) {
    hipLaunchKernelGGL((sisnr_partial_kernel<decltype(K)::value, decltype(VEC)::value>), grid, dim3(256), 0, st, p.sg, S,
                       (const int*)lengths, p.w.partial);
  }); });
  hipLaunchKernelGGL(sisnr_final_kernel, dim3((unsigned)N), dim3(64), 0, st, p.sg, k, S, (const int*)lengths,
                     (const double*)p.w.partial, value, (int*)perm, p.w.vals, p.w.extra, p.w.pj);
  if (total) hipLaunchKernelGGL(pit_total_kernel, dim3(1), dim3(64), 0, st, (const double*)p.w.vals, N, -1.0, total);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_sisnr_pit_backward_f32(const float* const* est_host, const int64_t* est_stride_host, const float* const* ref_host,
                                  const int64_t* ref_stride_host, int k, int N, int S, const int32_t* lengths,
                                  const float* g_value, const float* g_total, float* d_est, const void* ws, size_t ws_bytes,
                                  void* stream) {
  using namespace sisnr;
  Plan p;
  if (!d_est || (!g_value && !g_total)) return ONSSEN_E_ARG;
  const int rc = plan(est_host, est_stride_host, ref_host, ref_stride_host, k, N, S, const_cast<void*>(ws), ws_bytes, &p);
  if (rc != ONSSEN_OK) return rc;
  ONSSEN_CLEAR_ERROR();
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)ceil_div(S, 1024), (unsigned)N, (unsigned)k);
  pit::with_flags(p.vec, aligned16(d_est) && S % 4 == 0, [&](auto VIN, auto VOUT) {
    hipLaunchKernelGGL((sisnr_backward_kernel<decltype(VIN)::value, decltype(VOUT)::value>), grid, dim3(256), 0, st, p.sg, N, S,
                       (const int*)lengths, g_value, g_total, (const double*)p.w.extra, (const int*)p.w.pj, d_est);
  });
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

}  // extern "C"
