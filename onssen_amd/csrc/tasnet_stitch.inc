// Conv-TasNet long-form separation: a recording cut into K overlapping windows of W samples, `step` samples apart, each
// separated on its own, and the window estimates put back together on the device (DESIGN.md section 15).
//
// A separation model assigns speakers to output rows per window, so consecutive windows are permutation-aligned on their
// overlap of O = W - step samples before they are cross-faded:
//   tas_windows_kernel        x (S,) -> (K, W) rows x[k step, k step + W), zeros past S (the forward wants rows >= S apart, so
//                             overlapping windows cannot be a strided view of x)
//   tas_stitch_sim_kernel     sim[k][i][j] = sum_t est[i][k-1][step + t] est[j][k][t], t in [0, O): one workgroup per (pair, i, j),
//                             fp64 sums, thread e owns t = e, e + 256, ..., then a tree over the workgroup: a fixed order
//   tas_stitch_perm_kernel    per pair the permutation of maximal summed similarity (lexicographic scan, first maximum wins), then
//                             the serial composition into absolute permutations perm[k][c] = the row of window k that carries
//                             output channel c; one wave, 64 pairs per round through LDS
//   tas_stitch_kernel         out[c][t]: a copy where one window covers t, w_old a + w_new b on an overlap (w_new = (j + 0.5) / O)
// Geometry: O <= W / 2, so at most two windows cover a sample; all windows are full but the last, which holds v_last valid samples,
// O < v_last <= W, so every consecutive pair overlaps in exactly O samples and S_out = (K - 1) step + v_last.
// Permutations of <= 4 sources are carried as packed 2-bit fields (channel c in bits 2c, 2c + 1): no indexed private array, no scratch.
// No atomics, no value read back by the host: ordinary launches on one stream, two runs give the same bits.

namespace tas {

constexpr int STITCH_MAX_SPK = 4;

struct StitchGeo { int C, K, W, step, O, v_last; long S_out; size_t ws_bytes; };

static bool stitch_geo(int C, int K, int W, int step, int v_last, StitchGeo* g) {
  if (C < 1 || C > STITCH_MAX_SPK || K < 1 || W < 2 || step < 1 || step >= W) return false;
  const int O = W - step;
  if (O > W / 2 || v_last <= O || v_last > W) return false;
  if ((long)K * C * C > 0x7fffffffL / 8) return false;                     // sim's index, and K C perm entries, stay int-sized
  *g = StitchGeo{C, K, W, step, O, v_last, (long)(K - 1) * step + v_last, al((size_t)(K > 1 ? K - 1 : 1) * C * C * 8)};
  return true;
}

// ---- gather: window rows out of the signal ------------------------------------------------------------------------------------
// VEC: W, step multiples of 4 and both pointers 16-byte aligned: every float4 of a row is an aligned float4 of x.
template <bool VEC>
__global__ __launch_bounds__(256) void tas_windows_kernel(const float* __restrict__ x, long S, int K, int W, int step,
                                                          float* __restrict__ win) {
  constexpr int V = VEC ? 4 : 1;
  const long per_row = W / V, total = (long)K * per_row;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const long k = e / per_row;
    const int i = (int)(e - k * per_row) * V;
    const long src = k * step + i;
    if (VEC) {
      float4 v;
      if (src + 3 < S) {
        v = *reinterpret_cast<const float4*>(x + src);
      } else {
        v.x = src < S ? x[src] : 0.0f;
        v.y = src + 1 < S ? x[src + 1] : 0.0f;
        v.z = src + 2 < S ? x[src + 2] : 0.0f;
        v.w = 0.0f;
      }
      *reinterpret_cast<float4*>(win + k * W + i) = v;
    } else {
      win[k * W + i] = src < S ? x[src] : 0.0f;
    }
  }
}

// ---- similarity of the rows of two consecutive windows on their overlap -----------------------------------------------------------
// grid (pairs, C * C): blockIdx.x = k - 1, blockIdx.y = i * C + j.
__global__ __launch_bounds__(256) void tas_stitch_sim_kernel(const float* __restrict__ est, int C, int K, int W, int step, int O,
                                                             double* __restrict__ sim) {
  __shared__ double red[256];
  const int k = blockIdx.x + 1, i = blockIdx.y / C, j = blockIdx.y % C;
  const float* a = est + ((long)i * K + (k - 1)) * W + step;
  const float* b = est + ((long)j * K + k) * W;
  double acc = 0.0;
  for (int t = threadIdx.x; t < O; t += 256) acc += (double)a[t] * (double)b[t];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) sim[((long)(k - 1) * C + i) * C + j] = red[0];
}

// ---- best permutation per pair, composed serially ------------------------------------------------------------------------------------
// One workgroup of one wave.  Round r: lane l scans the permutations for pair 64 r + l (windows k - 1, k with k = 64 r + l + 1) in
// lexicographic order -- the codes 0 .. 255 read as four base-4 digits d0 d1 d2 d3, valid when d0 .. d(C-1) are a permutation of
// 0 .. C-1 and the rest sit at their own index -- and keeps the first of maximal sum_i sim[k][i][d_i] (a NaN never wins; nothing
// beats the identity on an all-silent overlap).  Lane 0 then walks the round's choices: perm[k][c] = pi_k(perm[k-1][c]).
__global__ __launch_bounds__(64) void tas_stitch_perm_kernel(const double* __restrict__ sim, int C, int K, int32_t* __restrict__ perm) {
  __shared__ int rel[64];
  const int identity = 0 | 1 << 2 | 2 << 4 | 3 << 6;
  int cur = identity;
  if (threadIdx.x == 0)
    for (int c = 0; c < C; ++c) perm[c] = c;
  for (int base = 1; base < K; base += 64) {
    const int k = base + (int)threadIdx.x;
    int best_p = identity;
    if (k < K) {
      const double* s = sim + (long)(k - 1) * C * C;
      double best = -INFINITY;
      for (int code = 0; code < 256; ++code) {
        const int d0 = code >> 6, d1 = (code >> 4) & 3, d2 = (code >> 2) & 3, d3 = code & 3;
        int seen = 1 << d0;
        bool ok = true;
        if (C > 1) seen |= 1 << d1; else ok = ok && d1 == 1;
        if (C > 2) seen |= 1 << d2; else ok = ok && d2 == 2;
        if (C > 3) seen |= 1 << d3; else ok = ok && d3 == 3;
        if (!ok || seen != (1 << C) - 1) continue;
        double score = s[d0];
        if (C > 1) score += s[C + d1];
        if (C > 2) score += s[2 * C + d2];
        if (C > 3) score += s[3 * C + d3];
        if (score > best) { best = score; best_p = d0 | d1 << 2 | d2 << 4 | d3 << 6; }
      }
    }
    rel[threadIdx.x] = best_p;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int m = K - base < 64 ? K - base : 64;
      for (int l = 0; l < m; ++l) {
        const int p = rel[l];
        int next = 0;
        for (int c = 0; c < STITCH_MAX_SPK; ++c) next |= ((p >> (2 * ((cur >> (2 * c)) & 3))) & 3) << (2 * c);
        cur = next;
        for (int c = 0; c < C; ++c) perm[(long)(base + l) * C + c] = (cur >> (2 * c)) & 3;
      }
    }
    __syncthreads();
  }
}

// ---- stitch: copy / cross-fade through perm -----------------------------------------------------------------------------------------
// Sample t of the output lies in window k = min(t / step, K - 1) at j = t - k step; for k >= 1 and j < O it also lies in window
// k - 1 at step + j.  VEC: W, step, S_out multiples of 4 (so O and every region boundary are) and both pointers 16-byte aligned:
// the four samples of an aligned float4 share k and their side of the boundary.
template <bool VEC>
__global__ __launch_bounds__(256) void tas_stitch_kernel(const float* __restrict__ est, int C, int K, int W, int step, int O,
                                                         long S_out, const int32_t* __restrict__ perm, float* __restrict__ out) {
  constexpr int V = VEC ? 4 : 1;
  const long per_row = S_out / V, total = (long)C * per_row;
  const float fO = (float)O;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int c = (int)(e / per_row);
    const long t = (e - (long)c * per_row) * V;
    long kk = t / step;
    const int k = kk < K - 1 ? (int)kk : K - 1;
    const int j = (int)(t - (long)k * step);
    const float* b = est + ((long)perm[(long)k * C + c] * K + k) * W + j;
    float* o = out + (long)c * S_out + t;
    if (k >= 1 && j < O) {
      const float* a = est + ((long)perm[(long)(k - 1) * C + c] * K + (k - 1)) * W + step + j;
      if (VEC) {
        const float4 va = *reinterpret_cast<const float4*>(a), vb = *reinterpret_cast<const float4*>(b);
        const float w0 = ((float)j + 0.5f) / fO, w1 = ((float)j + 1.5f) / fO, w2 = ((float)j + 2.5f) / fO, w3 = ((float)j + 3.5f) / fO;
        float4 r;
        r.x = (1.0f - w0) * va.x + w0 * vb.x;
        r.y = (1.0f - w1) * va.y + w1 * vb.y;
        r.z = (1.0f - w2) * va.z + w2 * vb.z;
        r.w = (1.0f - w3) * va.w + w3 * vb.w;
        *reinterpret_cast<float4*>(o) = r;
      } else {
        const float w_new = ((float)j + 0.5f) / fO;
        *o = (1.0f - w_new) * a[0] + w_new * b[0];
      }
    } else if (VEC) {
      *reinterpret_cast<float4*>(o) = *reinterpret_cast<const float4*>(b);
    } else {
      *o = b[0];
    }
  }
}

}  // namespace tas

extern "C" {

int onssen_tasnet_windows_f32(const float* x, int64_t S, int K, int W, int step, float* win, void* stream) {
  if (!x || !win || S < 1 || K < 1 || W < 1 || step < 1 || (int64_t)(K - 1) * step >= S) return ONSSEN_E_ARG;
  ONSSEN_CLEAR_ERROR();
  const bool vec = (W % 4) == 0 && (step % 4) == 0 && aligned16(x) && aligned16(win);
  if (vec)
    hipLaunchKernelGGL(tas::tas_windows_kernel<true>, dim3(tas::ew_grid((long)K * (W / 4))), dim3(256), 0, (hipStream_t)stream, x,
                       (long)S, K, W, step, win);
  else
    hipLaunchKernelGGL(tas::tas_windows_kernel<false>, dim3(tas::ew_grid((long)K * W)), dim3(256), 0, (hipStream_t)stream, x, (long)S,
                       K, W, step, win);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

size_t onssen_tasnet_stitch_workspace_bytes(int C, int K, int W, int step, int v_last) {
  tas::StitchGeo g;
  return tas::stitch_geo(C, K, W, step, v_last, &g) ? g.ws_bytes : 0;
}

int onssen_tasnet_stitch_f32(const float* est, int C, int K, int W, int step, int v_last, float* out, int32_t* perm_out, void* ws,
                             size_t ws_bytes, void* stream) {
  tas::StitchGeo g;
  if (!est || !out || !perm_out || !ws || !tas::stitch_geo(C, K, W, step, v_last, &g)) return ONSSEN_E_ARG;
  if (ws_bytes < g.ws_bytes) return ONSSEN_E_WORKSPACE;
  if (!aligned16(ws)) return ONSSEN_E_ALIGN;                                 // fp64 similarities, nothing wider
  ONSSEN_CLEAR_ERROR();
  hipStream_t st = (hipStream_t)stream;
  double* sim = static_cast<double*>(ws);
  if (K > 1)
    hipLaunchKernelGGL(tas::tas_stitch_sim_kernel, dim3((unsigned)(K - 1), (unsigned)(C * C)), dim3(256), 0, st, est, C, K, W, step,
                       g.O, sim);
  hipLaunchKernelGGL(tas::tas_stitch_perm_kernel, dim3(1), dim3(64), 0, st, (const double*)sim, C, K, perm_out);
  const bool vec = (W % 4) == 0 && (step % 4) == 0 && (g.S_out % 4) == 0 && aligned16(est) && aligned16(out);
  if (vec)
    hipLaunchKernelGGL(tas::tas_stitch_kernel<true>, dim3(tas::ew_grid((long)C * (g.S_out / 4))), dim3(256), 0, st, est, C, K, W, step,
                       g.O, g.S_out, (const int32_t*)perm_out, out);
  else
    hipLaunchKernelGGL(tas::tas_stitch_kernel<false>, dim3(tas::ew_grid((long)C * g.S_out)), dim3(256), 0, st, est, C, K, W, step, g.O,
                       g.S_out, (const int32_t*)perm_out, out);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

}  // extern "C"
