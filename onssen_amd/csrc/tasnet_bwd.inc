// Conv-TasNet training: the forward that keeps what the backward needs, and the backward (gradients of every packed
// parameter; none with respect to the waveform).  Rows and layout as in tasnet.inc: row = b * T + t, channels contiguous.
//
// Training forward = tas::run (tasnet_run.inc), the launch sequence of onssen_tasnet_forward_f32 (its output is bit-identical),
// over a Plan whose activations point into `saved` instead of the workspace: that alone selects tas_prelu_stats_kernel<true>,
// tas_residual_out_kernel and tas_mask_kernel<true>.  This file keeps the `saved` layout, the backward and its workspace.
// Saved once: the encoder output w [M][N], e = LayerN_S(w) [M][N], the gen_masks logits
// [M][spk N] and the masked encoder output d [M][spk N]; per block: its input x_j [M][B] (R X + 1 slots: slot j + 1 is the
// block's output), the conv1x1 output before PReLU u_j [M][H], the statistics of norm_1 (gLN: fp64 partial sums per utterance
// and 64-frame chunk; cLN: mean / rstd per row) and the depthwise output y_j [M][H].  PReLU(u) and the normalised signal are
// recomputed from u and the statistics wherever the backward needs them.
//
// Backward, in reverse order of the forward.  Every contraction is exact fp32 (no bf16 product touches a gradient):
//   tas_sum_kernel            d decoder.bias = sum of d_out
//   tas_frames_kernel         the L-sample frames of d_out (and later of x) as rows [M spk][L]
//   tas_mask_bwd_kernel       decoder input gradient, d = w m_s -> d m_s and the first part of d w, through the mask activation
//                             to the gradient of the gen_masks logits [M][spk N]
//   tas_wgrad_kernel          every weight gradient dW [I][J] = A^T X over all rows: 64 x 64 tiles, per-row-chunk partials
//   tas_colsum_kernel         every bias gradient (column sums over all rows), per-row-chunk partials
//   tas_merge_kernel /        partials -> the flat gradient buffer, summed in fp64 in a fixed order
//   tas_merge_wave_kernel
//   tas_transpose_pad_kernel  W^T (padded to a multiple of 4 columns): the input gradients are onssen_linear_f32 on it
//   tas_dw_bwd_kernel         depthwise convolution: input gradient (taps mirrored, the forward's zero padding), per-chunk
//                             partials of d norm_1.weight / bias, d dwconv.weight / bias, and the gLN sums (fp64)
//   tas_norm_prelu_bwd_kernel gLN / cLN input gradient fused with PReLU's (input gradient and d alpha partials)
//   tas_residual_kernel       dE = dy + d x_in
//   tas_ln_bwd_kernel         LayerN_S input gradient + the first part of d w; rows of d e * xhat for d LayerN_S.weight
// No atomics: per-workgroup partials, merged in a fixed order -- two runs give the same bits.  No spinning, no allocation.

namespace tas {

constexpr int BW_ROWS = 16;             // frames per workgroup of the depthwise / norm backward kernels (64: a quarter of the workgroups, 9.3 ms per recipe step in tas_dw_bwd_kernel)
constexpr int WG_TILE = 64, WG_KSTEP = 16, WG_MAX_CHUNKS = 64, CS_MAX_CHUNKS = 256;

static inline size_t max2(size_t a, size_t b) { return a > b ? a : b; }
static inline int wg_chunks(long Mr) { const long c = (Mr + 511) / 512; return (int)(c < 1 ? 1 : c > WG_MAX_CHUNKS ? WG_MAX_CHUNKS : c); }
static inline int cs_chunks(long Mr) { const long c = (Mr + 63) / 64; return (int)(c < 1 ? 1 : c > CS_MAX_CHUNKS ? CS_MAX_CHUNKS : c); }

// Byte offsets inside `saved` (each region 256-aligned)
struct Saved {
  size_t w, e, logits, d, x0, x_slot, blk0, blk_stride, u, y, st, total;
};

static Saved saved_layout(const Cfg& g, int n, int S) {
  Saved o;
  const Frames f = frames(g, n, S);
  const size_t M = (size_t)f.M;
  const size_t nch = (size_t)ceil_div(f.T, ROWS_PER_CHUNK);
  const size_t st_bytes = max2((size_t)n * nch * 2 * sizeof(double), M * 2 * sizeof(float));
  size_t p = 0;
  o.w = p; p += al(M * g.N * 4);
  o.e = p; p += al(M * g.N * 4);
  o.logits = p; p += al(M * g.spk * g.N * 4);
  o.d = p; p += al(M * g.spk * g.N * 4);
  o.x0 = p; o.x_slot = al(M * g.B * 4); p += o.x_slot * (size_t)(g.R * g.X + 1);
  o.blk0 = p;
  o.u = 0; o.y = al(M * g.H * 4); o.st = 2 * o.y;
  o.blk_stride = o.st + al(st_bytes);
  p += o.blk_stride * (size_t)(g.R * g.X);
  o.total = p;
  return o;
}

// Byte offsets inside the backward workspace
struct Bws {
  size_t gx, gt, gh, gz, gl, gn1, gn2, gn3, fr, wt, zero, part, gst, total;
  size_t part_floats;
};

static Bws bws_layout(const Cfg& g, int n, int S) {
  Bws o;
  const Frames f = frames(g, n, S);
  const size_t M = (size_t)f.M;
  const size_t sN = (size_t)g.spk * g.N;
  const size_t nchb = (size_t)ceil_div(f.T, BW_ROWS);
  size_t p = 0;
  o.gx = p; p += al(M * g.B * 4);
  o.gt = p; p += al(M * g.B * 4);
  o.gh = p; p += al(M * g.H * 4);
  o.gz = p; p += al(M * g.H * 4);
  o.gl = p; p += al(M * sN * 4);
  o.gn1 = p; p += al(M * g.N * 4);
  o.gn2 = p; p += al(M * g.N * 4);
  o.gn3 = p; p += al(M * g.N * 4);
  o.fr = p; p += al(M * g.spk * g.L * 4);
  const size_t wt = max2(max2((size_t)g.B * ld4(g.H), (size_t)g.H * ld4(g.B)), max2((size_t)g.B * ld4((int)sN), (size_t)g.N * ld4(g.B)));
  o.wt = p; p += al(wt * 4);
  const size_t zf = max2(max2((size_t)g.N, (size_t)g.B), (size_t)g.H);
  o.zero = p; p += al(zf * 4);
  const size_t ij = max2(max2((size_t)g.B * g.H, sN * g.B), max2((size_t)g.B * g.N, (size_t)g.N * g.L));
  size_t pf = (size_t)WG_MAX_CHUNKS * ij;
  pf = max2(pf, (size_t)CS_MAX_CHUNKS * max2(max2(sN, (size_t)g.H), max2((size_t)g.B, (size_t)g.N)));
  pf = max2(pf, (size_t)n * nchb * g.H * (3 + g.P));
  pf = max2(pf, (size_t)n * nchb);
  o.part_floats = pf;
  o.part = p; p += al(pf * 4);
  o.gst = p; p += al((size_t)n * nchb * 2 * sizeof(double));
  o.total = p;
  return o;
}

__global__ __launch_bounds__(256) void tas_residual_out_kernel(float* __restrict__ xo, const float* __restrict__ xi,
                                                               const float* __restrict__ y, long n) {
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) xo[e] = xi[e] + y[e];
}

// ---- reductions over partials -----------------------------------------------------------------------------------------------
// out[e] = sum over c < C of part[c * n + e], in fp64, c ascending.  One thread per element.
__global__ __launch_bounds__(256) void tas_merge_kernel(const float* __restrict__ part, int C, long n, float* __restrict__ out) {
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
    double s = 0.0;
    for (int c = 0; c < C; ++c) s += (double)part[(long)c * n + e];
    out[e] = (float)s;
  }
}
// The same with one wave per element (many partials, few elements): lane l sums c = l, l + 64, ..., then the lanes are summed.
__global__ __launch_bounds__(256) void tas_merge_wave_kernel(const float* __restrict__ part, int C, long n, float* __restrict__ out) {
  const int ln = threadIdx.x & 63;
  for (long e = (long)blockIdx.x * 4 + (threadIdx.x >> 6); e < n; e += (long)gridDim.x * 4) {
    double s = 0.0;
    for (int c = ln; c < C; c += 64) s += (double)part[(long)c * n + e];
    s = wave_sum_d(s);
    if (ln == 0) out[e] = (float)s;
  }
}

// part[chunk] = sum of src over the chunk's elements (grid = chunks); wave sums, then the four waves in order
__global__ __launch_bounds__(256) void tas_sum_kernel(const float* __restrict__ src, long total, float* __restrict__ part) {
  __shared__ double red[4];
  const long per = (total + gridDim.x - 1) / gridDim.x;
  const long e0 = (long)blockIdx.x * per, e1 = e0 + per < total ? e0 + per : total;
  double s = 0.0;
  for (long e = e0 + threadIdx.x; e < e1; e += blockDim.x) s += (double)src[e];
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (float)(((red[0] + red[1]) + red[2]) + red[3]);
}

// part[chunk * I + i] = sum over the chunk's rows of A[r][i]; grid (ceil(I / 256), chunks)
__global__ __launch_bounds__(256) void tas_colsum_kernel(const float* __restrict__ A, long lda, int I, long Mr, long rows_per_chunk,
                                                         float* __restrict__ part) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= I) return;
  const long r0 = (long)blockIdx.y * rows_per_chunk, r1 = r0 + rows_per_chunk < Mr ? r0 + rows_per_chunk : Mr;
  float s = 0.0f;
  for (long r = r0; r < r1; ++r) s += A[r * lda + i];
  part[(long)blockIdx.y * I + i] = s;
}

// ---- weight gradient: part[chunk][I][J] = sum over the chunk's rows of A[r][i] X[r][j] ----------------------------------------
// grid (ceil(I / 64), ceil(J / 64), chunks); 256 threads, each a 4 x 4 block of the 64 x 64 tile; 16 rows per LDS stage.
__global__ __launch_bounds__(256) void tas_wgrad_kernel(const float* __restrict__ A, long lda, int I, const float* __restrict__ X,
                                                        long ldx, int J, long Mr, long rows_per_chunk, int vecA, int vecX,
                                                        float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float As[WG_KSTEP][WG_TILE], Xs[WG_KSTEP][WG_TILE];
  const int i0 = blockIdx.x * WG_TILE, j0 = blockIdx.y * WG_TILE;
  const long r0 = (long)blockIdx.z * rows_per_chunk, r1 = r0 + rows_per_chunk < Mr ? r0 + rows_per_chunk : Mr;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int lr = threadIdx.x >> 4, lc = (threadIdx.x & 15) * 4;       // this thread's 4 floats of a stage
  float acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.0f;
  for (long r = r0; r < r1; r += WG_KSTEP) {
    const long rr = r + lr;
    float4 va = make_float4(0.0f, 0.0f, 0.0f, 0.0f), vx = va;
    if (rr < r1) {
      const float* pa = A + rr * lda + i0 + lc;
      if (vecA && i0 + lc + 3 < I) {
        va = *reinterpret_cast<const float4*>(pa);
      } else {
        if (i0 + lc < I) va.x = pa[0];
        if (i0 + lc + 1 < I) va.y = pa[1];
        if (i0 + lc + 2 < I) va.z = pa[2];
        if (i0 + lc + 3 < I) va.w = pa[3];
      }
      const float* px = X + rr * ldx + j0 + lc;
      if (vecX && j0 + lc + 3 < J) {
        vx = *reinterpret_cast<const float4*>(px);
      } else {
        if (j0 + lc < J) vx.x = px[0];
        if (j0 + lc + 1 < J) vx.y = px[1];
        if (j0 + lc + 2 < J) vx.z = px[2];
        if (j0 + lc + 3 < J) vx.w = px[3];
      }
    }
    __syncthreads();                                   // the previous stage has been read
    *reinterpret_cast<float4*>(&As[lr][lc]) = va;
    *reinterpret_cast<float4*>(&Xs[lr][lc]) = vx;
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < WG_KSTEP; ++kk) {
      const float4 a = *reinterpret_cast<const float4*>(&As[kk][ty * 4]);
      const float4 x = *reinterpret_cast<const float4*>(&Xs[kk][tx * 4]);
      const float av[4] = {a.x, a.y, a.z, a.w}, xv[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[p][q] += av[p] * xv[q];
    }
  }
  float* o = part + (long)blockIdx.z * I * J;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int i = i0 + ty * 4 + p;
    if (i >= I) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = j0 + tx * 4 + q;
      if (j < J) o[(long)i * J + j] = acc[p][q];
    }
  }
}

// dst [K][ld] = transpose of src [I][lds] (K columns used), zeros in columns [I, ld)
__global__ __launch_bounds__(256) void tas_transpose_pad_kernel(const float* __restrict__ src, int I, int K, int lds, int ld,
                                                                float* __restrict__ dst) {
  const long total = (long)K * ld;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int k = (int)(e / ld), i = (int)(e % ld);
    dst[e] = i < I ? src[(long)i * lds + k] : 0.0f;
  }
}

// fr[(row * spk + s) * L + l] = src[s * s_stride + b * b_stride + t * hop + l]
__global__ __launch_bounds__(256) void tas_frames_kernel(const float* __restrict__ src, long s_stride, long b_stride, int T, long M,
                                                         int spk, int L, float* __restrict__ fr) {
  const long total = M * spk * L;
  const int hop = L / 2;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int l = (int)(e % L);
    const long rs = e / L;
    const int s = (int)(rs % spk);
    const long row = rs / spk, b = row / T;
    const int t = (int)(row % T);
    fr[e] = src[(long)s * s_stride + b * b_stride + (long)t * hop + l];
  }
}

// ---- decoder input gradient + mask backward ------------------------------------------------------------------------------------
// One thread per (row, channel k): d_d[s] = sum_l G[row][s][l] dec_w[k][l]; d = w m_s gives d m_s = d_d[s] w and
// d w += sum_s d_d[s] m_s; the activation's derivative gives the gradient of the logits.
__global__ __launch_bounds__(256) void tas_mask_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ w,
                                                           const float* __restrict__ fr, const float* __restrict__ dec_w, long M,
                                                           int N, int L, int spk, int act, float* __restrict__ dlogit,
                                                           float* __restrict__ dw1) {
  const long total = M * N;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const long row = e / N;
    const int k = (int)(e % N);
    const float* q = logits + row * (long)spk * N + k;
    float* o = dlogit + row * (long)spk * N + k;
    const float wv = w[e];
    float dd[MAX_SPK], m[MAX_SPK];
    float mx = -3.0e38f;
#pragma unroll
    for (int s = 0; s < MAX_SPK; ++s) {
      dd[s] = 0.0f;
      m[s] = 0.0f;
      if (s < spk) {
        const float* g = fr + (row * spk + s) * L;
        float a = 0.0f;
        for (int l = 0; l < L; ++l) a += g[l] * dec_w[k * L + l];
        dd[s] = a;
        m[s] = q[(long)s * N];
        mx = fmaxf(mx, m[s]);
      }
    }
    float dwv = 0.0f;
    if (act == ONSSEN_TASNET_SOFTMAX) {
      float sum = 0.0f;
#pragma unroll
      for (int s = 0; s < MAX_SPK; ++s)
        if (s < spk) { m[s] = expf(m[s] - mx); sum += m[s]; }
      float dot = 0.0f;
#pragma unroll
      for (int s = 0; s < MAX_SPK; ++s)
        if (s < spk) { m[s] = m[s] / sum; dwv += dd[s] * m[s]; dot += dd[s] * wv * m[s]; }
#pragma unroll
      for (int s = 0; s < MAX_SPK; ++s)
        if (s < spk) o[(long)s * N] = m[s] * (dd[s] * wv - dot);
    } else {
#pragma unroll
      for (int s = 0; s < MAX_SPK; ++s)
        if (s < spk) {
          const float v = m[s];
          float ms, der;
          if (act == ONSSEN_TASNET_RELU) { ms = fmaxf(v, 0.0f); der = v > 0.0f ? 1.0f : 0.0f; }
          else { ms = 1.0f / (1.0f + expf(-v)); der = ms * (1.0f - ms); }
          dwv += dd[s] * ms;
          o[(long)s * N] = dd[s] * wv * der;
        }
    }
    dw1[e] = dwv;
  }
}

// ---- depthwise convolution backward ------------------------------------------------------------------------------------------
// grid (chunks of BW_ROWS frames, utterances); threads over channels.  dy = gradient of the depthwise output [M][H].
//   dz[tau][k] = sum_p dw[k][p] dy[tau - dil p + pad_l][k]  (frames outside [0, T) contribute nothing)      -> dz
//   cpart[chunk][0 .. H)          = sum_tau dz xhat        (d norm_1.weight)
//   cpart[chunk][H .. 2H)         = sum_tau dz             (d norm_1.bias)
//   cpart[chunk][2H + k P + p]    = sum_t dy[t][k] z[t + dil p - pad_l][k]    (d dwconv.weight), z = xhat gamma + beta
//   cpart[chunk][2H + H P + k]    = sum_t dy[t][k]         (d dwconv.bias)
//   gLN: gpart[(b nchb + chunk) 2 + {0, 1}] = fp64 sums of dz gamma and dz gamma xhat over the chunk
__global__ __launch_bounds__(256) void tas_dw_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ u, int T, int H, int P,
                                                         int dil, int pad_l, int norm, const double* __restrict__ part, int nch,
                                                         const float* __restrict__ rstat, const float* __restrict__ alpha,
                                                         const float* __restrict__ na, const float* __restrict__ nb,
                                                         const float* __restrict__ dw, float* __restrict__ dz,
                                                         float* __restrict__ cpart, double* __restrict__ gpart) {
  __shared__ float gstat[2];
  __shared__ double red[4][2];
  const int b = blockIdx.y, nchb = gridDim.x;
  if (threadIdx.x == 0) {
    float mean = 0.0f, rstd = 1.0f;
    if (norm == ONSSEN_TASNET_GLN) gln_stats(part + (long)b * nch * 2, nch, T, H, &mean, &rstd);
    gstat[0] = mean;
    gstat[1] = rstd;
  }
  __syncthreads();
  const float gmean = gstat[0], grstd = gstat[1], a = alpha[0];
  const int t0 = blockIdx.x * BW_ROWS, t1 = t0 + BW_ROWS < T ? t0 + BW_ROWS : T;
  const long base = (long)b * T;
  float* cp = cpart + ((long)b * nchb + blockIdx.x) * (long)H * (3 + P);
  double s1 = 0.0, s2 = 0.0;
  for (int k = threadIdx.x; k < H; k += blockDim.x) {
    const float ga = na[k], gb = nb[k];
    float sdz = 0.0f, sdzx = 0.0f, sdy = 0.0f;
    for (int t = t0; t < t1; ++t) {
      float g = 0.0f;
      for (int p = 0; p < P; ++p) {
        const int ts = t - dil * p + pad_l;
        if (ts >= 0 && ts < T) g += dw[k * P + p] * dy[(base + ts) * H + k];
      }
      dz[(base + t) * H + k] = g;
      float v = u[(base + t) * H + k];
      v = v >= 0.0f ? v : a * v;
      const float xh = norm == ONSSEN_TASNET_GLN ? (v - gmean) * grstd : (v - rstat[(base + t) * 2]) * rstat[(base + t) * 2 + 1];
      sdz += g;
      sdzx += g * xh;
      s1 += (double)(g * ga);
      s2 += (double)(g * ga) * (double)xh;
      sdy += dy[(base + t) * H + k];
    }
    cp[k] = sdzx;
    cp[H + k] = sdz;
    cp[2 * H + H * P + k] = sdy;
    for (int p = 0; p < P; ++p) {
      float acc = 0.0f;
      for (int t = t0; t < t1; ++t) {
        const int tau = t + dil * p - pad_l;
        if (tau < 0 || tau >= T) continue;
        float v = u[(base + tau) * H + k];
        v = v >= 0.0f ? v : a * v;
        const float xh = norm == ONSSEN_TASNET_GLN ? (v - gmean) * grstd
                                                   : (v - rstat[(base + tau) * 2]) * rstat[(base + tau) * 2 + 1];
        acc += dy[(base + t) * H + k] * (xh * ga + gb);
      }
      cp[2 * H + k * P + p] = acc;
    }
  }
  if (norm == ONSSEN_TASNET_GLN) {
    s1 = wave_sum_d(s1);
    s2 = wave_sum_d(s2);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = s1; red[threadIdx.x >> 6][1] = s2; }
    __syncthreads();
    if (threadIdx.x == 0) {
      gpart[((long)b * nchb + blockIdx.x) * 2] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
      gpart[((long)b * nchb + blockIdx.x) * 2 + 1] = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
    }
  }
}

// ---- norm_1 input gradient fused with PReLU_1's --------------------------------------------------------------------------------
// grid (chunks of BW_ROWS frames, utterances); each wave takes every 4th frame of the chunk.  In place over dz:
//   d v = rstd (dz gamma - c1 - xhat c2),  c1 = mean(dz gamma), c2 = mean(dz gamma xhat) over the utterance (gLN: from gpart,
//   merged in a fixed order) or over the row (cLN: summed here);  d u = d v (u >= 0 ? 1 : alpha);
//   apart[b nchb + chunk] = sum of d v min(u, 0) over the chunk (d alpha partial; fp64 inside the workgroup).
__global__ __launch_bounds__(256) void tas_norm_prelu_bwd_kernel(float* __restrict__ dz, const float* __restrict__ u, int T, int H,
                                                                 int norm, const double* __restrict__ part, int nch,
                                                                 const float* __restrict__ rstat, const double* __restrict__ gpart,
                                                                 const float* __restrict__ alpha, const float* __restrict__ na,
                                                                 float* __restrict__ apart) {
  __shared__ float gstat[4];
  __shared__ double red[4];
  const int ln = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int b = blockIdx.y, nchb = gridDim.x;
  if (threadIdx.x == 0) {
    float mean = 0.0f, rstd = 1.0f, c1 = 0.0f, c2 = 0.0f;
    if (norm == ONSSEN_TASNET_GLN) {
      gln_stats(part + (long)b * nch * 2, nch, T, H, &mean, &rstd);
      double s1 = 0.0, s2 = 0.0;
      for (int i = 0; i < nchb; ++i) { s1 += gpart[((long)b * nchb + i) * 2]; s2 += gpart[((long)b * nchb + i) * 2 + 1]; }
      c1 = (float)(s1 / ((double)T * H));
      c2 = (float)(s2 / ((double)T * H));
    }
    gstat[0] = mean; gstat[1] = rstd; gstat[2] = c1; gstat[3] = c2;
  }
  __syncthreads();
  const float a = alpha[0];
  const int t0 = blockIdx.x * BW_ROWS, t1 = t0 + BW_ROWS < T ? t0 + BW_ROWS : T;
  double da = 0.0;
  for (int t = t0 + wv; t < t1; t += 4) {
    const long row = (long)b * T + t;
    float* r = dz + row * H;
    const float* ur = u + row * H;
    float mean = gstat[0], rstd = gstat[1], c1 = gstat[2], c2 = gstat[3];
    if (norm == ONSSEN_TASNET_CLN) {
      mean = rstat[row * 2];
      rstd = rstat[row * 2 + 1];
      float s1 = 0.0f, s2 = 0.0f;
      for (int k = ln; k < H; k += 64) {
        float v = ur[k];
        v = v >= 0.0f ? v : a * v;
        const float gx = r[k] * na[k];
        s1 += gx;
        s2 += gx * ((v - mean) * rstd);
      }
      c1 = wave_sum(s1) / (float)H;
      c2 = wave_sum(s2) / (float)H;
    }
    for (int k = ln; k < H; k += 64) {
      const float uv = ur[k];
      const float v = uv >= 0.0f ? uv : a * uv;
      const float xh = (v - mean) * rstd;
      const float dv = rstd * (r[k] * na[k] - c1 - xh * c2);
      r[k] = uv >= 0.0f ? dv : a * dv;
      if (uv < 0.0f) da += (double)(dv * uv);
    }
  }
  da = wave_sum_d(da);
  if (ln == 0) red[wv] = da;
  __syncthreads();
  if (threadIdx.x == 0) apart[(long)b * nchb + blockIdx.x] = (float)(((red[0] + red[1]) + red[2]) + red[3]);
}

// ---- LayerN_S backward ---------------------------------------------------------------------------------------------------------
// One wave per row (as tas_encoder_kernel).  de = gradient of e = LayerN_S(w).  dwt (in: the masks' part of d w) becomes the whole
// d w; prod = de xhat (its column sums are d LayerN_S.weight; those of de are d LayerN_S.bias).
__global__ __launch_bounds__(256) void tas_ln_bwd_kernel(const float* __restrict__ w, const float* __restrict__ de, long M, int N,
                                                         const float* __restrict__ g, float* __restrict__ dwt,
                                                         float* __restrict__ prod) {
  const int ln = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;                               // no barrier in this kernel
  float v[MAX_N / 64];
  float s = 0.0f;
#pragma unroll
  for (int i = 0; i < MAX_N / 64; ++i) {
    const int c = ln + 64 * i;
    v[i] = c < N ? w[row * N + c] : 0.0f;
    s += v[i];
  }
  const float mean = wave_sum(s) / (float)N;
  float q = 0.0f;
#pragma unroll
  for (int i = 0; i < MAX_N / 64; ++i)
    if (ln + 64 * i < N) q += (v[i] - mean) * (v[i] - mean);
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)N + EPS);
  float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
  for (int i = 0; i < MAX_N / 64; ++i) {
    const int c = ln + 64 * i;
    if (c < N) {
      const float gx = de[row * N + c] * g[c];
      s1 += gx;
      s2 += gx * ((v[i] - mean) * rstd);
    }
  }
  const float c1 = wave_sum(s1) / (float)N, c2 = wave_sum(s2) / (float)N;
#pragma unroll
  for (int i = 0; i < MAX_N / 64; ++i) {
    const int c = ln + 64 * i;
    if (c < N) {
      const float xh = (v[i] - mean) * rstd, d = de[row * N + c];
      dwt[row * N + c] += rstd * (d * g[c] - c1 - xh * c2);
      prod[row * N + c] = d * xh;
    }
  }
}

// ---- host helpers ------------------------------------------------------------------------------------------------------------
struct BwdCtx {
  const Bws* w;
  char* wb;
  hipStream_t st;
  float* part() const { return reinterpret_cast<float*>(wb + w->part); }
};

static void merge(const BwdCtx& c, int C, long n, float* out) {
  if (C >= 64)
    hipLaunchKernelGGL(tas_merge_wave_kernel, dim3((unsigned)((n + 3) / 4 > 16384 ? 16384 : (n + 3) / 4)), dim3(256), 0, c.st, c.part(), C,
                       n, out);
  else
    hipLaunchKernelGGL(tas_merge_kernel, dim3(ew_grid(n)), dim3(256), 0, c.st, c.part(), C, n, out);
}

// dW [I][J] = A^T X over Mr rows
static void wgrad(const BwdCtx& c, const float* A, long lda, int I, const float* X, long ldx, int J, long Mr, float* dW) {
  const int ch = wg_chunks(Mr);
  long rpc = (Mr + ch - 1) / ch;
  rpc = (rpc + WG_KSTEP - 1) / WG_KSTEP * WG_KSTEP;
  const int vecA = aligned16(A) && (lda % 4) == 0, vecX = aligned16(X) && (ldx % 4) == 0;
  hipLaunchKernelGGL(tas_wgrad_kernel, dim3((unsigned)ceil_div(I, WG_TILE), (unsigned)ceil_div(J, WG_TILE), (unsigned)ch), dim3(256), 0,
                     c.st, A, lda, I, X, ldx, J, Mr, rpc, vecA, vecX, c.part());
  merge(c, ch, (long)I * J, dW);
}

// db [I] = column sums of A over Mr rows
static void colsum(const BwdCtx& c, const float* A, long lda, int I, long Mr, float* db) {
  const int ch = cs_chunks(Mr);
  const long rpc = (Mr + ch - 1) / ch;
  hipLaunchKernelGGL(tas_colsum_kernel, dim3((unsigned)ceil_div(I, 256), (unsigned)ch), dim3(256), 0, c.st, A, lda, I, Mr, rpc, c.part());
  merge(c, ch, I, db);
}

// dX [M][K] = dY [M][I] W, W [I][K] row-major with leading dimension ldw (the image's padded fp32 copy)
static int dgrad(const BwdCtx& c, const float* dY, long M, int I, const float* W, int K, int ldw, float* dX, void* stream) {
  float* wt = reinterpret_cast<float*>(c.wb + c.w->wt);
  const int ld = ld4(I);
  hipLaunchKernelGGL(tas_transpose_pad_kernel, dim3(ew_grid((long)K * ld)), dim3(256), 0, c.st, W, I, K, ldw, ld, wt);
  return onssen_linear_f32(dY, I, 0, 1, (int)M, I, wt, ld, reinterpret_cast<const float*>(c.wb + c.w->zero), K, ONSSEN_EPI_BIAS, 0, 0.0f,
                           nullptr, dX, K, 0, stream);
}

static bool train_cfg(const int32_t* c, Cfg* g) { return read_cfg(c, g) && g->norm != ONSSEN_TASNET_BN; }

}  // namespace tas

// =================================================================================================
// C ABI of Conv-TasNet training (include/onssen_hip.h)
// =================================================================================================
extern "C" {

size_t onssen_tasnet_saved_bytes(const int32_t* cfg_host, int n, int S) {
  tas::Cfg g;
  if (!tas::train_cfg(cfg_host, &g) || n <= 0 || S < g.L) return 0;
  return tas::saved_layout(g, n, S).total;
}

size_t onssen_tasnet_backward_workspace_bytes(const int32_t* cfg_host, int n, int S) {
  tas::Cfg g;
  if (!tas::train_cfg(cfg_host, &g) || n <= 0 || S < g.L) return 0;
  return tas::bws_layout(g, n, S).total;
}

int onssen_tasnet_train_forward_f32(const int32_t* cfg_host, const void* image, const float* x, int n, int S, int64_t x_stride,
                                    float* out, void* saved, size_t saved_bytes, void* ws, size_t ws_bytes, void* stream) {
  tas::Cfg g;
  if (!tas::train_cfg(cfg_host, &g) || !image || !x || !out || !saved || !ws || n <= 0 || S < g.L || x_stride < S) return ONSSEN_E_ARG;
  const tas::Ws w = tas::ws_layout(g, n, S);
  const tas::Saved sv = tas::saved_layout(g, n, S);
  if (ws_bytes < w.total || saved_bytes < sv.total) return ONSSEN_E_WORKSPACE;
  if (!aligned256(image) || !aligned256(ws) || !aligned256(saved)) return ONSSEN_E_ALIGN;
  const tas::Frames f = tas::frames(g, n, S);
  if (!f.ok) return ONSSEN_E_ARG;
  // c, t and the GEMM image stay in the workspace; everything the backward reads goes to `saved`
  tas::Plan p = tas::in_place(tas::RECT, n, f.T, f.M, x, (long)x_stride, out, ws, w);
  char* sb = static_cast<char*>(saved);
  auto fs = [&](size_t off) { return reinterpret_cast<float*>(sb + off); };
  p.S_out = f.S_out;
  p.w = fs(sv.w); p.e = fs(sv.e); p.logits = fs(sv.logits); p.d = fs(sv.d);
  p.xs = sb + sv.x0; p.x_step = sv.x_slot;
  p.u = sb + sv.blk0 + sv.u; p.y = sb + sv.blk0 + sv.y; p.st = sb + sv.blk0 + sv.st; p.blk_step = sv.blk_stride;
  return tas::run(g, image, p, stream);
}

int onssen_tasnet_backward_f32(const int32_t* cfg_host, const void* image, const float* x, int n, int S, int64_t x_stride,
                               const void* saved, size_t saved_bytes, const float* d_out, float* d_params, void* ws, size_t ws_bytes,
                               void* stream) {
  tas::Cfg g;
  if (!tas::train_cfg(cfg_host, &g) || !image || !x || !saved || !d_out || !d_params || !ws || n <= 0 || S < g.L || x_stride < S)
    return ONSSEN_E_ARG;
  const tas::Layout o = tas::layout(g);
  const tas::Flat fl = tas::flat_layout(g);              // the gradient buffer has the order of onssen_tasnet_pack_f32's params
  const tas::Saved sv = tas::saved_layout(g, n, S);
  const tas::Bws w = tas::bws_layout(g, n, S);
  if (ws_bytes < w.total || saved_bytes < sv.total) return ONSSEN_E_WORKSPACE;
  if (!aligned256(image) || !aligned256(ws) || !aligned256(saved)) return ONSSEN_E_ALIGN;
  const tas::Frames f = tas::frames(g, n, S);
  const int T = f.T, S_out = f.S_out;
  const long M = f.M;
  if (!f.ok || M * g.spk > 0x7fffffffL / 4) return ONSSEN_E_ARG;
  ONSSEN_CLEAR_ERROR();
  hipStream_t st = (hipStream_t)stream;
  const char* im = static_cast<const char*>(image);
  const char* sb = static_cast<const char*>(saved);
  char* wb = static_cast<char*>(ws);
  auto fi = [&](size_t off) { return reinterpret_cast<const float*>(im + off); };
  auto fs = [&](size_t off) { return reinterpret_cast<const float*>(sb + off); };
  auto fw = [&](size_t off) { return reinterpret_cast<float*>(wb + off); };
  const tas::BwdCtx c{&w, wb, st};
  const int N = g.N, L = g.L, B = g.B, H = g.H, P = g.P, sN = g.spk * g.N, RX = g.R * g.X;
  const int ldN = tas::ld4(N), ldB = tas::ld4(B), ldH = tas::ld4(H);
  float *gx = fw(w.gx), *gt = fw(w.gt), *gh = fw(w.gh), *gz = fw(w.gz), *gl = fw(w.gl), *gn1 = fw(w.gn1), *gn2 = fw(w.gn2),
        *gn3 = fw(w.gn3), *fr = fw(w.fr);
  double* gst = reinterpret_cast<double*>(wb + w.gst);
  hipError_t he = hipMemsetAsync(wb + w.zero, 0, (size_t)(N > B ? (N > H ? N : H) : (B > H ? B : H)) * 4, st);
  if (he != hipSuccess) return (int)he;
  // 1. decoder and masks
  const long n_out = (long)g.spk * n * S_out;
  const int sch = (int)(n_out / 4096 < 1 ? 1 : n_out / 4096 > 256 ? 256 : n_out / 4096);
  hipLaunchKernelGGL(tas::tas_sum_kernel, dim3((unsigned)sch), dim3(256), 0, st, d_out, n_out, c.part());
  tas::merge(c, sch, 1, d_params + fl.dec_b);
  hipLaunchKernelGGL(tas::tas_frames_kernel, dim3(tas::ew_grid(M * g.spk * L)), dim3(256), 0, st, d_out, (long)n * S_out, (long)S_out, T,
                     M, g.spk, L, fr);
  hipLaunchKernelGGL(tas::tas_mask_bwd_kernel, dim3(tas::ew_grid(M * N)), dim3(256), 0, st, fs(sv.logits), fs(sv.w), fr, fi(o.dec_w), M,
                     N, L, g.spk, g.act, gl, gn1);
  tas::wgrad(c, fs(sv.d), N, N, fr, L, L, M * g.spk, d_params + fl.dec_w);
  const float* x_last = fs(sv.x0 + (size_t)RX * sv.x_slot);
  tas::wgrad(c, gl, sN, sN, x_last, B, B, M, d_params + fl.mask_w);
  tas::colsum(c, gl, sN, sN, M, d_params + fl.mask_b);
  ONSSEN_LAUNCH_CHECK();
  int rc = tas::dgrad(c, gl, M, sN, fi(o.mask_w), B, ldB, gx, stream);
  if (rc) return rc;
  // 2. the blocks, last to first
  const int nch = ceil_div(T, tas::ROWS_PER_CHUNK), nchb = ceil_div(T, tas::BW_ROWS);
  for (int j = RX - 1; j >= 0; --j) {
    const size_t k = o.blk0 + (size_t)j * o.blk_stride;
    const size_t sj = sv.blk0 + (size_t)j * sv.blk_stride;
    const float *xi = fs(sv.x0 + (size_t)j * sv.x_slot), *bu = fs(sj + sv.u), *by = fs(sj + sv.y);
    const double* part = reinterpret_cast<const double*>(sb + sj + sv.st);
    const float* rstat = reinterpret_cast<const float*>(sb + sj + sv.st);
    float* dp = d_params + fl.blk0 + fl.blk_stride * j;
    const int dil = 1 << (j % g.X), pad_l = tas::pad_left(g, dil);
    tas::wgrad(c, gx, B, B, by, H, H, M, dp + fl.sc_w);
    tas::colsum(c, gx, B, B, M, dp + fl.sc_b);
    ONSSEN_LAUNCH_CHECK();
    rc = tas::dgrad(c, gx, M, B, fi(k + o.sc_w), H, ldH, gh, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(tas::tas_dw_bwd_kernel, dim3((unsigned)nchb, (unsigned)n), dim3(256), 0, st, gh, bu, T, H, P, dil, pad_l, g.norm,
                       part, nch, rstat, fi(k + o.alpha), fi(k + o.n_a), fi(k + o.n_b), fi(k + o.dw_w), gz, c.part(), gst);
    // ONE merge for four tensors: cpart's order [n_w | n_b | dw_w | dw_b] is Flat's, which keeps them adjacent (training has no
    // bn, so nothing lies between n_b and dw_w): fl.dw_b + H - fl.n_w == H (3 + P)
    tas::merge(c, n * nchb, (long)H * (3 + P), dp + fl.n_w);
    hipLaunchKernelGGL(tas::tas_norm_prelu_bwd_kernel, dim3((unsigned)nchb, (unsigned)n), dim3(256), 0, st, gz, bu, T, H, g.norm, part,
                       nch, rstat, gst, fi(k + o.alpha), fi(k + o.n_a), c.part());
    tas::merge(c, n * nchb, 1, dp + fl.alpha);
    tas::wgrad(c, gz, H, H, xi, B, B, M, dp + fl.c1_w);
    tas::colsum(c, gz, H, H, M, dp + fl.c1_b);
    ONSSEN_LAUNCH_CHECK();
    rc = tas::dgrad(c, gz, M, H, fi(k + o.c1_w), B, ldB, gt, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(tas::tas_residual_kernel, dim3(tas::ew_grid(M * B)), dim3(256), 0, st, gx, gt, M * B);
    ONSSEN_LAUNCH_CHECK();
  }
  // 3. bottleneck, LayerN_S, encoder
  tas::wgrad(c, gx, B, B, fs(sv.e), N, N, M, d_params + fl.bott_w);
  tas::colsum(c, gx, B, B, M, d_params + fl.bott_b);
  ONSSEN_LAUNCH_CHECK();
  rc = tas::dgrad(c, gx, M, B, fi(o.bott_w), N, ldN, gn2, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(tas::tas_ln_bwd_kernel, dim3((unsigned)ceil_div((int)M, 4)), dim3(256), 0, st, fs(sv.w), gn2, M, N, fi(o.ln_g), gn1,
                     gn3);
  tas::colsum(c, gn3, N, N, M, d_params + fl.ln_g);
  tas::colsum(c, gn2, N, N, M, d_params + fl.ln_b);
  hipLaunchKernelGGL(tas::tas_frames_kernel, dim3(tas::ew_grid(M * L)), dim3(256), 0, st, x, 0L, (long)x_stride, T, M, 1, L, fr);
  tas::wgrad(c, gn1, N, N, fr, L, L, M, d_params + fl.enc_w);
  tas::colsum(c, gn1, N, N, M, d_params + fl.enc_b);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

}  // extern "C"
