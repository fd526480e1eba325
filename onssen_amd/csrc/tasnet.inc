// Conv-TasNet separation forward (onssen/nn/tasnet.py:166-264), eval semantics.
//
// Layout: activations are time-major rows, row = b * T + t (b = utterance, t = encoder frame), the channels of a row
// contiguous -- every 1x1 convolution is then a row GEMM Y = X W^T + b over the existing GEMM family (onssen_linear_f32 for
// exact fp32, an x3 image + onssen_linear_x3p for split-bf16 / bf16).  The kernels here do what lies between the GEMMs:
//   tas_encoder_kernel      Conv1d(1, N, L, stride L/2) + LayerN_S (LayerNorm over the N channels of each frame)
//   tas_prelu_stats_kernel  PReLU_1 in place + the statistics of norm_1: gLN partial sums per (utterance, 64-frame chunk) in
//                           fp64, cLN mean / rstd per row; BatchNorm needs none (running statistics)
//   tas_dwconv_kernel       gLN partials reduced in a fixed order, norm_1 applied on load (a per-channel affine), the dilated
//                           depthwise convolution with zero padding on the NORMALISED signal (causal: left padding only)
//   tas_residual_kernel     x += Sc_conv(...)
//   tas_mask_kernel         mask activation (relu / sigmoid / softmax across speakers) times the encoder output w, in place
//   tas_decoder_kernel      ConvTranspose1d(N, 1, L, stride L/2): per frame a contraction over N, then the overlap-add of the
//                           two frames that cover each output sample, plus the bias; each output sample has exactly one owner
// No atomics, no spinning, no allocation: the whole forward is a fixed sequence of ordinary launches on one stream.
//
// Ragged batches (onssen_tasnet_forward_ragged_f32): COMPACT rows -- utterance b owns rows [row[b], row[b] + T_b), no padded
// rows exist, so the GEMMs, the residual and the mask kernel run unchanged over M = sum T_b rows.  The four kernels that know
// where an utterance ends (encoder, statistics, depthwise convolution, decoder) have a *_ragged_kernel twin over the SAME
// device body: the twin only finds (utterance, first frame) of its workgroup from a table of prefix sums that travels by value
// as a kernel argument (struct Rag; host integers in, no copy, no synchronisation), so one output element is computed by the
// same instructions in the same order as in a one-utterance rectangular run.
// PReLU_2 / norm_2 exist upstream but the block's forward never calls them (tasnet.py:149-163): they are not packed.
//
// ONE launch sequence: tas::run (tasnet_run.inc) alone walks the network.  Each entry validates its arguments and fills a Plan:
// the kind of batch (RECT / RAGGED / STREAM picks the launch of the four boundary-aware steps) and where every activation lives;
// the kernel variants follow from the pointers.  The two entries here work in place in the workspace (in_place()); the ragged
// one adds its Geo tables.

namespace tas {

constexpr int ROWS_PER_CHUNK = 64;      // gLN partial sums: one per (utterance, 64 frames)
constexpr int DW_ROWS = 32;             // depthwise convolution: frames per workgroup
constexpr int DEC_FRAMES = 16;          // decoder: 16 hop-sized output blocks per workgroup
constexpr int MAX_L = 64, MAX_N = 1024, MAX_SPK = 8, MAX_P = 32;
constexpr float EPS = 1e-5f;            // GlobalLayerNorm, LayerNorm and BatchNorm1d defaults of the reference
constexpr int MAX_UTT = ONSSEN_TASNET_RAGGED_MAX;   // utterances of one ragged forward (bounds the by-value table)

// Table of a ragged batch: row[b] = first row of utterance b (prefix sums of T_b), blk[b] = first workgroup of utterance b in
// the launch that receives this copy (prefix sums of that kernel's per-utterance workgroup count).  Both strictly increasing.
struct Rag {
  int n;
  int row[MAX_UTT + 1];
  int blk[MAX_UTT + 1];
};

// largest b with pre[b] <= v (pre[0] = 0 <= v < pre[n])
__device__ __forceinline__ int rag_find(const int* pre, int n, int v) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (pre[mid] <= v) lo = mid; else hi = mid;
  }
  return lo;
}

struct Cfg {
  int N, L, B, H, P, X, R, norm, spk, act, causal, prec, exact;   // exact: ONSSEN_TASNET_EXACT_* kinds kept on exact fp32
};

static bool read_cfg(const int32_t* c, Cfg* g) {
  if (!c) return false;
  *g = Cfg{c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9], c[10], c[11] & 0xff, (c[11] >> 8) & 0xff};
  if (g->N <= 0 || g->N > MAX_N || g->L < 2 || g->L > MAX_L || (g->L % 2) != 0) return false;
  if (g->B <= 0 || g->H <= 0 || g->P <= 0 || g->P > MAX_P || g->X <= 0 || g->R <= 0 || g->X > 30) return false;
  if (!g->causal && (g->P % 2) == 0) return false;                 // non-causal even P changes the frame count upstream
  if (g->norm < ONSSEN_TASNET_GLN || g->norm > ONSSEN_TASNET_BN) return false;
  if (g->spk <= 0 || g->spk > MAX_SPK) return false;
  if (g->act < ONSSEN_TASNET_RELU || g->act > ONSSEN_TASNET_SOFTMAX) return false;
  if (g->prec < ONSSEN_TASNET_F32 || g->prec > ONSSEN_TASNET_BF16 || (c[11] >> 16) != 0 || g->exact > 15) return false;
  return true;
}

static inline size_t al(size_t x) { return align256(x); }
static inline int ld4(int k) { return (k + 3) / 4 * 4; }

// Offsets (bytes) of the weight image: fp32 copies (1x1 weights padded to a multiple of 4 columns, zeros beyond K) followed by
// the x3 images of the four GEMM weight kinds.  The image does not depend on the precision: one image serves all three.
struct Layout {
  size_t enc_w, enc_b, ln_g, ln_b, bott_w, bott_b, mask_w, mask_b, dec_w, dec_b, blk0, blk_stride;
  size_t c1_w, c1_b, alpha, n_a, n_b, dw_w, dw_b, sc_w, sc_b;     // inside a block
  size_t bott_x3, mask_x3, x3_blk0, x3_blk_stride, c1_x3, sc_x3, total;
};

static Layout layout(const Cfg& g) {
  Layout o;
  const int ldN = ld4(g.N), ldB = ld4(g.B), ldH = ld4(g.H);
  size_t p = 0;
  auto take = [&](size_t floats) { const size_t at = p; p += al(floats * 4); return at; };
  o.enc_w = take((size_t)g.N * g.L); o.enc_b = take(g.N); o.ln_g = take(g.N); o.ln_b = take(g.N);
  o.bott_w = take((size_t)g.B * ldN); o.bott_b = take(g.B);
  o.mask_w = take((size_t)g.spk * g.N * ldB); o.mask_b = take((size_t)g.spk * g.N);
  o.dec_w = take((size_t)g.N * g.L); o.dec_b = take(1);
  o.blk0 = p;
  size_t q = 0;
  auto tb = [&](size_t floats) { const size_t at = q; q += al(floats * 4); return at; };
  o.c1_w = tb((size_t)g.H * ldB); o.c1_b = tb(g.H); o.alpha = tb(1); o.n_a = tb(g.H); o.n_b = tb(g.H);
  o.dw_w = tb((size_t)g.H * g.P); o.dw_b = tb(g.H); o.sc_w = tb((size_t)g.B * ldH); o.sc_b = tb(g.B);
  o.blk_stride = q;
  p += q * (size_t)(g.R * g.X);
  const int kbN = ceil_div(g.N, 32), kbB = ceil_div(g.B, 32), kbH = ceil_div(g.H, 32);
  o.bott_x3 = p; p += al((size_t)g.B * kbN * 128);
  o.mask_x3 = p; p += al((size_t)g.spk * g.N * kbB * 128);
  o.x3_blk0 = p;
  o.c1_x3 = 0; o.sc_x3 = al((size_t)g.H * kbB * 128);
  o.x3_blk_stride = o.sc_x3 + al((size_t)g.B * kbH * 128);
  p += o.x3_blk_stride * (size_t)(g.R * g.X);
  o.total = p;
  return o;
}

// Offsets (floats) of the flat parameter buffer that onssen_tasnet_pack_f32 reads and onssen_tasnet_backward_f32 writes -- THE
// order of include/onssen_hip.h: encoder, LayerN_S, bottleneck, the R X blocks, gen_masks, decoder.  norm = bn: a block also
// carries the running mean and variance (n_mu, n_var) behind norm_1's weight and bias; they do not exist otherwise, and then
// n_w, n_b, dw_w, dw_b are adjacent (the backward merges the four in one go).
struct Flat {
  int64_t enc_w, enc_b, ln_g, ln_b, bott_w, bott_b, blk0, blk_stride, mask_w, mask_b, dec_w, dec_b, total;
  int64_t c1_w, c1_b, alpha, n_w, n_b, n_mu, n_var, dw_w, dw_b, sc_w, sc_b;     // inside a block
};

static Flat flat_layout(const Cfg& g) {
  Flat o;
  int64_t p = 0;
  auto take = [&](int64_t floats) { const int64_t at = p; p += floats; return at; };
  o.c1_w = take((int64_t)g.H * g.B); o.c1_b = take(g.H); o.alpha = take(1); o.n_w = take(g.H); o.n_b = take(g.H);
  o.n_mu = o.n_var = p;
  if (g.norm == ONSSEN_TASNET_BN) { o.n_mu = take(g.H); o.n_var = take(g.H); }
  o.dw_w = take((int64_t)g.H * g.P); o.dw_b = take(g.H); o.sc_w = take((int64_t)g.B * g.H); o.sc_b = take(g.B);
  o.blk_stride = p;
  p = 0;
  o.enc_w = take((int64_t)g.N * g.L); o.enc_b = take(g.N); o.ln_g = take(g.N); o.ln_b = take(g.N);
  o.bott_w = take((int64_t)g.B * g.N); o.bott_b = take(g.B);
  o.blk0 = take(o.blk_stride * g.R * g.X);
  o.mask_w = take((int64_t)g.spk * g.N * g.B); o.mask_b = take((int64_t)g.spk * g.N);
  o.dec_w = take((int64_t)g.N * g.L); o.dec_b = take(1);
  o.total = p;
  return o;
}

static int64_t param_floats(const Cfg& g) { return flat_layout(g).total; }

// Workspace (bytes, each region 256-aligned): w [M][N], e / depthwise output [M][max(N, H)], x [M][B], c [M][H],
// t [M][max(B, spk N)], the GEMM A-operand image [M][KBmax][2][32], statistics (max of gLN partials and cLN rows).
struct Ws {
  size_t w, e, x, c, t, img, st, total;
};

// M rows in all, nchunks gLN partial pairs in all (rectangular: n T and n ceil(T / 64))
static Ws ws_layout_rows(const Cfg& g, size_t M, size_t nchunks) {
  Ws o;
  const int kbmax = ceil_div(g.N > g.B ? (g.N > g.H ? g.N : g.H) : (g.B > g.H ? g.B : g.H), 32);
  const int NH = g.N > g.H ? g.N : g.H, BS = g.B > g.spk * g.N ? g.B : g.spk * g.N;
  const size_t st_bytes = nchunks * 2 * sizeof(double) > M * 2 * sizeof(float) ? nchunks * 2 * sizeof(double) : M * 2 * sizeof(float);
  size_t p = 0;
  o.w = p; p += al(M * g.N * 4);
  o.e = p; p += al(M * NH * 4);
  o.x = p; p += al(M * g.B * 4);
  o.c = p; p += al(M * g.H * 4);
  o.t = p; p += al(M * BS * 4);
  o.img = p; p += al(M * kbmax * 128);
  o.st = p; p += al(st_bytes);
  o.total = p;
  return o;
}

// n utterances of S samples: T frames each, S_out samples out, M = n T rows; ok = M within the GEMMs' row bound
struct Frames { int T, S_out; long M; bool ok; };
static Frames frames(const Cfg& g, int n, int S) {
  const int hop = g.L / 2, T = (S - g.L) / hop + 1;
  const long M = (long)n * T;
  return Frames{T, (T - 1) * hop + g.L, M, M <= 0x7fffffffL / 4};
}

// zero frames in front of a block's depthwise convolution of dilation dil
static inline int pad_left(const Cfg& g, int dil) { return g.causal ? dil * (g.P - 1) : dil * (g.P - 1) / 2; }

static Ws ws_layout(const Cfg& g, int n, int S) {
  const Frames f = frames(g, n, S);
  return ws_layout_rows(g, (size_t)f.M, (size_t)n * ceil_div(f.T, ROWS_PER_CHUNK));
}

// ---- packing ----------------------------------------------------------------------------------------------------------------
// rows x K (row-major, contiguous) -> rows x ld (zeros in columns [K, ld))
__global__ __launch_bounds__(256) void tas_copy_pad_kernel(const float* __restrict__ src, long rows, int K, int ld,
                                                           float* __restrict__ dst) {
  const long total = rows * ld;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const long r = e / ld;
    const int k = (int)(e % ld);
    dst[e] = k < K ? src[r * K + k] : 0.0f;
  }
}

// BatchNorm1d (eval) folded to a per-channel affine: a = g / sqrt(var + eps), b = beta - mean a (fp64)
__global__ __launch_bounds__(256) void tas_fold_bn_kernel(const float* __restrict__ g, const float* __restrict__ be,
                                                          const float* __restrict__ mu, const float* __restrict__ var, int H,
                                                          float* __restrict__ a, float* __restrict__ b) {
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < H; c += gridDim.x * blockDim.x) {
    const double s = (double)g[c] / sqrt((double)var[c] + (double)EPS);
    a[c] = (float)s;
    b[c] = (float)((double)be[c] - (double)mu[c] * s);
  }
}

// ---- K1: encoder + LayerN_S -------------------------------------------------------------------------------------------------
// One wave per frame; lane j owns channels j, j + 64, ... (N <= 1024: 16 per lane, register-resident).
__device__ __forceinline__ void tas_encoder_row(const float* __restrict__ fr, long row, int N, int L, const float* __restrict__ ew,
                                                const float* __restrict__ eb, const float* __restrict__ g,
                                                const float* __restrict__ be, float* __restrict__ w_out, float* __restrict__ e_out) {
  const int ln = threadIdx.x & 63;
  float v[MAX_N / 64];
  float s = 0.0f;
#pragma unroll
  for (int i = 0; i < MAX_N / 64; ++i) {
    const int c = ln + 64 * i;
    float acc = 0.0f;
    if (c < N) {
      acc = eb[c];
      for (int l = 0; l < L; ++l) acc += ew[c * L + l] * fr[l];
      w_out[row * N + c] = acc;
      s += acc;
    }
    v[i] = acc;
  }
  const float mean = wave_sum(s) / (float)N;
  float q = 0.0f;
#pragma unroll
  for (int i = 0; i < MAX_N / 64; ++i)
    if (ln + 64 * i < N) q += (v[i] - mean) * (v[i] - mean);
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)N + EPS);
#pragma unroll
  for (int i = 0; i < MAX_N / 64; ++i) {
    const int c = ln + 64 * i;
    if (c < N) e_out[row * N + c] = (v[i] - mean) * rstd * g[c] + be[c];
  }
}

__global__ __launch_bounds__(256) void tas_encoder_kernel(const float* __restrict__ x, long x_s, int T, long M, int N, int L,
                                                          const float* __restrict__ ew, const float* __restrict__ eb,
                                                          const float* __restrict__ g, const float* __restrict__ be,
                                                          float* __restrict__ w_out, float* __restrict__ e_out) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;                               // no barrier in this kernel
  const long b = row / T;
  const int t = (int)(row % T);
  tas_encoder_row(x + b * x_s + (long)t * (L / 2), row, N, L, ew, eb, g, be, w_out, e_out);
}

// Ragged: frame t of utterance b covers samples [t L/2, t L/2 + L) of its row, all below S_out_b <= S_b.
__global__ __launch_bounds__(256) void tas_encoder_ragged_kernel(const float* __restrict__ x, long x_s, Rag rg, int N, int L,
                                                                 const float* __restrict__ ew, const float* __restrict__ eb,
                                                                 const float* __restrict__ g, const float* __restrict__ be,
                                                                 float* __restrict__ w_out, float* __restrict__ e_out) {
  const int row = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (row >= rg.row[rg.n]) return;                    // no barrier in this kernel
  const int b = rag_find(rg.row, rg.n, row);
  const int t = row - rg.row[b];
  tas_encoder_row(x + (long)b * x_s + (long)t * (L / 2), row, N, L, ew, eb, g, be, w_out, e_out);
}

// ---- PReLU_1 + statistics of norm_1 -----------------------------------------------------------------------------------------
// grid (chunks of 64 frames, utterances); each wave takes every 4th frame of the chunk.
//   gLN: fp64 (sum, sum of squares) of the chunk -> part[(b * nch + chunk) * 2 + {0, 1}] (fixed order: lanes, then waves)
//   cLN: per frame (mean, rstd) -> rstat[row * 2 + {0, 1}] (two passes over the row, as LayerNorm)
// SAVE (training forward): the pre-PReLU values are read from `src` and stay there; c receives PReLU(src).
// One chunk: frames [t0, t1) of the utterance whose rows start at `base`; part2 = this chunk's (sum, sum of squares) pair.
template <bool SAVE>
__device__ __forceinline__ void tas_prelu_stats_chunk(float* __restrict__ c, long base, int t0, int t1, int H,
                                                      const float* __restrict__ alpha, int norm, double* __restrict__ part2,
                                                      float* __restrict__ rstat, const float* __restrict__ src) {
  __shared__ double red[4][2];
  const int ln = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float a = alpha[0];
  double s = 0.0, q = 0.0;
  for (int t = t0 + wv; t < t1; t += 4) {
    float* r = c + (base + t) * H;
    float rs = 0.0f;
    for (int k = ln; k < H; k += 64) {
      float v = SAVE ? src[(base + t) * H + k] : r[k];
      v = v >= 0.0f ? v : a * v;
      r[k] = v;
      if (norm == ONSSEN_TASNET_GLN) { s += (double)v; q += (double)v * (double)v; }
      rs += v;
    }
    if (norm == ONSSEN_TASNET_CLN) {
      const float mean = wave_sum(rs) / (float)H;
      float rq = 0.0f;
      for (int k = ln; k < H; k += 64) rq += (r[k] - mean) * (r[k] - mean);
      const float var = wave_sum(rq) / (float)H;
      if (ln == 0) {
        rstat[(base + t) * 2] = mean;
        rstat[(base + t) * 2 + 1] = 1.0f / sqrtf(var + EPS);
      }
    }
  }
  if (norm == ONSSEN_TASNET_GLN) {
    s = wave_sum_d(s);
    q = wave_sum_d(q);
    if (ln == 0) { red[wv][0] = s; red[wv][1] = q; }
  }
  __syncthreads();
  if (norm == ONSSEN_TASNET_GLN && threadIdx.x == 0) {
    part2[0] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
    part2[1] = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
  }
}

template <bool SAVE>
__global__ __launch_bounds__(256) void tas_prelu_stats_kernel(float* __restrict__ c, int T, int H, const float* __restrict__ alpha,
                                                              int norm, double* __restrict__ part, float* __restrict__ rstat,
                                                              const float* __restrict__ src) {
  const int b = blockIdx.y, nch = gridDim.x;
  const int t0 = blockIdx.x * ROWS_PER_CHUNK, t1 = t0 + ROWS_PER_CHUNK < T ? t0 + ROWS_PER_CHUNK : T;
  tas_prelu_stats_chunk<SAVE>(c, (long)b * T, t0, t1, H, alpha, norm, part + ((long)b * nch + blockIdx.x) * 2, rstat, src);
}

// Ragged: grid = all chunks of all utterances; chunks are counted from the utterance's own frame 0, and the partial sums of
// utterance b lie at part[2 blk[b] ...] in chunk order -- the partition and the merge order of the one-utterance run.
__global__ __launch_bounds__(256) void tas_prelu_stats_ragged_kernel(float* __restrict__ c, Rag rg, int H,
                                                                     const float* __restrict__ alpha, int norm,
                                                                     double* __restrict__ part, float* __restrict__ rstat) {
  const int b = rag_find(rg.blk, rg.n, (int)blockIdx.x);
  const int T = rg.row[b + 1] - rg.row[b];
  const int t0 = ((int)blockIdx.x - rg.blk[b]) * ROWS_PER_CHUNK, t1 = t0 + ROWS_PER_CHUNK < T ? t0 + ROWS_PER_CHUNK : T;
  tas_prelu_stats_chunk<false>(c, (long)rg.row[b], t0, t1, H, alpha, norm, part + (long)blockIdx.x * 2, rstat, nullptr);
}

// ---- K2: norm_1 on load + dilated depthwise convolution ----------------------------------------------------------------------
// gLN statistics of one utterance of T frames from its nch partial pairs, merged in chunk order (one thread; the forward's
// depthwise kernel and the two backward kernels that recompute the normalised signal all call this).
__device__ __forceinline__ void gln_stats(const double* __restrict__ part, int nch, int T, int H, float* mean, float* rstd) {
  double s = 0.0, q = 0.0;
  for (int i = 0; i < nch; ++i) { s += part[(long)i * 2]; q += part[(long)i * 2 + 1]; }
  const double cnt = (double)T * H, m = s / cnt;
  double var = q / cnt - m * m;
  var = var > 0.0 ? var : 0.0;
  *mean = (float)m;
  *rstd = (float)(1.0 / sqrt(var + (double)EPS));
}

// norm_1 of one tap: (mean, rstd) of the utterance (gLN) or of the tap's frame (cLN); BatchNorm is the folded affine alone
__device__ __forceinline__ float norm_tap(float v, float mean, float rstd, float ga, float gb, int norm) {
  return norm == ONSSEN_TASNET_BN ? v * ga + gb : (v - mean) * rstd * ga + gb;
}

// grid (chunks of 32 frames, utterances); threads over channels.  Output frame t reads normalised frames t + d p - pad_l,
// zeros outside [0, T).
// One tile: output frames [t0, t0 + DW_ROWS) of the utterance of T frames whose rows start at `base`; part = that utterance's
// nch gLN partial pairs.
__device__ __forceinline__ void tas_dwconv_tile(const float* __restrict__ c, long base, int T, int t0, int H, int P, int dil,
                                                int pad_l, int norm, const double* __restrict__ part, int nch,
                                                const float* __restrict__ rstat, const float* __restrict__ na,
                                                const float* __restrict__ nb, const float* __restrict__ dw,
                                                const float* __restrict__ dwb, float* __restrict__ out) {
  __shared__ float gstat[2];
  if (threadIdx.x == 0) {
    float mean = 0.0f, rstd = 1.0f;
    if (norm == ONSSEN_TASNET_GLN) gln_stats(part, nch, T, H, &mean, &rstd);
    gstat[0] = mean;
    gstat[1] = rstd;
  }
  __syncthreads();
  const float gmean = gstat[0], grstd = gstat[1];
  const int t1 = t0 + DW_ROWS < T ? t0 + DW_ROWS : T;
  for (int k = threadIdx.x; k < H; k += blockDim.x) {
    const float ga = na[k], gb = nb[k], bias = dwb[k];
    for (int t = t0; t < t1; ++t) {
      float acc = bias;
      for (int p = 0; p < P; ++p) {
        const int tau = t + dil * p - pad_l;
        if (tau < 0 || tau >= T) continue;
        const float v = c[(base + tau) * H + k];
        const float nv = norm == ONSSEN_TASNET_GLN   ? norm_tap(v, gmean, grstd, ga, gb, norm)
                         : norm == ONSSEN_TASNET_CLN ? norm_tap(v, rstat[(base + tau) * 2], rstat[(base + tau) * 2 + 1], ga, gb, norm)
                                                     : norm_tap(v, 0.0f, 1.0f, ga, gb, norm);
        acc += dw[k * P + p] * nv;
      }
      out[(base + t) * H + k] = acc;
    }
  }
}

__global__ __launch_bounds__(256) void tas_dwconv_kernel(const float* __restrict__ c, int T, int H, int P, int dil, int pad_l,
                                                         int norm, const double* __restrict__ part, int nch,
                                                         const float* __restrict__ rstat, const float* __restrict__ na,
                                                         const float* __restrict__ nb, const float* __restrict__ dw,
                                                         const float* __restrict__ dwb, float* __restrict__ out) {
  const int b = blockIdx.y;
  tas_dwconv_tile(c, (long)b * T, T, blockIdx.x * DW_ROWS, H, P, dil, pad_l, norm, part + (long)b * nch * 2, nch, rstat, na, nb, dw,
                  dwb, out);
}

// Ragged: grid = all 32-frame tiles of all utterances.  A tap outside [0, T_b) of the OWN utterance is zero padding (it never
// reads a neighbour's rows); cs[b] = first gLN chunk of utterance b (the statistics kernel's blk table).
struct RagChunks { int at[MAX_UTT + 1]; };
__global__ __launch_bounds__(256) void tas_dwconv_ragged_kernel(const float* __restrict__ c, Rag rg, RagChunks cs, int H, int P,
                                                                int dil, int pad_l, int norm, const double* __restrict__ part,
                                                                const float* __restrict__ rstat, const float* __restrict__ na,
                                                                const float* __restrict__ nb, const float* __restrict__ dw,
                                                                const float* __restrict__ dwb, float* __restrict__ out) {
  const int b = rag_find(rg.blk, rg.n, (int)blockIdx.x);
  const int T = rg.row[b + 1] - rg.row[b];
  tas_dwconv_tile(c, (long)rg.row[b], T, ((int)blockIdx.x - rg.blk[b]) * DW_ROWS, H, P, dil, pad_l, norm,
                  part + (long)cs.at[b] * 2, cs.at[b + 1] - cs.at[b], rstat, na, nb, dw, dwb, out);
}

__global__ __launch_bounds__(256) void tas_residual_kernel(float* __restrict__ x, const float* __restrict__ y, long n) {
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) x[e] += y[e];
}

// ---- masks: activation (softmax across speakers) times w, in place over the gen_masks output [M][spk N] ----------------------
// SAVE (training forward): the logits are read from `src` [M][spk N] and stay there; m receives the masked encoder output.
template <bool SAVE>
__global__ __launch_bounds__(256) void tas_mask_kernel(float* __restrict__ m, const float* __restrict__ w, long M, int N, int spk,
                                                       int act, const float* __restrict__ src) {
  const long total = M * N;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const long row = e / N;
    const int k = (int)(e % N);
    float* r = m + row * (long)spk * N + k;
    const float* q = SAVE ? src + row * (long)spk * N + k : r;
    const float wv = w[e];
    if (act == ONSSEN_TASNET_SOFTMAX) {
      float mx = q[0];
      for (int s = 1; s < spk; ++s) mx = fmaxf(mx, q[(long)s * N]);
      float sum = 0.0f;
      for (int s = 0; s < spk; ++s) sum += expf(q[(long)s * N] - mx);
      for (int s = 0; s < spk; ++s) r[(long)s * N] = wv * (expf(q[(long)s * N] - mx) / sum);
    } else {
      for (int s = 0; s < spk; ++s) {
        const float v = q[(long)s * N];
        r[(long)s * N] = wv * (act == ONSSEN_TASNET_RELU ? fmaxf(v, 0.0f) : 1.0f / (1.0f + expf(-v)));
      }
    }
  }
}

// ---- K3: decoder (ConvTranspose1d(N, 1, L, stride L/2)) ----------------------------------------------------------------------
// grid (chunks of 16 hop-sized output blocks, utterances, speakers).  Output block j (samples [j hop, (j + 1) hop)) is covered
// by frames j (first half of its L taps) and j - 1 (second half); there are T + 1 blocks.  The workgroup first contracts the 17
// frames it needs over the N channels into LDS, then every output sample is written by exactly one thread.
// Tap l of one frame: its row r of N masked channels contracted with column l of the decoder weight [N][L], k ascending.
__device__ __forceinline__ float dec_tap(const float* __restrict__ r, const float* __restrict__ dw, int N, int L, int l) {
  float acc = 0.0f;
  for (int k = 0; k < N; ++k) acc += r[k] * dw[k * L + l];
  return acc;
}

// One tile: output blocks [j0, j0 + DEC_FRAMES) of speaker s of the utterance of T frames whose rows start at `base`; o = that
// (speaker, utterance)'s output row of S_out valid samples.
__device__ __forceinline__ void tas_decoder_tile(const float* __restrict__ d, long base, int T, int j0, int s, int N, int L,
                                                 int spk, const float* __restrict__ dw, const float* __restrict__ db,
                                                 float* __restrict__ o, int S_out) {
  __shared__ float Ps[(DEC_FRAMES + 1) * MAX_L];
  const int hop = L / 2;
  const long ldd = (long)spk * N;
  for (int e = threadIdx.x; e < (DEC_FRAMES + 1) * L; e += blockDim.x) {
    const int jj = e / L, l = e % L, f = j0 - 1 + jj;
    float acc = 0.0f;
    if (f >= 0 && f < T) acc = dec_tap(d + (base + f) * ldd + (long)s * N, dw, N, L, l);
    Ps[jj * L + l] = acc;
  }
  __syncthreads();
  const float bias = db[0];
  const int i0 = j0 * hop, i1 = (j0 + DEC_FRAMES) * hop < S_out ? (j0 + DEC_FRAMES) * hop : S_out;
  for (int i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
    const int j = i / hop, off = i - j * hop, jj = j - (j0 - 1);
    float v = bias;
    if (j < T) v += Ps[jj * L + off];                 // frame j, tap off
    if (j >= 1) v += Ps[(jj - 1) * L + off + hop];    // frame j - 1, tap off + hop
    o[i] = v;
  }
}

__global__ __launch_bounds__(256) void tas_decoder_kernel(const float* __restrict__ d, int T, int N, int L, int spk,
                                                          const float* __restrict__ dw, const float* __restrict__ db,
                                                          float* __restrict__ out, int S_out) {
  const int b = blockIdx.y, s = blockIdx.z, n = gridDim.y;
  tas_decoder_tile(d, (long)b * T, T, blockIdx.x * DEC_FRAMES, s, N, L, spk, dw, db, out + ((long)s * n + b) * S_out, S_out);
}

// Ragged: grid (all 16-block tiles of all utterances, speakers); out = spk x n rows of out_stride floats.  The utterance's last
// tile also writes the zeros of [S_out_b, out_stride), so every float of `out` has exactly one writer.
__global__ __launch_bounds__(256) void tas_decoder_ragged_kernel(const float* __restrict__ d, Rag rg, int N, int L, int spk,
                                                                 const float* __restrict__ dw, const float* __restrict__ db,
                                                                 float* __restrict__ out, long out_stride) {
  const int b = rag_find(rg.blk, rg.n, (int)blockIdx.x), s = blockIdx.y;
  const int T = rg.row[b + 1] - rg.row[b], S_out = (T - 1) * (L / 2) + L;
  float* o = out + ((long)s * rg.n + b) * out_stride;
  tas_decoder_tile(d, (long)rg.row[b], T, ((int)blockIdx.x - rg.blk[b]) * DEC_FRAMES, s, N, L, spk, dw, db, o, S_out);
  if ((int)blockIdx.x + 1 == rg.blk[b + 1])
    for (long i = S_out + threadIdx.x; i < out_stride; i += blockDim.x) o[i] = 0.0f;
}

static unsigned ew_grid(long total) { const long nb = (total + 255) / 256; return (unsigned)(nb > 16384 ? 16384 : nb < 1 ? 1 : nb); }

// One 1x1 convolution: C [M][Nout] = A [M][K] W^T + b in the configured precision (image = scratch for A's x3 image).
static int gemm(const Cfg& g, int kind, const float* A, long M, int K, const float* w32, const uint16_t* w3, const float* bias,
                int Nout, float* C, uint16_t* image, void* stream) {
  if (g.prec == ONSSEN_TASNET_F32 || (g.exact & kind))
    return onssen_linear_f32(A, K, 0, 1, (int)M, K, w32, ld4(K), bias, Nout, ONSSEN_EPI_BIAS, 0, 0.0f, nullptr, C, Nout, 0, stream);
  int rc = onssen_x3_image_f32(A, K, 0, 1, (int)M, K, image, stream);
  if (rc) return rc;
  const int mode = ONSSEN_EPI_BIAS | (g.prec == ONSSEN_TASNET_BF16 ? ONSSEN_EPI_BF16 : 0);
  return onssen_linear_x3p(image, (int)M, K, w3, bias, Nout, mode, 0, 0.0f, C, 1, Nout, 0, stream);
}

// The tables of a ragged batch: what the four boundary-aware kernels (encoder, statistics, depthwise convolution, decoder) need
// to find an utterance -- the same row prefix sums, each with its own workgroup prefix sums -- built from the host lengths.
struct Geo {
  int S_out;                       // the longest output: the least out_stride
  long M;                          // rows in all
  long out_stride;                 // floats per (speaker, utterance) row of out
  Rag st, dwc, dec;                // blk = 64-frame chunks / 32-frame tiles / 16-block decoder tiles
  RagChunks cs;
};

// false: a length the ragged forward refuses (n out of range, S_b < L, S_b > x_stride, M over the GEMMs' row bound)
static bool ragged_geo(const Cfg& g, int n, const int32_t* len, int64_t x_stride, Geo* o) {
  if (n <= 0 || n > MAX_UTT || !len) return false;
  o->st.n = o->dwc.n = o->dec.n = n;
  o->S_out = 0;
  o->st.row[0] = o->st.blk[0] = o->dwc.blk[0] = o->dec.blk[0] = 0;
  long M = 0;
  for (int b = 0; b < n; ++b) {
    if (len[b] < g.L || (x_stride >= 0 && len[b] > x_stride)) return false;
    const Frames f = frames(g, 1, len[b]);
    M += f.T;
    if (M > 0x7fffffffL / 4) return false;
    if (f.S_out > o->S_out) o->S_out = f.S_out;
    o->st.row[b + 1] = (int)M;
    o->st.blk[b + 1] = o->st.blk[b] + ceil_div(f.T, ROWS_PER_CHUNK);
    o->dwc.blk[b + 1] = o->dwc.blk[b] + ceil_div(f.T, DW_ROWS);
    o->dec.blk[b + 1] = o->dec.blk[b] + ceil_div(f.T + 1, DEC_FRAMES);
  }
  for (int b = 0; b <= n; ++b) {
    o->dwc.row[b] = o->dec.row[b] = o->st.row[b];
    o->cs.at[b] = o->st.blk[b];
  }
  o->M = M;
  return true;
}

// ---- the plan of one run of the network (tas::run, tasnet_run.inc) -----------------------------------------------------------
// kind: RECT = n utterances of T frames (eval and training); RAGGED = the Geo tables; STREAM = n streams advance by T frames (the
// stage launch goes in front of the encoder, which then reads the staging rows, the history launch behind each depthwise one).
enum Kind { RECT, RAGGED, STREAM };

struct Plan {
  Kind kind;
  int n, T, S_out;                 // S_out: RECT
  long M, x_stride;                // rows in all; x = the waveforms (STREAM: the new samples), rows of x_stride floats
  const float* x;
  float* out;
  const Geo* geo;                  // RAGGED
  long long* cnt;                  // STREAM: frame counters, input carry, decoder carry, staging rows, block 0's history
  float *carry_x, *carry_d, *stage;
  char* hist;
  // Where the activations live.  In place (in_place(): eval, ragged, stream) they are regions of the workspace and u == c,
  // xi == xo, logits == d; the training forward points u, y, st, the block inputs, w, e, logits and d into `saved` instead.
  float *w, *e, *c, *t, *logits, *d;       // c = PReLU(u); t = Sc_conv's output
  uint16_t* img;                           // the GEMMs' A-operand image
  char *xs, *u, *y, *st;                   // block j: xi = xs + j x_step, xo = xs + (j + 1) x_step; u, y, st at + j blk_step
  size_t x_step, blk_step;                 // (y = depthwise output, st = the statistics of norm_1)
};

static Plan in_place(Kind kind, int n, int T, long M, const float* x, long x_stride, float* out, void* ws, const Ws& w) {
  char* wb = static_cast<char*>(ws);
  auto f = [&](size_t off) { return reinterpret_cast<float*>(wb + off); };
  Plan p{};
  p.kind = kind; p.n = n; p.T = T; p.M = M; p.x = x; p.x_stride = x_stride; p.out = out;
  p.w = f(w.w); p.e = f(w.e); p.c = f(w.c); p.t = p.logits = p.d = f(w.t);
  p.img = reinterpret_cast<uint16_t*>(wb + w.img);
  p.xs = wb + w.x; p.u = wb + w.c; p.y = wb + w.e; p.st = wb + w.st;
  return p;
}

static int run(const Cfg& g, const void* image, const Plan& p, void* stream);

}  // namespace tas

// =================================================================================================
// C ABI of the Conv-TasNet forward (include/onssen_hip.h)
// =================================================================================================
extern "C" {

int64_t onssen_tasnet_param_floats(const int32_t* cfg_host) {
  tas::Cfg g;
  return tas::read_cfg(cfg_host, &g) ? tas::param_floats(g) : (int64_t)ONSSEN_E_ARG;
}

size_t onssen_tasnet_image_bytes(const int32_t* cfg_host) {
  tas::Cfg g;
  return tas::read_cfg(cfg_host, &g) ? tas::layout(g).total : 0;
}

int onssen_tasnet_pack_f32(const int32_t* cfg_host, const float* params, void* image, size_t image_bytes, void* stream) {
  tas::Cfg g;
  if (!tas::read_cfg(cfg_host, &g) || !params || !image) return ONSSEN_E_ARG;
  const tas::Layout o = tas::layout(g);
  const tas::Flat fl = tas::flat_layout(g);
  if (image_bytes < o.total) return ONSSEN_E_WORKSPACE;
  if (!aligned256(image)) return ONSSEN_E_ALIGN;
  ONSSEN_CLEAR_ERROR();
  char* im = static_cast<char*>(image);
  hipStream_t st = (hipStream_t)stream;
  auto f = [&](size_t off) { return reinterpret_cast<float*>(im + off); };
  auto u = [&](size_t off) { return reinterpret_cast<uint16_t*>(im + off); };
  auto copy = [&](int64_t at, long rows, int K, int ld, size_t off) {      // rows x K floats of the flat buffer -> image (padded)
    hipLaunchKernelGGL(tas::tas_copy_pad_kernel, dim3(tas::ew_grid(rows * ld)), dim3(256), 0, st, params + at, rows, K, ld, f(off));
  };
  const int ldN = tas::ld4(g.N), ldB = tas::ld4(g.B), ldH = tas::ld4(g.H);
  copy(fl.enc_w, g.N, g.L, g.L, o.enc_w); copy(fl.enc_b, 1, g.N, g.N, o.enc_b);
  copy(fl.ln_g, 1, g.N, g.N, o.ln_g); copy(fl.ln_b, 1, g.N, g.N, o.ln_b);
  copy(fl.bott_w, g.B, g.N, ldN, o.bott_w); copy(fl.bott_b, 1, g.B, g.B, o.bott_b);
  for (int j = 0; j < g.R * g.X; ++j) {
    const size_t k = o.blk0 + (size_t)j * o.blk_stride;
    const int64_t b = fl.blk0 + j * fl.blk_stride;
    copy(b + fl.c1_w, g.H, g.B, ldB, k + o.c1_w); copy(b + fl.c1_b, 1, g.H, g.H, k + o.c1_b); copy(b + fl.alpha, 1, 1, 1, k + o.alpha);
    if (g.norm == ONSSEN_TASNET_BN) {
      hipLaunchKernelGGL(tas::tas_fold_bn_kernel, dim3((unsigned)ceil_div(g.H, 256)), dim3(256), 0, st, params + b + fl.n_w,
                         params + b + fl.n_b, params + b + fl.n_mu, params + b + fl.n_var, g.H, f(k + o.n_a), f(k + o.n_b));
    } else {
      copy(b + fl.n_w, 1, g.H, g.H, k + o.n_a); copy(b + fl.n_b, 1, g.H, g.H, k + o.n_b);
    }
    copy(b + fl.dw_w, g.H, g.P, g.P, k + o.dw_w); copy(b + fl.dw_b, 1, g.H, g.H, k + o.dw_b);
    copy(b + fl.sc_w, g.B, g.H, ldH, k + o.sc_w); copy(b + fl.sc_b, 1, g.B, g.B, k + o.sc_b);
  }
  copy(fl.mask_w, (long)g.spk * g.N, g.B, ldB, o.mask_w); copy(fl.mask_b, 1, g.spk * g.N, g.spk * g.N, o.mask_b);
  copy(fl.dec_w, g.N, g.L, g.L, o.dec_w); copy(fl.dec_b, 1, 1, 1, o.dec_b);
  ONSSEN_LAUNCH_CHECK();
  // x3 images of the 1x1 weights (the split-bf16 / bf16 GEMMs' B operand) from the padded fp32 copies
  int rc = onssen_x3_image_f32(f(o.bott_w), ldN, 0, 1, g.B, g.N, u(o.bott_x3), stream);
  if (!rc) rc = onssen_x3_image_f32(f(o.mask_w), ldB, 0, 1, g.spk * g.N, g.B, u(o.mask_x3), stream);
  for (int j = 0; j < g.R * g.X && !rc; ++j) {
    const size_t k = o.blk0 + (size_t)j * o.blk_stride, k3 = o.x3_blk0 + (size_t)j * o.x3_blk_stride;
    rc = onssen_x3_image_f32(f(k + o.c1_w), ldB, 0, 1, g.H, g.B, u(k3 + o.c1_x3), stream);
    if (!rc) rc = onssen_x3_image_f32(f(k + o.sc_w), ldH, 0, 1, g.B, g.H, u(k3 + o.sc_x3), stream);
  }
  return rc;
}

size_t onssen_tasnet_workspace_bytes(const int32_t* cfg_host, int n, int S) {
  tas::Cfg g;
  if (!tas::read_cfg(cfg_host, &g) || n <= 0 || S < g.L) return 0;
  return tas::ws_layout(g, n, S).total;
}

int onssen_tasnet_forward_f32(const int32_t* cfg_host, const void* image, const float* x, int n, int S, int64_t x_stride,
                              float* out, void* ws, size_t ws_bytes, void* stream) {
  tas::Cfg g;
  if (!tas::read_cfg(cfg_host, &g) || !image || !x || !out || !ws || n <= 0 || S < g.L || x_stride < S) return ONSSEN_E_ARG;
  const tas::Ws w = tas::ws_layout(g, n, S);
  if (ws_bytes < w.total) return ONSSEN_E_WORKSPACE;
  if (!aligned256(image) || !aligned256(ws)) return ONSSEN_E_ALIGN;
  const tas::Frames f = tas::frames(g, n, S);
  if (!f.ok) return ONSSEN_E_ARG;
  tas::Plan p = tas::in_place(tas::RECT, n, f.T, f.M, x, (long)x_stride, out, ws, w);
  p.S_out = f.S_out;
  return tas::run(g, image, p, stream);
}

size_t onssen_tasnet_ragged_workspace_bytes(const int32_t* cfg_host, int n, const int32_t* lengths_host) {
  tas::Cfg g;
  tas::Geo q{};
  if (!tas::read_cfg(cfg_host, &g) || !tas::ragged_geo(g, n, lengths_host, -1, &q)) return 0;
  return tas::ws_layout_rows(g, (size_t)q.M, (size_t)q.st.blk[n]).total;
}

int onssen_tasnet_forward_ragged_f32(const int32_t* cfg_host, const void* image, const float* x, int n,
                                     const int32_t* lengths_host, int64_t x_stride, float* out, int64_t out_stride, void* ws,
                                     size_t ws_bytes, void* stream) {
  tas::Cfg g;
  tas::Geo q{};
  if (!tas::read_cfg(cfg_host, &g) || !image || !x || !out || !ws || x_stride < 0) return ONSSEN_E_ARG;
  if (!tas::ragged_geo(g, n, lengths_host, x_stride, &q) || out_stride < q.S_out) return ONSSEN_E_ARG;
  const tas::Ws w = tas::ws_layout_rows(g, (size_t)q.M, (size_t)q.st.blk[n]);
  if (ws_bytes < w.total) return ONSSEN_E_WORKSPACE;
  if (!aligned256(image) || !aligned256(ws)) return ONSSEN_E_ALIGN;
  q.out_stride = out_stride;
  tas::Plan p = tas::in_place(tas::RAGGED, n, 0, q.M, x, (long)x_stride, out, ws, w);
  p.geo = &q;
  return tas::run(g, image, p, stream);
}

}  // extern "C"
