// GEMM host side (part of onssen_hip.hip; right after gemm.inc, whose kernels it launches): ONE filler for the arguments every
// x3p / x3q caller shares (xp_args), ONE tile chooser (x3q_tile), ONE dispatcher per kernel family (launch_*: every instantiation
// the library carries is spelled out there, and nowhere else), ONE reader of the four environment switches (x3q_env), the shared
// checks, and the C ABI entries over them.

#ifndef ONSSEN_X3Q_SMALL_DEFAULT
#define ONSSEN_X3Q_SMALL_DEFAULT 0   // onssen_linear_x3p, bias mode: KB (32-k blocks) up to which 128 x 128 tiles run (0 = never); ONSSEN_X3Q_SMALL overrides
#endif
#ifndef ONSSEN_X3R_DEFAULT
#define ONSSEN_X3R_DEFAULT 0     // onssen_linear_x3p, bias mode: 1 = the 32x32x16-MFMA kernel (linear_x3r_kernel) unless ONSSEN_X3R=0 says otherwise
#endif

// rows of `n` floats at p + i*s0 + j*s1 can be read / written 16 bytes at a time
static bool vec4_ok(const void* p, long n, long s0, long s1) { return aligned16(p) && (n % 4) == 0 && (s0 % 4) == 0 && (s1 % 4) == 0; }
// the register L2-norm epilogues: whole feature groups per wave tile (80 columns), at most 4 groups per lane
static bool l2_group_ok(int group) { return group > 0 && (group % 4) == 0 && (80 % group) == 0 && 80 / group <= 4; }
// the kernels index an x3 image with 32-bit byte offsets: `rows` rows (a tile's, or a row-major image's) of `blocks` 128-byte blocks
static bool x3_offsets_fit(long rows, int blocks) { return rows * blocks * 128 <= 0x7fffffffL; }

// what every x3p / x3q launch shares; the rest keeps LinearXpArgs's defaults (no batch, no second output, no residual, no
// compaction, tile_group 4, scalar C stores) until the caller sets what is its own
static LinearXpArgs xp_args(const uint16_t* a_img, const uint16_t* w_img, const float* bias, float* C, int64_t c_s0, int64_t c_s1, int R,
                            int M, int N, int KB) {
  LinearXpArgs p;
  p.A = a_img; p.W = w_img; p.bias = bias; p.C = C; p.c_s0 = (long)c_s0; p.c_s1 = (long)c_s1; p.R = R; p.M = M; p.N = N; p.KB = KB;
  return p;
}

// ---- tile shape of linear_x3q_kernel / linear_x3r_kernel ---------------------------------------------------------------
// 256 or 128 rows x 320 or 256 columns (LDS-DMA staging).  One workgroup per CU: the shape with the smallest (rounds of 256
// workgroups) x (tile area) wins, half-height tiles charged 15 % for their lower MFMA : fragment-read ratio.  The L2-norm epilogues
// stay at 320 columns (allow_bn256 = false).  force_bn = 320 / 256 and force_bm = 256 / 128 pin a dimension (other values: free).
// Candidates in the order 256x320, 256x256, 128x320, 128x256 and a strict <: the first of equal costs wins.
// rows_only: the cost without the column factor, as the pair and the compact entry have always computed it.  1.15 is no binary fraction:
// at real-number ties (40 rounds of half-height tiles against 23 of full-height ones) the two products round to different sides and the
// forms choose differently (tools/micro/gemm_host_check.cpp: 127 of the pairs up to 4096 rounds), so each caller keeps its own.
struct XqTile { int bm, bn; };
static double x3q_cost(int rounds, int bm, int bn, bool rows_only) { return (double)rounds * bm * (rows_only ? 1 : bn) * (bm == 128 ? 1.15 : 1.0); }
static XqTile x3q_tile(int M, int N, bool allow_bn256, int force_bn, int force_bm, bool rows_only = false) {
  XqTile t{256, 320};
  double best = 1e30;
  for (int cbm = 256; cbm >= 128; cbm -= 128)
    for (int cbn = 320; cbn >= 256; cbn -= 64) {
      if (cbn == 256 && (!allow_bn256 || force_bn == 320)) continue;
      if (cbn == 320 && allow_bn256 && force_bn == 256) continue;
      if (force_bm && cbm != force_bm) continue;
      const double cost = x3q_cost(ceil_div((long)ceil_div(M, cbm) * ceil_div(N, cbn), 256), cbm, cbn, rows_only);
      if (cost < best) { best = cost; t = XqTile{cbm, cbn}; }
    }
  return t;
}
static dim3 x3q_grid(XqTile t, int M, int N) { return dim3((unsigned)ceil_div(N, t.bn), (unsigned)ceil_div(M, t.bm)); }

// ---- the environment switches, read on every call (the tests switch them between calls) -------------------------------
struct X3qEnv {
  int q;          // ONSSEN_X3Q: 0 = the round-1 kernel (256 x 160), 320 / 256 = that tile width; pairs, residual and inv_norm ignore it
  int bm;         // ONSSEN_X3Q_BM: 256 / 128 = that tile height (onssen_linear_x3p and its _norms / _resid forms only)
  bool r;         // ONSSEN_X3R: the bias mode on v_mfma_f32_32x32x16_bf16 tiles (linear_x3r_kernel), every tile shape
  int small_kb;   // ONSSEN_X3Q_SMALL: the largest KB whose bias-mode GEMM takes 128 x 128 tiles (64 KB of LDS: two workgroups per CU)
};
static X3qEnv x3q_env() {
  const char *q = getenv("ONSSEN_X3Q"), *bm = getenv("ONSSEN_X3Q_BM"), *r = getenv("ONSSEN_X3R"), *s = getenv("ONSSEN_X3Q_SMALL");
  return X3qEnv{q ? atoi(q) : 1, bm ? atoi(bm) : 0, r ? atoi(r) != 0 : ONSSEN_X3R_DEFAULT != 0, s ? atoi(s) : ONSSEN_X3Q_SMALL_DEFAULT};
}

// ---- dispatchers: run-time choice -> instantiation ----------------------------------------------------------------------
// linear_x3q_kernel: 256-column tiles exist for BIAS and SIGMOID only (the L2-norm epilogues are 320 wide); both term counts
template <int MODE, int TERMS>
static void launch_x3q_terms(XqTile t, dim3 grid, hipStream_t st, const LinearXpArgs& p) {
  if constexpr (MODE == ONSSEN_EPI_BIAS || MODE == ONSSEN_EPI_SIGMOID) {
    if (t.bn != 320) {
      if (t.bm == 256) hipLaunchKernelGGL((linear_x3q_kernel<MODE, TERMS, false, 256, 256>), grid, dim3(512), 0, st, p);
      else hipLaunchKernelGGL((linear_x3q_kernel<MODE, TERMS, false, 256, 128>), grid, dim3(512), 0, st, p);
      return;
    }
  }
  if (t.bm == 256) hipLaunchKernelGGL((linear_x3q_kernel<MODE, TERMS, false, 320, 256>), grid, dim3(512), 0, st, p);
  else hipLaunchKernelGGL((linear_x3q_kernel<MODE, TERMS, false, 320, 128>), grid, dim3(512), 0, st, p);
}
template <int MODE>
static void launch_x3q(XqTile t, int terms, hipStream_t st, const LinearXpArgs& p) {
  if (terms == 1) launch_x3q_terms<MODE, 1>(t, x3q_grid(t, p.M, p.N), st, p);
  else launch_x3q_terms<MODE, 3>(t, x3q_grid(t, p.M, p.N), st, p);
}
// ... its 128 x 128 form: BIAS only
static void launch_x3q_small(int terms, hipStream_t st, const LinearXpArgs& p) {
  const dim3 grid((unsigned)ceil_div(p.N, 128), (unsigned)ceil_div(p.M, 128));
  if (terms == 1) hipLaunchKernelGGL((linear_x3q_kernel<ONSSEN_EPI_BIAS, 1, false, 128, 128>), grid, dim3(512), 0, st, p);
  else hipLaunchKernelGGL((linear_x3q_kernel<ONSSEN_EPI_BIAS, 3, false, 128, 128>), grid, dim3(512), 0, st, p);
}
// linear_x3r_kernel: BIAS only, the four tile shapes
template <int TERMS>
static void launch_x3r_terms(XqTile t, dim3 grid, hipStream_t st, const LinearXpArgs& p) {
  if (t.bm == 256 && t.bn == 320) hipLaunchKernelGGL((linear_x3r_kernel<TERMS, 320, 256>), grid, dim3(512), 0, st, p);
  else if (t.bm == 256) hipLaunchKernelGGL((linear_x3r_kernel<TERMS, 256, 256>), grid, dim3(512), 0, st, p);
  else if (t.bn == 320) hipLaunchKernelGGL((linear_x3r_kernel<TERMS, 320, 128>), grid, dim3(512), 0, st, p);
  else hipLaunchKernelGGL((linear_x3r_kernel<TERMS, 256, 128>), grid, dim3(512), 0, st, p);
}
static void launch_x3r(XqTile t, int terms, hipStream_t st, const LinearXpArgs& p) {
  if (terms == 1) launch_x3r_terms<1>(t, x3q_grid(t, p.M, p.N), st, p);
  else launch_x3r_terms<3>(t, x3q_grid(t, p.M, p.N), st, p);
}
// linear_x3p_kernel (round 1, 256 x 160): 8 or 4 waves (wms = 4 / 2), both term counts; BIAS, L2NORM, SIGMOID
template <int MODE>
static void launch_x3p(int wms, int terms, hipStream_t st, const LinearXpArgs& p) {
  const dim3 grid((unsigned)ceil_div(p.N, lxp::BN), (unsigned)ceil_div(p.M, lxp::BM)), block(128 * wms);
  if (wms == 4 && terms == 1) hipLaunchKernelGGL((linear_x3p_kernel<MODE, 4, 1>), grid, block, 0, st, p);
  else if (wms == 4) hipLaunchKernelGGL((linear_x3p_kernel<MODE, 4, 3>), grid, block, 0, st, p);
  else if (terms == 1) hipLaunchKernelGGL((linear_x3p_kernel<MODE, 2, 1>), grid, block, 0, st, p);
  else hipLaunchKernelGGL((linear_x3p_kernel<MODE, 2, 3>), grid, block, 0, st, p);
}
// linear_kernel (exact fp32): BIAS, L2NORM, SIGMOID, RELU, both A load paths; false: no such mode
template <int MODE>
static void launch_lin_mode(bool a_vec, dim3 grid, hipStream_t st, const LinearArgs& p) {
  if (a_vec) hipLaunchKernelGGL((linear_kernel<true, MODE>), grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL((linear_kernel<false, MODE>), grid, dim3(256), 0, st, p);
}
static bool launch_lin(int mode, bool a_vec, hipStream_t st, const LinearArgs& p) {
  const dim3 grid((unsigned)ceil_div(p.N, lin::BN), (unsigned)ceil_div(p.M, lin::BM));
  if (mode == ONSSEN_EPI_BIAS) launch_lin_mode<ONSSEN_EPI_BIAS>(a_vec, grid, st, p);
  else if (mode == ONSSEN_EPI_L2NORM) launch_lin_mode<ONSSEN_EPI_L2NORM>(a_vec, grid, st, p);
  else if (mode == ONSSEN_EPI_SIGMOID) launch_lin_mode<ONSSEN_EPI_SIGMOID>(a_vec, grid, st, p);
  else if (mode == ONSSEN_EPI_RELU) launch_lin_mode<ONSSEN_EPI_RELU>(a_vec, grid, st, p);
  else return false;
  return true;
}
// linear_x3_kernel (split-bf16, fp32 A): BIAS, L2NORM, SIGMOID (no RELU), both A load paths, 4 or 2 waves along M
template <int MODE>
static void launch_lx3_mode(bool a_vec, int wm, dim3 grid, hipStream_t st, const LinearX3Args& p) {
  if (a_vec && wm == 4) hipLaunchKernelGGL((linear_x3_kernel<true, MODE, 4>), grid, dim3(512), 0, st, p);
  else if (a_vec) hipLaunchKernelGGL((linear_x3_kernel<true, MODE, 2>), grid, dim3(256), 0, st, p);
  else if (wm == 4) hipLaunchKernelGGL((linear_x3_kernel<false, MODE, 4>), grid, dim3(512), 0, st, p);
  else hipLaunchKernelGGL((linear_x3_kernel<false, MODE, 2>), grid, dim3(256), 0, st, p);
}
static bool launch_lx3(int mode, bool a_vec, int wm, hipStream_t st, const LinearX3Args& p) {
  const dim3 grid((unsigned)ceil_div(p.N, lx3::BN), (unsigned)ceil_div(p.M, 64 * wm));
  if (mode == ONSSEN_EPI_BIAS) launch_lx3_mode<ONSSEN_EPI_BIAS>(a_vec, wm, grid, st, p);
  else if (mode == ONSSEN_EPI_L2NORM) launch_lx3_mode<ONSSEN_EPI_L2NORM>(a_vec, wm, grid, st, p);
  else if (mode == ONSSEN_EPI_SIGMOID) launch_lx3_mode<ONSSEN_EPI_SIGMOID>(a_vec, wm, grid, st, p);
  else return false;
  return true;
}

// ---- fp32-A entries ----------------------------------------------------------------------------------------------------
int onssen_linear_f32(const float* A, int64_t a_s0, int64_t a_s1, int R, int M, int K, const float* W, int ldw,
                      const float* bias, int N, int mode, int group, float eps, const float* resid, float* C,
                      int64_t c_s0, int64_t c_s1, void* stream) {
  if (!A || !W || !bias || !C || R <= 0 || M <= 0 || K <= 0 || N <= 0 || ldw < K) return ONSSEN_E_ARG;
  if ((ldw % 4) != 0 || !aligned16(W)) return ONSSEN_E_ALIGN;
  if (mode == ONSSEN_EPI_L2NORM && (group <= 0 || (lin::BN % group) != 0 || (N % group) != 0)) return ONSSEN_E_ARG;
  if (mode != ONSSEN_EPI_L2NORM && mode != ONSSEN_EPI_RELU && resid) return ONSSEN_E_ARG;
  ONSSEN_CLEAR_ERROR();
  LinearArgs p;
  p.A = A; p.a_s0 = (long)a_s0; p.a_s1 = (long)a_s1; p.W = W; p.bias = bias; p.resid = resid; p.C = C;
  p.c_s0 = (long)c_s0; p.c_s1 = (long)c_s1; p.R = R; p.M = M; p.N = N; p.K = K; p.ldw = ldw; p.group = group; p.eps = eps;
  if (!launch_lin(mode, vec4_ok(A, K, a_s0, a_s1), (hipStream_t)stream, p)) return ONSSEN_E_ARG;
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_linear_pack_bf16x3(const float* w, int N, int K, int ld_in, int ld_out, uint16_t* planes, void* stream) {
  if (!w || !planes || N <= 0 || K <= 0 || ld_in < K || ld_out < K || (ld_out % 32) != 0) return ONSSEN_E_ARG;
  ONSSEN_CLEAR_ERROR();
  const long n = (long)N * ld_out;
  hipLaunchKernelGGL(pack_w_bf16x3_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, w, N, K, ld_in, ld_out, planes,
                     planes + n);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_linear_bf16x3(const float* A, int64_t a_s0, int64_t a_s1, int R, int M, int K, const uint16_t* w_planes,
                         int ldw, const float* bias, int N, int mode, int group, float eps, const float* resid,
                         float* C, int64_t c_s0, int64_t c_s1, void* stream) {
  if (!A || !w_planes || !bias || !C || R <= 0 || M <= 0 || K <= 0 || N <= 0 || ldw < K) return ONSSEN_E_ARG;
  if ((ldw % 32) != 0 || !aligned16(w_planes)) return ONSSEN_E_ALIGN;
  if (mode == ONSSEN_EPI_L2NORM && (group <= 0 || (lx3::BN % group) != 0 || (N % group) != 0)) return ONSSEN_E_ARG;
  if (mode != ONSSEN_EPI_L2NORM && resid) return ONSSEN_E_ARG;
  ONSSEN_CLEAR_ERROR();
  LinearX3Args p;
  p.A = A; p.a_s0 = (long)a_s0; p.a_s1 = (long)a_s1; p.Whi = w_planes; p.Wlo = w_planes + (size_t)N * ldw;
  p.bias = bias; p.resid = resid; p.C = C; p.c_s0 = (long)c_s0; p.c_s1 = (long)c_s1; p.R = R; p.M = M; p.N = N;
  p.K = K; p.ldw = ldw; p.group = group; p.eps = eps;
  static const int x3_ablate = ONSSEN_KNOB_INT("ONSSEN_X3_ABLATE", 0), x3_gn = ONSSEN_KNOB_INT("ONSSEN_X3_GN", 4);
  p.ablate = x3_ablate; p.tile_group = x3_gn < 1 ? 1 : x3_gn;
  p.c_vec = vec4_ok(C, N, c_s0, c_s1);
  // tile height: 256 rows x 1 workgroup per CU (default), or 128 rows x 2 co-resident (ONSSEN_X3_WM=2)
  static const int wm_env = ONSSEN_KNOB_INT("ONSSEN_X3_WM", 0);
  const int wm = wm_env == 2 ? 2 : 4;   // measured: the 256-row tile re-reads W half as often and wins end to end
  if (!launch_lx3(mode, vec4_ok(A, K, a_s0, a_s1), wm, (hipStream_t)stream, p)) return ONSSEN_E_ARG;
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

// ---- fp32 -> x3 operand images -----------------------------------------------------------------------------------------
int onssen_x3_image_f32(const float* src, int64_t s0, int64_t s1, int R, int rows, int K, uint16_t* img, void* stream) {
  if (!src || !img || R <= 0 || rows <= 0 || K <= 0) return ONSSEN_E_ARG;
  if (!aligned16(img)) return ONSSEN_E_ALIGN;
  ONSSEN_CLEAR_ERROR();
  const int KB = ceil_div(K, 32);
  const long n = (long)rows * KB * 4;
  hipLaunchKernelGGL(x3_image_kernel, dim3((unsigned)((n + 255) / 256 > 16384 ? 16384 : (n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, src, (long)s0, (long)s1, R, rows, K, KB, img);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_x3_image_t_f32(const float* src, int64_t ld, int M, int K, int k_shift, uint16_t* img, void* stream) {
  if (!src || !img || M <= 0 || K <= 0 || ld < M) return ONSSEN_E_ARG;
  if (!aligned16(img)) return ONSSEN_E_ALIGN;
  ONSSEN_CLEAR_ERROR();
  const int KB = ceil_div(K, 32);
  hipLaunchKernelGGL(x3_image_t_kernel, dim3((unsigned)ceil_div(M, 64), (unsigned)KB), dim3(256), 0, (hipStream_t)stream, src,
                     (long)ld, M, K, KB, k_shift, img);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

static int x3_image_both_impl(const float* src, int64_t ld, int M, int K, uint16_t* img_rows, uint16_t* img_t, float* colsum,
                              void* stream) {
  if (!src || !img_rows || !img_t || M <= 0 || K <= 0 || ld < M) return ONSSEN_E_ARG;
  if (!aligned16(img_rows) || !aligned16(img_t)) return ONSSEN_E_ALIGN;
  ONSSEN_CLEAR_ERROR();
  const int KB = ceil_div(K, 32), MB = ceil_div(M, 32);
  hipLaunchKernelGGL(x3_image_both_kernel, dim3((unsigned)ceil_div(M, 64), (unsigned)KB), dim3(256), 0, (hipStream_t)stream, src,
                     (long)ld, M, K, KB, MB, img_rows, img_t, colsum);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_x3_image_both_f32(const float* src, int64_t ld, int M, int K, uint16_t* img_rows, uint16_t* img_t, void* stream) {
  return x3_image_both_impl(src, ld, M, K, img_rows, img_t, nullptr, stream);
}

int onssen_x3_image_both_colsum_f32(const float* src, int64_t ld, int M, int K, uint16_t* img_rows, uint16_t* img_t, float* colsum,
                                    void* stream) {
  if (!colsum) return ONSSEN_E_ARG;
  return x3_image_both_impl(src, ld, M, K, img_rows, img_t, colsum, stream);
}

// ---- batched weight-gradient GEMMs (linear_x3p_kernel's BATCH instantiation) ---------------------------------------------
static int linear_x3p_batched_impl(const uint16_t* a_img, int64_t a_bs, int M, int K, const uint16_t* w_img, int64_t w_bs,
                                   const float* bias, int N, int R, float* C, int64_t c_bs, int64_t c_s0, int64_t c_s1, int n_split,
                                   float* C2, int64_t c2_bs, int64_t c2_s0, int64_t c2_s1, int batch, void* stream,
                                   int n_split_odd = 0) {
  if (!a_img || !w_img || !bias || !C || M <= 0 || K <= 0 || N <= 0 || R <= 0 || batch <= 0 || batch > 65535) return ONSSEN_E_ARG;
  if (C2 && (n_split <= 0 || n_split >= N)) return ONSSEN_E_ARG;
  if (n_split_odd && (!C2 || n_split_odd < 0 || n_split_odd >= N)) return ONSSEN_E_ARG;
  if (!aligned16(a_img) || !aligned16(w_img) || (a_bs % 8) != 0 || (w_bs % 8) != 0) return ONSSEN_E_ALIGN;
  const int KB = ceil_div(K, 32);
  if (!x3_offsets_fit(lxp::BM, KB)) return ONSSEN_E_ARG;
  ONSSEN_CLEAR_ERROR();
  LinearXpArgs p = xp_args(a_img, w_img, bias, C, c_s0, c_s1, R, M, N, KB);
  p.c_vec = !C2 && vec4_ok(C, N, c_s0, c_s1) && (c_bs % 4) == 0;
  p.a_bs = (long)a_bs; p.w_bs = (long)w_bs; p.c_bs = (long)c_bs;
  p.C2 = C2; p.c2_s0 = (long)c2_s0; p.c2_s1 = (long)c2_s1; p.c2_bs = (long)c2_bs; p.n_split = n_split; p.n_split_odd = n_split_odd;
  const dim3 grid((unsigned)ceil_div(N, lxp::BN), (unsigned)ceil_div(M, lxp::BM), (unsigned)batch);
  hipLaunchKernelGGL((linear_x3p_kernel<ONSSEN_EPI_BIAS, 4, 3, true>), grid, dim3(512), 0, (hipStream_t)stream, p);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_linear_x3p_batched(const uint16_t* a_img, int64_t a_bs, int M, int K, const uint16_t* w_img, int64_t w_bs,
                              const float* bias, int N, float* C, int64_t c_bs, int64_t ldc, int batch, void* stream) {
  if (ldc < N) return ONSSEN_E_ARG;
  return linear_x3p_batched_impl(a_img, a_bs, M, K, w_img, w_bs, bias, N, 1, C, c_bs, ldc, 0, 0, nullptr, 0, 0, 0, batch, stream);
}

int onssen_linear_x3p_batched_split(const uint16_t* a_img, int64_t a_bs, int M, int K, const uint16_t* w_img, int64_t w_bs,
                                    const float* bias, int N, int R, float* C, int64_t c_bs, int64_t c_s0, int64_t c_s1,
                                    int n_split, float* C2, int64_t c2_bs, int64_t c2_s0, int64_t c2_s1, int batch, void* stream) {
  if (!C2) return ONSSEN_E_ARG;
  return linear_x3p_batched_impl(a_img, a_bs, M, K, w_img, w_bs, bias, N, R, C, c_bs, c_s0, c_s1, n_split, C2, c2_bs, c2_s0, c2_s1,
                                 batch, stream);
}

int onssen_linear_x3p_batched_split_alt(const uint16_t* a_img, int64_t a_bs, int M, int K, const uint16_t* w_img, int64_t w_bs,
                                        const float* bias, int N, int R, float* C, int64_t c_bs, int64_t c_s0, int64_t c_s1,
                                        int n_split, float* C2, int64_t c2_bs, int64_t c2_s0, int64_t c2_s1, int n_split_odd,
                                        int batch, void* stream) {
  if (!C2 || n_split_odd <= 0) return ONSSEN_E_ARG;
  return linear_x3p_batched_impl(a_img, a_bs, M, K, w_img, w_bs, bias, N, R, C, c_bs, c_s0, c_s1, n_split, C2, c2_bs, c2_s0, c2_s1,
                                 batch, stream, n_split_odd);
}

// dW_hh[d] = dP_d^T h_prev_d and dW_ih[d] = dP_d^T x of one bidirectional LSTM layer (the header has the layouts): two problems, two segments each
int onssen_lstm_wgrad_images_f32(const uint16_t* dp_img, const uint16_t* y_img, const uint16_t* x_img, int K, int B, int NP, int Hp,
                                 int Kx, const float* zero16, int R, float* dW_ih, int64_t ih_bs, int64_t ih_s0, int64_t ih_s1,
                                 float* dW_hh, int64_t hh_bs, int64_t hh_s0, int64_t hh_s1, void* stream) {
  if (!dp_img || !y_img || !x_img || !zero16 || !dW_ih || !dW_hh || K <= 0 || B <= 0 || R <= 0 || NP <= 0 || Hp <= 0 || Kx <= 0 ||
      (NP % 32) != 0 || (Hp % 8) != 0 || !x3_offsets_fit(K, (2 * NP) / 32))
    return ONSSEN_E_ARG;
  const int Kx8 = (Kx + 7) & ~7;          // x is read in 8-column pieces: up to 7 columns of its image's zero padding, never stored
  if (!aligned16(dp_img) || !aligned16(y_img) || !aligned16(x_img) || !aligned16(zero16)) return ONSSEN_E_ALIGN;
  ONSSEN_CLEAR_ERROR();
  LinearXtArgs p;
  p.A = dp_img; p.a_pitch = (long)(2 * NP / 32) * 128; p.a_col0[0] = 0; p.a_col0[1] = NP;
  const long y_pitch = (long)ceil_div(2 * Hp, 32) * 128, x_pitch = (long)ceil_div(Kx, 32) * 128;
  // forward direction: [h_prev (y columns [0, Hp), rows k - B) | x];  reverse: [x | h_prev (y columns [Hp, 2 Hp), rows k + B)]
  p.seg[0][0] = XtSeg{y_img, y_pitch, 0, Hp, -B, Hp};   p.seg[0][1] = XtSeg{x_img, x_pitch, 0, Kx8, 0, Kx};
  p.seg[1][0] = XtSeg{x_img, x_pitch, 0, Kx8, 0, Kx};   p.seg[1][1] = XtSeg{y_img, y_pitch, Hp, Hp, B, Hp};
  p.zero = (const unsigned short*)zero16;
  p.M = NP; p.N = Hp + Kx8; p.K = K; p.R = R;
  p.C[0][0] = dW_hh;           p.s0[0][0] = hh_s0; p.s1[0][0] = hh_s1;
  p.C[0][1] = dW_ih;           p.s0[0][1] = ih_s0; p.s1[0][1] = ih_s1;
  p.C[1][0] = dW_ih + ih_bs;   p.s0[1][0] = ih_s0; p.s1[1][0] = ih_s1;
  p.C[1][1] = dW_hh + hh_bs;   p.s0[1][1] = hh_s0; p.s1[1][1] = hh_s1;
  const dim3 grid((unsigned)ceil_div(p.N, 160), (unsigned)ceil_div(p.M, 256), 2);
  hipLaunchKernelGGL((linear_x3t_kernel<3>), grid, dim3(512), 0, (hipStream_t)stream, p);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

// one plain weight gradient C = A^T W from the images of dy and x as they were made for the forward / input-gradient GEMMs: one problem, one segment
int onssen_linear_x3t(const uint16_t* a_img, const uint16_t* w_img, int K, int M, int N, const float* zero16, float* C, int64_t ldc,
                      void* stream) {
  if (!a_img || !w_img || !zero16 || !C || K <= 0 || M <= 0 || N <= 0 || ldc < N || !x3_offsets_fit(K, ceil_div(M, 32)))
    return ONSSEN_E_ARG;
  if (!aligned16(a_img) || !aligned16(w_img) || !aligned16(zero16)) return ONSSEN_E_ALIGN;
  ONSSEN_CLEAR_ERROR();
  LinearXtArgs p;
  p.A = a_img; p.a_pitch = (long)ceil_div(M, 32) * 128;
  const long w_pitch = (long)ceil_div(N, 32) * 128;
  const int N8 = (N + 7) & ~7;
  for (int zz = 0; zz < 2; ++zz) {
    p.seg[zz][0] = XtSeg{w_img, w_pitch, 0, N8, 0, N};
    p.seg[zz][1] = XtSeg{w_img, w_pitch, 0, 0, 0, 0};
    p.C[zz][0] = p.C[zz][1] = C;
    p.s0[zz][0] = p.s0[zz][1] = ldc;
  }
  p.zero = (const unsigned short*)zero16;
  p.M = M; p.N = N8; p.K = K;
  const dim3 grid((unsigned)ceil_div(p.N, 160), (unsigned)ceil_div(p.M, 256), 1);
  hipLaunchKernelGGL((linear_x3t_kernel<3>), grid, dim3(512), 0, (hipStream_t)stream, p);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

// ---- GEMMs over x3 images: C = epi(A W^T + bias) ---------------------------------------------------------------------------
static int linear_x3p_impl(const uint16_t* a_img, int M, int K, const uint16_t* w_img, const float* bias, int N, int mode,
                           int group, float eps, const float* resid, int resid_mod, float* C, int R, int64_t c_s0,
                           int64_t c_s1, void* stream, float* inv_norm = nullptr) {
  if (!a_img || !w_img || !bias || !C || R <= 0 || M <= 0 || K <= 0 || N <= 0) return ONSSEN_E_ARG;
  if (!aligned16(a_img) || !aligned16(w_img)) return ONSSEN_E_ALIGN;
  const int KB = ceil_div(K, 32);
  if (!x3_offsets_fit(lxp::BM, KB)) return ONSSEN_E_ARG;
  const int terms = (mode & ONSSEN_EPI_BF16) ? 1 : 3;     // plain bf16 products: hi halves only
  mode &= ~ONSSEN_EPI_BF16;
  // pairs (group 2) and the residual exist in the 256/128 x 320 kernel only (onssen_linear_x3p_resid)
  const bool pairs = mode == ONSSEN_EPI_L2NORM && group == 2;
  if (mode != ONSSEN_EPI_BIAS && mode != ONSSEN_EPI_L2NORM && mode != ONSSEN_EPI_SIGMOID) return ONSSEN_E_ARG;
  if (mode == ONSSEN_EPI_L2NORM && ((!pairs && !l2_group_ok(group)) || (N % group) != 0)) return ONSSEN_E_ARG;
  if (resid && (mode != ONSSEN_EPI_L2NORM || resid_mod <= 0)) return ONSSEN_E_ARG;
  if (inv_norm && (mode != ONSSEN_EPI_L2NORM || pairs)) return ONSSEN_E_ARG;
  ONSSEN_CLEAR_ERROR();
  const X3qEnv env = x3q_env();
  LinearXpArgs p = xp_args(a_img, w_img, bias, C, c_s0, c_s1, R, M, N, KB);
  p.group = group; p.eps = eps; p.resid = resid; p.r_mod = resid ? resid_mod : 1; p.C2 = inv_norm;
  static const int x3_gn = ONSSEN_KNOB_INT("ONSSEN_X3_GN", 4);
  p.tile_group = x3_gn < 1 ? 1 : x3_gn;
  p.c_vec = vec4_ok(C, N, c_s0, c_s1);
  hipStream_t st = (hipStream_t)stream;
  const bool q_only = pairs || resid || inv_norm;         // no round-1 form of these: ONSSEN_X3Q does not apply
  const int use_q = q_only ? 1 : env.q;
  if (q_only && !x3_offsets_fit(lxq::BM_MAX, KB)) return ONSSEN_E_ARG;
  if (use_q && x3_offsets_fit(lxq::BM_MAX, KB)) {
    const XqTile t = x3q_tile(M, N, mode != ONSSEN_EPI_L2NORM, use_q, env.bm);
    // the bias mode (the projections): linear_x3r_kernel where ONSSEN_X3R asks for it -- every tile shape, so that a row's bits do not
    // depend on the shape its batch selects; else short K (KB <= ONSSEN_X3Q_SMALL) on 128 x 128 tiles (same bits as every x3q tile)
    if (mode == ONSSEN_EPI_BIAS && !env.r && KB <= env.small_kb) launch_x3q_small(terms, st, p);
    else if (mode == ONSSEN_EPI_BIAS && env.r) launch_x3r(t, terms, st, p);
    else if (mode == ONSSEN_EPI_BIAS) launch_x3q<ONSSEN_EPI_BIAS>(t, terms, st, p);
    else if (mode == ONSSEN_EPI_L2NORM) launch_x3q<ONSSEN_EPI_L2NORM>(t, terms, st, p);
    else launch_x3q<ONSSEN_EPI_SIGMOID>(t, terms, st, p);
    ONSSEN_LAUNCH_CHECK();
    return ONSSEN_OK;
  }
  static const int xp_wms = ONSSEN_KNOB_INT("ONSSEN_X3P_WAVES", 8) == 4 ? 2 : 4;   // 8 waves unless =4
  if (mode == ONSSEN_EPI_BIAS) launch_x3p<ONSSEN_EPI_BIAS>(xp_wms, terms, st, p);
  else if (mode == ONSSEN_EPI_L2NORM) launch_x3p<ONSSEN_EPI_L2NORM>(xp_wms, terms, st, p);
  else launch_x3p<ONSSEN_EPI_SIGMOID>(xp_wms, terms, st, p);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_linear_x3p(const uint16_t* a_img, int M, int K, const uint16_t* w_img, const float* bias, int N, int mode,
                      int group, float eps, float* C, int R, int64_t c_s0, int64_t c_s1, void* stream) {
  if ((mode & ~ONSSEN_EPI_BF16) == ONSSEN_EPI_L2NORM && group == 2) return ONSSEN_E_ARG;      // pairs: onssen_linear_x3p_resid
  return linear_x3p_impl(a_img, M, K, w_img, bias, N, mode, group, eps, nullptr, 0, C, R, c_s0, c_s1, stream);
}

int onssen_linear_x3p_norms(const uint16_t* a_img, int M, int K, const uint16_t* w_img, const float* bias, int N, int group,
                            float eps, float* C, float* inv_norm, void* stream) {
  if (!inv_norm || group <= 2) return ONSSEN_E_ARG;
  return linear_x3p_impl(a_img, M, K, w_img, bias, N, ONSSEN_EPI_L2NORM, group, eps, nullptr, 0, C, 1, N, 0, stream, inv_norm);
}

int onssen_linear_x3p_resid(const uint16_t* a_img, int M, int K, const uint16_t* w_img, const float* bias, int N, int group,
                            float eps, const float* resid, int resid_mod, float* C, int R, int64_t c_s0, int64_t c_s1,
                            int bf16_only, void* stream) {
  if (group != 2 && (group <= 0 || (group % 4) != 0)) return ONSSEN_E_ARG;
  return linear_x3p_impl(a_img, M, K, w_img, bias, N, ONSSEN_EPI_L2NORM | (bf16_only ? ONSSEN_EPI_BF16 : 0), group, eps, resid,
                         resid_mod, C, R, c_s0, c_s1, stream);
}

// two heads in one launch (chimera): columns < n_split normalised per group into C, the rest through the logistic into C2.
// Half-height tiles where 256-row tiles would leave CUs idle; no environment switch applies (nor to the compact form below).
int onssen_linear_x3p_pair(const uint16_t* a_img, int M, int K, const uint16_t* w_img, const float* bias, int N, int n_split,
                           int group, float eps, float* C, int R, int64_t c_s0, int64_t c_s1, float* C2, int64_t c2_s0,
                           int64_t c2_s1, int bf16_only, void* stream) {
  if (!a_img || !w_img || !bias || !C || !C2 || R <= 0 || M <= 0 || K <= 0 || N <= 0) return ONSSEN_E_ARG;
  if (!l2_group_ok(group)) return ONSSEN_E_ARG;
  if (n_split <= 0 || n_split >= N || (n_split % group) != 0) return ONSSEN_E_ARG;
  if (!aligned16(a_img) || !aligned16(w_img)) return ONSSEN_E_ALIGN;
  const int KB = ceil_div(K, 32);
  if (!x3_offsets_fit(lxq::BM_MAX, KB)) return ONSSEN_E_ARG;
  ONSSEN_CLEAR_ERROR();
  LinearXpArgs p = xp_args(a_img, w_img, bias, C, c_s0, c_s1, R, M, N, KB);
  p.group = group; p.eps = eps;
  p.C2 = C2; p.c2_s0 = (long)c2_s0; p.c2_s1 = (long)c2_s1; p.n_split = n_split;
  p.c_vec = vec4_ok(C, n_split, c_s0, c_s1);
  launch_x3q<ONSSEN_EPI_L2NORM_SIGMOID>(x3q_tile(M, N, false, 0, 0, true), bf16_only ? 1 : 3, (hipStream_t)stream, p);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

// the deep-clustering head straight into the compacted array of the active bins (dest: dc_run.inc's index)
int onssen_linear_x3p_compact(const uint16_t* a_img, int M, int K, const uint16_t* w_img, const float* bias, int N, int group,
                              float eps, const int32_t* dest, int64_t dest_bs, int F, float* comp, int R, int64_t comp_bs,
                              int bf16_only, void* stream) {
  if (!a_img || !w_img || !bias || !dest || !comp || R <= 0 || M <= 0 || K <= 0 || N <= 0 || F <= 0) return ONSSEN_E_ARG;
  if (!l2_group_ok(group) || N != F * group) return ONSSEN_E_ARG;
  if (!aligned16(a_img) || !aligned16(w_img) || !aligned16(comp) || (comp_bs % 4) != 0) return ONSSEN_E_ALIGN;
  const int KB = ceil_div(K, 32);
  if (!x3_offsets_fit(lxq::BM_MAX, KB)) return ONSSEN_E_ARG;
  ONSSEN_CLEAR_ERROR();
  LinearXpArgs p = xp_args(a_img, w_img, bias, comp, 0, comp_bs, R, M, N, KB);
  p.group = group; p.eps = eps;
  p.dest = dest; p.dest_bs = (long)dest_bs; p.F = F;
  p.c_vec = 1;
  launch_x3q<ONSSEN_EPI_L2NORM_COMPACT>(x3q_tile(M, N, false, 0, 0, true), bf16_only ? 1 : 3, (hipStream_t)stream, p);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}
