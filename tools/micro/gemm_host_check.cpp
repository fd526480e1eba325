// The GEMM host code (csrc/gemm_run.inc) as a stand-alone host program: the library's translation unit compiled against the mock HIP
// runtime of tests/emu, INCLUDED here so that the file-local tile chooser can be called.  From the repository root:
//   g++ -x c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover -I tests/emu/include -pthread \
//       tools/micro/gemm_host_check.cpp -o gemm_host_check && ./gemm_host_check
// 1. Tile chooser sweep.  The three cost expressions as the GEMM entries carried them before x3q_tile existed -- the loop of
//    onssen_linear_x3p and the two closed expressions of onssen_linear_x3p_pair / _compact -- verbatim beside x3q_cost / x3q_tile:
//    over every round-count pair (r128, r256), r256 <= r128 <= 2 r256 <= 8192, and over every M in 1 .. 16384 for 13 widths N, every
//    forcing of onssen_linear_x3p.  Also counted: where the loop's form and the closed form differ from EACH OTHER (the reason why
//    x3q_tile has its rows_only flag).
// 2. Every GEMM entry once or twice on small host buffers of exactly the size the call may touch (for the sanitizers), and a
//    refusal of each.
// Prints its counts and exits 0 if nothing disagrees and no return code is unexpected; a sanitizer report aborts.
#include "../../onssen_amd/csrc/onssen_hip.hip"

#include <stdio.h>
#include <string.h>
#include <vector>

// ---- the expressions before x3q_tile, verbatim ------------------------------------------------------------------------
static void old_loop(int M, int N, int mode, int use_q, int force_bm, int* bm_out, int* bn_out) {
  int bm = 256, bn = 320;
  double best = 1e30;
  for (int cbm = 256; cbm >= 128; cbm -= 128)
    for (int cbn = 320; cbn >= 256; cbn -= 64) {
      if (cbn == 256 && (mode == ONSSEN_EPI_L2NORM || use_q == 320)) continue;
      if (cbn == 320 && use_q == 256 && mode != ONSSEN_EPI_L2NORM) continue;
      if (force_bm && cbm != force_bm) continue;
      const double cost = (double)ceil_div((long)ceil_div(M, cbm) * ceil_div(N, cbn), 256) * cbm * cbn * (cbm == 128 ? 1.15 : 1.0);
      if (cost < best) { best = cost; bm = cbm; bn = cbn; }
    }
  *bm_out = bm; *bn_out = bn;
}
static int old_pair(int M, int N) {
  const long t256 = (long)ceil_div(M, 256) * ceil_div(N, 320), t128 = (long)ceil_div(M, 128) * ceil_div(N, 320);
  const int bm = (double)ceil_div(t128, 256L) * 128 * 1.15 < (double)ceil_div(t256, 256L) * 256 ? 128 : 256;
  return bm;
}
static int old_compact(int M, int N) {
  const long t256 = (long)ceil_div(M, 256) * ceil_div(N, 320), t128 = (long)ceil_div(M, 128) * ceil_div(N, 320);
  const int bm = (double)ceil_div(t128, 256L) * 128 * 1.15 < (double)ceil_div(t256, 256L) * 256 ? 128 : 256;
  return bm;
}

static long sweep() {
  long bad = 0, pairs = 0, forms_differ = 0, shapes = 0;
  for (int r256 = 1; r256 <= 4096; ++r256)
    for (int r128 = r256; r128 <= 2 * r256; ++r128, ++pairs) {
      const bool closed = (double)r128 * 128 * 1.15 < (double)r256 * 256;
      const bool loop = (double)r128 * 128 * 320 * 1.15 < (double)r256 * 256 * 320 * 1.0;
      bad += closed != (x3q_cost(r128, 128, 320, true) < x3q_cost(r256, 256, 320, true));
      bad += loop != (x3q_cost(r128, 128, 320, false) < x3q_cost(r256, 256, 320, false));
      if (closed != loop && forms_differ++ < 4) printf("  the two forms differ at r128 = %d, r256 = %d: closed %d, loop %d\n", r128, r256, closed, loop);
    }
  const int Ns[] = {1, 129, 256, 257, 320, 321, 440, 514, 600, 1200, 2400, 2580, 4800};
  const int modes[] = {ONSSEN_EPI_BIAS, ONSSEN_EPI_L2NORM, ONSSEN_EPI_SIGMOID}, qs[] = {1, 256, 320}, bms[] = {0, 128, 256, 64};
  for (int N : Ns)
    for (int M = 1; M <= 16384; ++M, ++shapes) {
      for (int mode : modes)
        for (int q : qs)
          for (int fbm : bms) {
            int bm, bn;
            old_loop(M, N, mode, q, fbm, &bm, &bn);
            const XqTile t = x3q_tile(M, N, mode != ONSSEN_EPI_L2NORM, q, fbm);
            bad += t.bm != bm || t.bn != bn;
          }
      const XqTile t = x3q_tile(M, N, false, 0, 0, true);
      bad += t.bn != 320 || t.bm != old_pair(M, N) || t.bm != old_compact(M, N);
    }
  printf("tile chooser: %ld round-count pairs (both forms) and %ld shapes x (36 forcings of x3p + pair + compact): %ld disagreements; "
         "the loop's and the closed form differ from each other at %ld pairs\n", pairs, shapes, bad, forms_differ);
  return bad;
}

// ---- every entry on exactly-sized host buffers --------------------------------------------------------------------------
template <class T>
static T* exact(size_t n, int fill) {          // n elements, 16-byte aligned, nothing behind them
  T* p = (T*)aligned_alloc(16, (n * sizeof(T) + 15) / 16 * 16);
  memset(p, fill, n * sizeof(T));
  return p;
}
static float* values(size_t n, unsigned seed) {
  float* p = exact<float>(n, 0);
  for (size_t i = 0; i < n; ++i) p[i] = (float)(((i + seed) * 2654435761u >> 7) % 2001) / 1000.f - 1.f;
  return p;
}

static int entries() {
  int bad = 0;
  const int R = 3, T = 11, M = R * T, K = 37, N = 40, KB = (K + 31) / 32, ld32 = 64, group = 20, F = N / group;
  float *A = values((size_t)M * K, 1), *W = values((size_t)N * ld32, 2), *bias = values(N, 3), *resid = values((size_t)M * N, 4);
  float *C = exact<float>((size_t)M * N, 0xff), *C2 = exact<float>((size_t)M * N, 0xff), *zero16 = exact<float>(4, 0);
  uint16_t *planes = exact<uint16_t>((size_t)2 * N * ld32, 0xa5), *a_img = exact<uint16_t>((size_t)M * KB * 64, 0xa5);
  uint16_t *w_img = exact<uint16_t>((size_t)N * KB * 64, 0xa5);
  // fp32-A forms: every mode, scalar (odd K) A loads; refusals
  for (int mode : {ONSSEN_EPI_BIAS, ONSSEN_EPI_L2NORM, ONSSEN_EPI_SIGMOID, ONSSEN_EPI_RELU})
    bad += onssen_linear_f32(A, K, (int64_t)T * K, R, M, K, W, ld32, bias, N, mode, group, 1e-12f, mode == ONSSEN_EPI_RELU ? resid : nullptr, C, N,
                             (int64_t)T * N, nullptr) != 0;
  bad += onssen_linear_f32(A, K, (int64_t)T * K, R, M, K, W, ld32, bias, N, 7, group, 0.f, nullptr, C, N, (int64_t)T * N, nullptr) != ONSSEN_E_ARG;
  bad += onssen_linear_f32(A, K, (int64_t)T * K, R, M, K, W, 38, bias, N, 0, 0, 0.f, nullptr, C, N, (int64_t)T * N, nullptr) != ONSSEN_E_ALIGN;
  bad += onssen_linear_pack_bf16x3(W, N, K, ld32, ld32, planes, nullptr) != 0;
  bad += onssen_linear_pack_bf16x3(W, N, K, ld32, 40, planes, nullptr) != ONSSEN_E_ARG;
  for (int mode : {ONSSEN_EPI_BIAS, ONSSEN_EPI_L2NORM, ONSSEN_EPI_SIGMOID})
    bad += onssen_linear_bf16x3(A, K, (int64_t)T * K, R, M, K, planes, ld32, bias, N, mode, group, 1e-12f, nullptr, C, N, (int64_t)T * N, nullptr) != 0;
  bad += onssen_linear_bf16x3(A, K, (int64_t)T * K, R, M, K, planes, ld32, bias, N, ONSSEN_EPI_RELU, 0, 0.f, nullptr, C, N, (int64_t)T * N, nullptr) != ONSSEN_E_ARG;
  // images
  bad += onssen_x3_image_f32(A, K, (int64_t)T * K, R, M, K, a_img, nullptr) != 0;
  bad += onssen_x3_image_f32(W, ld32, 0, 1, N, K, w_img, nullptr) != 0;
  bad += onssen_x3_image_f32(A, K, (int64_t)T * K, R, M, K, a_img + 1, nullptr) != ONSSEN_E_ALIGN;
  // x3 GEMMs: every mode and kernel family, both term counts
  const char* q_env[] = {nullptr, "0", "256", "320"};
  for (const char* q : q_env)
    for (int r = 0; r < 2; ++r)
      for (int mode : {ONSSEN_EPI_BIAS, ONSSEN_EPI_L2NORM, ONSSEN_EPI_SIGMOID | ONSSEN_EPI_BF16}) {
        q ? setenv("ONSSEN_X3Q", q, 1) : unsetenv("ONSSEN_X3Q");
        setenv("ONSSEN_X3R", r ? "1" : "0", 1);
        setenv("ONSSEN_X3Q_BM", r ? "128" : "256", 1);
        bad += onssen_linear_x3p(a_img, M, K, w_img, bias, N, mode, group, 1e-12f, C, R, N, (int64_t)T * N, nullptr) != 0;
      }
  unsetenv("ONSSEN_X3Q"); unsetenv("ONSSEN_X3R"); unsetenv("ONSSEN_X3Q_BM");
  setenv("ONSSEN_X3Q_SMALL", "4", 1);
  bad += onssen_linear_x3p(a_img, M, K, w_img, bias, N, ONSSEN_EPI_BIAS, 0, 0.f, C, R, N, (int64_t)T * N, nullptr) != 0;
  unsetenv("ONSSEN_X3Q_SMALL");
  bad += onssen_linear_x3p(a_img, M, K, w_img, bias, N, ONSSEN_EPI_L2NORM, 2, 1e-12f, C, R, N, (int64_t)T * N, nullptr) != ONSSEN_E_ARG;
  bad += onssen_linear_x3p(a_img, M, K, w_img, bias, N, ONSSEN_EPI_L2NORM, 12, 1e-12f, C, R, N, (int64_t)T * N, nullptr) != ONSSEN_E_ARG;
  bad += onssen_linear_x3p_norms(a_img, M, K, w_img, bias, N, group, 1e-12f, C, C2, nullptr) != 0;          // C2: [M][N / group]
  bad += onssen_linear_x3p_norms(a_img, M, K, w_img, bias, N, 2, 1e-12f, C, C2, nullptr) != ONSSEN_E_ARG;
  for (int g : {2, 20})
    bad += onssen_linear_x3p_resid(a_img, M, K, w_img, bias, N, g, 1e-12f, resid, R, C, R, N, (int64_t)T * N, g == 2, nullptr) != 0;
  bad += onssen_linear_x3p_resid(a_img, M, K, w_img, bias, N, 3, 1e-12f, resid, R, C, R, N, (int64_t)T * N, 0, nullptr) != ONSSEN_E_ARG;
  for (int bf = 0; bf < 2; ++bf)                                                                             // columns [0, 20) -> C, [20, 40) -> C2
    bad += onssen_linear_x3p_pair(a_img, M, K, w_img, bias, N, group, group, 1e-12f, C, R, group, (int64_t)T * group, C2, N - group,
                                  (int64_t)T * (N - group), bf, nullptr) != 0;
  bad += onssen_linear_x3p_pair(a_img, M, K, w_img, bias, N, 10, group, 1e-12f, C, R, N, (int64_t)T * N, C2, N, (int64_t)T * N, 0, nullptr) != ONSSEN_E_ARG;
  {
    int32_t* dest = exact<int32_t>((size_t)R * T * F, 0);                                                    // every second bin kept
    for (int b = 0; b < R; ++b)
      for (int i = 0; i < T * F; ++i) dest[b * T * F + i] = (i & 1) ? -1 : i / 2;
    float* comp = exact<float>((size_t)R * T * F * group, 0xff);
    for (int bf = 0; bf < 2; ++bf)
      bad += onssen_linear_x3p_compact(a_img, M, K, w_img, bias, N, group, 1e-12f, dest, (int64_t)T * F, F, comp, R, (int64_t)T * F * group, bf, nullptr) != 0;
    bad += onssen_linear_x3p_compact(a_img, M, K, w_img, bias, N, group, 1e-12f, dest, (int64_t)T * F, F + 1, comp, R, (int64_t)T * F * group, 0, nullptr) != ONSSEN_E_ARG;
    free(dest); free(comp);
  }
  // batched forms (A = the weights' image as a second batch of rows), with and without the second output
  bad += onssen_linear_x3p_batched(a_img, 0, M, K, w_img, 0, bias, N, C, 0, N, 1, nullptr) != 0;
  bad += onssen_linear_x3p_batched_split(a_img, 0, M, K, w_img, 0, bias, N, 1, C, 0, 24, 0, 24, C2, 0, 16, 0, 1, nullptr) != 0;
  bad += onssen_linear_x3p_batched_split_alt(a_img, 0, M, K, w_img, 0, bias, N, 1, C, 0, 24, 0, 24, C2, 0, 16, 0, 16, 1, nullptr) != 0;
  bad += onssen_linear_x3p_batched(a_img, 0, M, K, w_img, 0, bias, N, C, 0, N, 65536, nullptr) != ONSSEN_E_ARG;
  bad += onssen_linear_x3p_batched_split(a_img, 4, M, K, w_img, 0, bias, N, 1, C, 0, 24, 0, 24, C2, 0, 16, 0, 1, nullptr) != ONSSEN_E_ALIGN;
  // weight gradients from row-major images: dy [Kc][Mg], x [Kc][Ng]
  {
    const int Kc = 21, Mg = 44, Ng = 27, MB = (Mg + 31) / 32, NB = (Ng + 31) / 32;
    float *dy = values((size_t)Kc * Mg, 5), *x = values((size_t)Kc * Ng, 6), *dW = exact<float>((size_t)Mg * Ng, 0xff);
    uint16_t *dy_rows = exact<uint16_t>((size_t)Kc * MB * 64, 0xa5), *x_rows = exact<uint16_t>((size_t)Kc * NB * 64, 0xa5);
    uint16_t *dy_t = exact<uint16_t>((size_t)Mg * ((Kc + 31) / 32) * 64, 0xa5), *x_t = exact<uint16_t>((size_t)Ng * ((Kc + 31) / 32) * 64, 0xa5);
    float* colsum = exact<float>((size_t)((Kc + 31) / 32) * Mg, 0xff);
    bad += onssen_x3_image_both_f32(dy, Mg, Mg, Kc, dy_rows, dy_t, nullptr) != 0;
    bad += onssen_x3_image_both_colsum_f32(x, Ng, Ng, Kc, x_rows, x_t, colsum, nullptr) != 0;
    bad += onssen_x3_image_both_colsum_f32(x, Ng, Ng, Kc, x_rows, x_t, nullptr, nullptr) != ONSSEN_E_ARG;
    bad += onssen_x3_image_t_f32(dy, Mg, Mg, Kc, 0, dy_t, nullptr) != 0;
    bad += onssen_x3_image_t_f32(dy, Mg - 1, Mg, Kc, 0, dy_t, nullptr) != ONSSEN_E_ARG;
    bad += onssen_linear_x3t(dy_rows, x_rows, Kc, Mg, Ng, zero16, dW, Ng, nullptr) != 0;
    bad += onssen_linear_x3t(dy_rows, x_rows, Kc, Mg, Ng, zero16, dW, Ng - 1, nullptr) != ONSSEN_E_ARG;
    free(dy); free(x); free(dW); free(dy_rows); free(x_rows); free(dy_t); free(x_t); free(colsum);
  }
  {
    const int B = 2, Tt = 3, Kc = B * Tt, Hp = 8, NP = 32, Kx = 13;                                          // one BLSTM layer: H = Hp = 8
    uint16_t* dp = exact<uint16_t>((size_t)Kc * (2 * NP / 32) * 64, 0), *y = exact<uint16_t>((size_t)Kc * 1 * 64, 0);
    uint16_t* xi = exact<uint16_t>((size_t)Kc * 1 * 64, 0);
    float *dW_ih = exact<float>((size_t)2 * NP * Kx, 0xff), *dW_hh = exact<float>((size_t)2 * NP * Hp, 0xff);
    bad += onssen_lstm_wgrad_images_f32(dp, y, xi, Kc, B, NP, Hp, Kx, zero16, 1, dW_ih, (int64_t)NP * Kx, Kx, 0, dW_hh, (int64_t)NP * Hp, Hp, 0, nullptr) != 0;
    bad += onssen_lstm_wgrad_images_f32(dp, y, xi, Kc, B, 40, Hp, Kx, zero16, 1, dW_ih, (int64_t)NP * Kx, Kx, 0, dW_hh, (int64_t)NP * Hp, Hp, 0, nullptr) != ONSSEN_E_ARG;
    free(dp); free(y); free(xi); free(dW_ih); free(dW_hh);
  }
  free(A); free(W); free(bias); free(resid); free(C); free(C2); free(zero16); free(planes); free(a_img); free(w_img);
  printf("entries: %d unexpected return codes\n", bad);
  return bad;
}

int main() {
  const long bad = sweep() + entries();
  return bad != 0;
}
