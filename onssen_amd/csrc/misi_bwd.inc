// Backward of the MISI half-step (part of onssen_hip.hip): from the gradient at the C phase maps misi_phase_kernel wrote to the
// gradient at the C time-domain estimates it read -- the link that lets a mask network be trained through K unfolded MISI
// iterations (Wang, Le Roux, Wang & Hershey 2018).  Two launches, no atomics, nothing read back by the host.
// =================================================================================================
// misi_phase_kernel computes, per utterance and in fp64,
//   u_c = s_c + (x - sum_j s_j) / C,   Z_c[t] = rfft(w * frame_t(reflect-padded u_c)),   p_c = Z_c / |Z_c|
// with p_c = (1, 0) where Z_c = 0, where the frame's operand is all zero and for the frames after the row's own.  With g_p the
// gradient at p (C, B, T, F, 2), the adjoint is
//   g_Z   = (g_p - p (p . g_p)) / |Z|                       (a real 2-vector dot product per bin; 0 where the forward fell back)
//   r_t   = w[i] * sum_f H[f] e^{+2 pi i f i / N}           the unscaled inverse transform of the Hermitian extension
//                                                           H[f] = g_Z[f] / 2 (0 < f < N/2), H[0] = Re g_Z[0], H[N/2] = Re g_Z[N/2]
//   g_u   = overlap-add of r_t on the padded axis, the reflect padding folded back:
//             padded q < N/2 adds to sample N/2 - q,  padded q >= N/2 + n_b adds to sample 2 (n_b - 1) - (q - N/2)
//   g_s_c = g_u_c - (1 / C) sum_j g_u_j                     the mixture is data and gets no gradient
// The contract is the Jacobian AT THE FLOAT32 ESTIMATES, evaluated in fp64 and rounded once: Z is recomputed from the same float32
// mix and est (the forward's float32 p is not read), every product and sum is fp64 in a fixed order, the only rounding to
// float32 is the store of g_s.  At DC and Nyquist Z is real, so p = (+-1, 0) exactly and Re g_Z = g_re - p_re p_re g_re = 0: both
// bins of H are written as 0 and their g_p is never used.
//
// (a) misi_bwd_frames_kernel -- misi_phase_kernel's layout: one wave per frame and speaker pair, `fpw` consecutive frames per wave,
//     no workgroup barrier.  The forward transform of the pair (u_c0 in the real part, u_c1 in the imaginary part), the
//     normalisation Jacobian per bin, and ONE complex inverse transform of H_c0 + i H_c1 (both Hermitian, so the result is
//     r_c0 + i r_c1: mask_istft_kernel<PAIR>'s trick) run in the same LDS buffer; the windowed frames go to the workspace
//     (C, B, T, N) as fp64.  The frame's g_p is requested before the forward transform, the next frame's samples as well.
// (b) misi_bwd_gather_kernel -- one thread per output sample: the <= 3 ceil(N / hop) workspace entries of its three padded
//     positions (its own, its mirror in the left padding, its mirror in the right padding; frames ascending) are summed in fp64
//     for all C speakers, the residual adjoint is applied and C floats are stored.  The mirrors of a sample near the right edge
//     live in the row's LAST frames, wherever the sample's own frames are: which is why the overlap-add is a pass of its own and
//     not the tail of a chunked transform kernel -- and that edge differs per row of a ragged batch.
// Ragged batch (n_per_utt): row b mirrors about its own last sample and owns frames 0 .. n_b / hop; the frames after them
// contribute nothing, their g_p and workspace entries are neither read nor written; g_s is exactly 0 from n_b on.  A device
// length is kept inside the row as misi_phase_kernel keeps it.
// =================================================================================================
// fft_wave's stages with the lane's precomputed constants (N = 256), the constants taken BY REFERENCE.  This kernel transforms
// twice per frame; through fft_wave's optional pointer the null check of the second call is not folded, and a structure whose
// address is compared stays in scratch (264 bytes per lane, measured).  Same table entries, same arithmetic and order as
// fft_wave; kept here, beside its only caller, so that fft.inc and the instruction streams of the kernels built from it stay
// exactly what they were.
template <int N>
__device__ __forceinline__ void fft_wave_lc(double* re, double* im, bool inverse, const FftLaneConst<N>& lc) {
  const double sg = inverse ? 1.0 : -1.0;   // sign of the imaginary part of the twiddles / of the +-i rotations
#pragma unroll
  for (int d = 0; d < FftPlan<N>::DIG; ++d) {
    __builtin_amdgcn_wave_barrier();
    double xr[4], xi[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double ar = re[lc.pos[d][q]], ai = im[lc.pos[d][q]];
      if (q == 0 || d == 0) {
        xr[q] = ar;
        xi[q] = ai;
      } else {
        const double wr = lc.wr[d][q - 1], wi = sg * lc.wi[d][q - 1];
        xr[q] = ar * wr - ai * wi;
        xi[q] = ar * wi + ai * wr;
      }
    }
    const double ar = xr[0] + xr[2], ai = xi[0] + xi[2], br = xr[0] - xr[2], bi = xi[0] - xi[2];
    const double cr = xr[1] + xr[3], ci = xi[1] + xi[3], dr = xr[1] - xr[3], di = xi[1] - xi[3];
    const int p0 = lc.pos[d][0], p1 = lc.pos[d][1], p2 = lc.pos[d][2], p3 = lc.pos[d][3];
    re[p0] = ar + cr;  im[p0] = ai + ci;
    re[p2] = ar - cr;  im[p2] = ai - ci;
    re[p1] = br - sg * di;  im[p1] = bi + sg * dr;
    re[p3] = br + sg * di;  im[p3] = bi - sg * dr;
  }
  __builtin_amdgcn_wave_barrier();
}

template <int N, int CT>
__global__ __launch_bounds__(256) void misi_bwd_frames_kernel(const float* __restrict__ mix, long mix_stride,
                                                              const float* __restrict__ est, long est_sb, long est_sc, int B,
                                                              int C, int n_samples, int hop, int T, int fpw,
                                                              const float* __restrict__ g_phase, double* __restrict__ ws,
                                                              const int* __restrict__ n_per_utt) {
  __shared__ double buf_re[4][fft_buf_len<N>()], buf_im[4][fft_buf_len<N>()];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int F = N / 2 + 1;
  const int ngrp = (T + 4 * fpw - 1) / (4 * fpw), utt = (int)blockIdx.x / ngrp, grp = (int)blockIdx.x - utt * ngrp;
  int t = (grp * 4 + wave) * fpw;
  int tend = t + fpw < T ? t + fpw : T;
  const int c0 = 2 * (int)blockIdx.y, c1 = c0 + 1 < C ? c0 + 1 : c0;
  double* re = buf_re[wave];
  double* im = buf_im[wave];
  if (n_per_utt) {                                     // (a device value cannot be refused by the host: kept inside the row)
    const int nb = n_per_utt[utt];
    n_samples = nb > n_samples ? n_samples : nb <= N / 2 ? N / 2 + 1 : nb;
  }
  const int Tb = 1 + n_samples / hop;                  // the row's own frames (a uniform batch: T)
  tend = tend < Tb ? tend : Tb;                        // the frames after them contribute nothing: neither read nor written
  if (t >= tend) return;                               // no workgroup-wide synchronisation anywhere in this kernel
  const float* xs = mix + (long)utt * mix_stride;
  const float* es = est + (long)utt * est_sb;
  const float* ea = es + (long)c0 * est_sc;
  const float* eb = es + (long)c1 * est_sc;
  const float* qa = g_phase + (((long)c0 * B + utt) * T) * F * 2;
  const float* qb = g_phase + (((long)c1 * B + utt) * T) * F * 2;
  double* wa = ws + (((long)c0 * B + utt) * T) * N;
  double* wb = ws + (((long)c1 * B + utt) * T) * N;
  constexpr int SPL = N / 64, FPL = N / 128;           // samples / bins below Nyquist per lane
  // the forward's operand: centred frames, reflect padding, ONE index per sample for the mixture and every estimate
  float xv[SPL], sv[CT][SPL];
  [[maybe_unused]] float sa[SPL], sb[SPL];             // CT > 2: the pair's own estimates (CT = 2: they are sv[0], sv[1])
  auto fetch = [&](int tt) {
    const int o = tt * hop - N / 2;
    const bool inside = o >= 0 && o + N <= n_samples;  // wave-uniform
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
      int p = o + lane + 64 * k;
      if (!inside) {
        p = p < 0 ? -p : p;
        p = p >= n_samples ? 2 * (n_samples - 1) - p : p;
      }
      xv[k] = xs[p];
#pragma unroll
      for (int j = 0; j < CT; ++j) sv[j][k] = es[(long)(j < C ? j : C - 1) * est_sc + p];
      if constexpr (CT > 2) {
        sa[k] = ea[p];
        sb[k] = eb[p];
      }
    }
  };
  fetch(t);
  float2 gav[FPL], gbv[FPL];                           // g_p of this lane's bins below Nyquist, both speakers
  auto fetch_g = [&](int tt) {
#pragma unroll
    for (int k = 0; k < FPL; ++k) {
      gav[k] = *reinterpret_cast<const float2*>(qa + (long)tt * F * 2 + 2 * (lane + 64 * k));
      gbv[k] = *reinterpret_cast<const float2*>(qb + (long)tt * F * 2 + 2 * (lane + 64 * k));
    }
  };
  // what does not depend on the frame: where a lane's samples go before the forward transform and its bins before the inverse
  // one (bit-reversed positions), the window weights and -- one butterfly per lane and stage, N = 256 -- the stage constants
  int jpos[SPL], jf[FPL], jmir[FPL];
  double wwin[SPL];
#pragma unroll
  for (int k = 0; k < SPL; ++k) {
    jpos[k] = fft_idx(fft_perm<N>(lane + 64 * k));
    wwin[k] = fft_win<N>(lane + 64 * k);
  }
#pragma unroll
  for (int k = 0; k < FPL; ++k) {
    const int f = lane + 64 * k;
    jf[k] = fft_idx(fft_perm<N>(f));
    jmir[k] = fft_idx(fft_perm<N>(f > 0 ? N - f : 0));
  }
  const int jnyq = fft_idx(fft_perm<N>(N / 2));
  constexpr bool kLaneConst = (N / 4 == 64) && !FftPlan<N>::kOdd;
  FftLaneConst<kLaneConst ? N : 256> lcs;
  if constexpr (kLaneConst) fft_lane_const<N>(lane, lcs);
  const double cd = (double)C;
  const bool has_b = c1 != c0;
  for (; t < tend; ++t) {
    // the forward's operand, exactly as misi_phase_kernel forms it; a frame whose operand is all zero fell back to (1, 0)
    bool za = true, zb = true;
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
      double sum = 0.0;
#pragma unroll
      for (int j = 0; j < CT; ++j) sum += j < C ? (double)sv[j][k] : 0.0;
      const double d = ((double)xv[k] - sum) / cd;
      double ua, ub;
      if constexpr (CT > 2) {
        ua = (double)sa[k];
        ub = (double)sb[k];
      } else {
        ua = (double)sv[0][k];
        ub = (double)sv[1][k];
      }
      ua += d;
      ub += d;
      za = za && ua == 0.0;
      zb = zb && ub == 0.0;
      re[jpos[k]] = ua * wwin[k];
      im[jpos[k]] = ub * wwin[k];
    }
    za = __all(za);
    zb = __all(zb);
    if (t + 1 < tend) fetch(t + 1);                    // lands under this frame's transforms
    fetch_g(t);
    if constexpr (kLaneConst) fft_wave_lc<N>(re, im, false, lcs); else fft_wave<N>(re, im, lane, false);
    // Z_a, Z_b of bins 0 .. N/2 - 1 (Nyquist needs none: its H is 0), all read before the buffer is overwritten
    double ar[FPL], ai[FPL], br[FPL], bi[FPL];
#pragma unroll
    for (int k = 0; k < FPL; ++k) {
      const int f = lane + 64 * k, fn = (N - f) & (N - 1);
      const double zr = re[fft_idx(f)], zi = im[fft_idx(f)], nr = re[fft_idx(fn)], ni = im[fft_idx(fn)];
      ar[k] = 0.5 * (zr + nr); ai[k] = 0.5 * (zi - ni);
      br[k] = 0.5 * (zi + ni); bi[k] = 0.5 * (nr - zr);
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < FPL; ++k) {
      const bool dc = (k == 0 && lane == 0);
      // H_c[f] = (g - p (p . g)) / (2 |Z|), p = Z / |Z| in fp64; 0 at DC and where the forward wrote its fallback
      const double ha = hypot(ar[k], ai[k]), hb = hypot(br[k], bi[k]);
      const bool oka = ha > 0.0 && !za && !dc, okb = hb > 0.0 && !zb && !dc && has_b;
      const double ia = 1.0 / (oka ? ha : 1.0), ib = 1.0 / (okb ? hb : 1.0);
      const double par = ar[k] * ia, pai = ai[k] * ia, pbr = br[k] * ib, pbi = bi[k] * ib;
      const double gar = (double)gav[k].x, gai = (double)gav[k].y, gbr = (double)gbv[k].x, gbi = (double)gbv[k].y;
      const double da = par * gar + pai * gai, db = pbr * gbr + pbi * gbi;
      const double har = oka ? (gar - par * da) * (0.5 * ia) : 0.0, hai = oka ? (gai - pai * da) * (0.5 * ia) : 0.0;
      const double hbr = okb ? (gbr - pbr * db) * (0.5 * ib) : 0.0, hbi = okb ? (gbi - pbi * db) * (0.5 * ib) : 0.0;
      re[jf[k]] = har - hbi;           // W[f] = H_a[f] + i H_b[f]
      im[jf[k]] = hai + hbr;
      if (!dc) {                       // Hermitian mirrors: W[N-f] = conj(H_a[f]) + i conj(H_b[f])
        re[jmir[k]] = har + hbi;
        im[jmir[k]] = -hai + hbr;
      }
    }
    if (lane == 0) {
      re[jnyq] = 0.0;
      im[jnyq] = 0.0;
    }
    if constexpr (kLaneConst) fft_wave_lc<N>(re, im, true, lcs); else fft_wave<N>(re, im, lane, true);
    double* wat = wa + (long)t * N;
    double* wbt = wb + (long)t * N;
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
      const int i = lane + 64 * k;
      wat[i] = wwin[k] * re[fft_idx(i)];
      if (has_b) wbt[i] = wwin[k] * im[fft_idx(i)];
    }
    __builtin_amdgcn_wave_barrier();   // the next frame overwrites the buffer
  }
}

template <int CT>
__global__ __launch_bounds__(256) void misi_bwd_gather_kernel(const double* __restrict__ ws, int B, int C, int n_max, int N, int hop,
                                                              int T, float* __restrict__ g_est, const int* __restrict__ n_per_utt) {
  const int b = (int)blockIdx.y, n = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (n >= n_max) return;
  const int H = N / 2;
  int nb = n_max;
  if (n_per_utt) {                                     // the clamp of misi_bwd_frames_kernel
    const int v = n_per_utt[b];
    nb = v > n_max ? n_max : v <= H ? H + 1 : v;
  }
  float* out = g_est + (long)b * C * n_max + n;
  if (n >= nb) {                                       // beyond the row's own samples: exactly 0
    for (int c = 0; c < C; ++c) out[(long)c * n_max] = 0.0f;
    return;
  }
  const int Tb = 1 + nb / hop;
  // the padded positions that carry sample n: its own, its mirror in the left padding (1 <= n <= N/2) and its mirror in the
  // right padding (n_b - 1 - N/2 <= n <= n_b - 2)
  const int q[3] = {n + H, (n >= 1 && n <= H) ? H - n : -1, (n <= nb - 2 && n >= nb - 1 - H) ? H + 2 * (nb - 1) - n : -1};
  double gu[CT];
#pragma unroll
  for (int j = 0; j < CT; ++j) gu[j] = 0.0;
  const long sc = (long)B * T * N;                     // a speaker's plane of the workspace
  const double* wrow = ws + (long)b * T * N;
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    const int p = q[m];
    if (p < 0) continue;
    const int tlo = p < N ? 0 : (p - N) / hop + 1;
    int thi = p / hop;
    thi = thi > Tb - 1 ? Tb - 1 : thi;
    for (int t = tlo; t <= thi; ++t) {                 // frames in ascending order
      const double* e = wrow + (long)t * N + (p - t * hop);
#pragma unroll
      for (int j = 0; j < CT; ++j) gu[j] += e[(long)(j < C ? j : C - 1) * sc];
    }
  }
  double sum = 0.0;
#pragma unroll
  for (int j = 0; j < CT; ++j) sum += j < C ? gu[j] : 0.0;
  const double mean = sum / (double)C;
#pragma unroll
  for (int j = 0; j < CT; ++j)
    if (j < C) out[(long)j * n_max] = (float)(gu[j] - mean);
}

// The refusals shared by the workspace query and the launch: ONSSEN_OK or ONSSEN_E_ARG.
static int misi_bwd_geometry(int B, int C, int n, int n_fft, int hop) {
  if (B <= 0 || C < 2 || C > 8 || hop <= 0 || hop > n_fft) return ONSSEN_E_ARG;
  if (n_fft != 256 && n_fft != 512 && n_fft != 1024) return ONSSEN_E_ARG;
  if (n <= n_fft / 2) return ONSSEN_E_ARG;
  return ONSSEN_OK;
}

extern "C" {

size_t onssen_misi_phase_backward_workspace_bytes(int B, int C, int n, int n_fft, int hop) {
  if (misi_bwd_geometry(B, C, n, n_fft, hop) != ONSSEN_OK) return 0;
  return (size_t)C * (size_t)B * (size_t)(1 + n / hop) * (size_t)n_fft * sizeof(double);
}

int onssen_misi_phase_backward_f32(const float* mix, int64_t mix_stride, const float* est, int64_t est_sb, int64_t est_sc, int B,
                                   int C, int n_max, const int32_t* n_per_utt, int n_fft, int hop, const float* g_phase,
                                   float* g_est, void* ws, size_t ws_bytes, void* stream) {
  if (!mix || !est || !g_phase || !g_est || !ws) return ONSSEN_E_ARG;
  if (misi_bwd_geometry(B, C, n_max, n_fft, hop) != ONSSEN_OK) return ONSSEN_E_ARG;
  if (ws_bytes < onssen_misi_phase_backward_workspace_bytes(B, C, n_max, n_fft, hop)) return ONSSEN_E_WORKSPACE;
  if ((reinterpret_cast<uintptr_t>(g_phase) & 7u) || (reinterpret_cast<uintptr_t>(ws) & 7u)) return ONSSEN_E_ALIGN;   // (re, im) pairs are read as one word
  ONSSEN_CLEAR_ERROR();
  const int T = 1 + n_max / hop;
  // the forward's grid: one wave per frame and speaker pair, `fpw` consecutive frames per wave, fewer when CUs would idle
  const int npair = ceil_div(C, 2);
  int fpw = 4;
  while (fpw > 1 && (long)B * npair * ceil_div(T, 4 * fpw) < 512) --fpw;
  const dim3 grid((unsigned)((long)B * ceil_div(T, 4 * fpw)), (unsigned)npair), block(256);
  const dim3 ggrid((unsigned)ceil_div(n_max, 256), (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
  double* wsd = static_cast<double*>(ws);
#define ONSSEN_MISI_BWD(N_, CT_)                                                                                              \
  do {                                                                                                                        \
    hipLaunchKernelGGL((misi_bwd_frames_kernel<N_, CT_>), grid, block, 0, st, mix, (long)mix_stride, est, (long)est_sb,       \
                       (long)est_sc, B, C, n_max, hop, T, fpw, g_phase, wsd, n_per_utt);                                      \
    hipLaunchKernelGGL((misi_bwd_gather_kernel<CT_>), ggrid, block, 0, st, (const double*)wsd, B, C, n_max, N_, hop, T, g_est, \
                       n_per_utt);                                                                                            \
  } while (0)
#define ONSSEN_MISI_BWD_N(N_)                                                                                              \
  do {                                                                                                                     \
    if (C == 2) ONSSEN_MISI_BWD(N_, 2);                                                                                    \
    else if (C <= 4) ONSSEN_MISI_BWD(N_, 4);                                                                               \
    else ONSSEN_MISI_BWD(N_, 8);                                                                                           \
  } while (0)
  if (n_fft == 256) ONSSEN_MISI_BWD_N(256);
  else if (n_fft == 512) ONSSEN_MISI_BWD_N(512);
  else ONSSEN_MISI_BWD_N(1024);
#undef ONSSEN_MISI_BWD_N
#undef ONSSEN_MISI_BWD
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

}  // extern "C"
