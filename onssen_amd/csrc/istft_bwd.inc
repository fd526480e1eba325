// Backward of mask_istft_kernel (part of onssen_hip.hip): from the gradient at the C waveforms to the gradient at the masks /
// magnitudes (and, in the phase mode, at the phase maps), in one launch.
// =================================================================================================
// mask_istft_kernel computes, for row b, speaker c and sample n < len_b,
//   y_c[n] = rw[n] * sum_t (w[i] / N) * c2r(S_c[t])[i],   i = n + N/2 - t hop,  0 <= i < N,  t < T_b
//   rw[n]  = 1 / wss[n] if wss[n] > DBL_MIN else 1,       wss[n] = sum_t w[i]^2 over the same frames
// with S_c = X m_c (MASK), m_c |X| p_c (PHASE) or m_c X / |X| (MAG); the imaginary parts at DC and Nyquist are ignored.  There is
// no reflect padding on that side, so with gy the gradient at y (taken as zero at n >= len_b) the adjoint is a windowed forward
// transform of a real signal:
//   g_t[i]    = (w[i] / N) * rw[n] * gy_c[n],  n = t hop + i - N/2   (0 outside [0, len_b))
//   G_c[t, f] = a_f * sum_i g_t[i] e^{-2 pi i f i / N},               a_f = 1 at f in {0, N/2}, else 2
//   MASK :  g_mask_c = Re X Re G + Im X Im G                          (the Im X term is 0 at DC / Nyquist)
//   PHASE:  g_mask_c = |X| (Re p Re G + Im p Im G),  g_phase_c = m_c |X| (Re G, Im G), imaginary part 0 at DC / Nyquist
//   MAG  :  g_mag_c  = Re u Re G + Im u Im G,  u = X / |X| exactly as the forward forms it
// and everything is zero for the frames t >= T_b.
//
// One wave per frame, no workgroup barrier, `fpw` consecutive frames of one utterance per wave -- stft_logmag_kernel's shape with
// another load and another epilogue.  PAIR: TWO speakers of one frame share one complex transform (g of c0 in the real part, of
// c1 in the imaginary part; both are real, so FFT(g_c0)[f] = (Z[f] + conj Z[N-f]) / 2 and FFT(g_c1)[f] = (Z[f] - conj Z[N-f]) / (2i));
// blockIdx.y counts speaker pairs, the last pair of an odd C repeats its speaker and drops the copy.  MAG is unpaired, like its
// forward.
// The operand is formed on load in fp64.  rw[n] is RECOMPUTED there, not read from a prescaled copy of gy: the window terms of a
// sample are w[i - e hop]^2 over the frames t + e that exist, so for every frame whose neighbours all exist -- all but
// ceil(N / hop) - 1 frames at either end of an utterance -- the coefficient (w[i] / N) rw[n] does not depend on the frame: a wave
// builds it once per lane and sample and a frame's load is then one multiplication per sample; only the edge frames walk their
// window terms.  (A prescale would need a workspace, a launch and another pass over gy.)
// A frame's samples are one batch of independent loads, the next frame's batch is issued before this frame's transform; the
// epilogue's operands (X, and in the phase mode the masks and phase vectors) are requested before the transform as well.
// The epilogue is fp64 with one rounding.  g_operand is (B, T, F, C) contiguous -- one 8-byte store per bin when C = 2 and the
// buffer allows it (V2) --, g_phase (C, B, T, F, 2) contiguous, one 8-byte store per bin: the layout phase_istft reads.
// Deterministic (no atomics), nothing is read of gy beyond len_b or of X / mask / phase at t >= T_b.
// =================================================================================================
template <int N, bool PAIR, int MODE>
__global__ __launch_bounds__(256) void istft_bwd_kernel(const float* __restrict__ stft_ri, const float* __restrict__ mask, long m_sb,
                                                        long m_sc, long m_st, long m_sf, const float* __restrict__ phase, long p_sc,
                                                        int B, int C, int T, int hop, int length, int fpw,
                                                        const int* __restrict__ frames, const int* __restrict__ lengths,
                                                        const float* __restrict__ gy, float* __restrict__ g_op,
                                                        float* __restrict__ g_phase, int v2) {
  constexpr bool PHASE = MODE == ISTFT_PHASE, MAG = MODE == ISTFT_MAG;
  static_assert(!(MAG && PAIR), "the magnitude form is unpaired");
  __shared__ double buf_re[4][fft_buf_len<N>()], buf_im[4][fft_buf_len<N>()];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int F = N / 2 + 1;
  const int ngrp = (T + 4 * fpw - 1) / (4 * fpw), b = (int)blockIdx.x / ngrp, grp = (int)blockIdx.x - b * ngrp;
  int t = (grp * 4 + wave) * fpw;
  const int tend = t + fpw < T ? t + fpw : T;
  if (t >= tend) return;                               // no workgroup-wide synchronisation anywhere in this kernel
  const int c0 = PAIR ? 2 * (int)blockIdx.y : (int)blockIdx.y, c1 = (PAIR && c0 + 1 < C) ? c0 + 1 : c0;
  const bool has_b = c1 != c0;
  double* re = buf_re[wave];
  double* im = buf_im[wave];
  // (device values cannot be refused by the host: kept inside the row)
  int Tb = frames ? frames[b] : T, len_b = lengths ? lengths[b] : length;
  Tb = Tb < 0 ? 0 : Tb > T ? T : Tb;
  len_b = len_b < 0 ? 0 : len_b > length ? length : len_b;
  const float* ga = gy + ((long)b * C + c0) * length;
  const float* gb = gy + ((long)b * C + c1) * length;
  constexpr int SPL = N / 64, FPL = N / 128;           // samples / bins below Nyquist per lane
  float sa[SPL];
  [[maybe_unused]] float sb[SPL];
  auto fetch = [&](int tt) {
    const int o = tt * hop - N / 2;
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
      const int n = o + lane + 64 * k;
      const bool ok = n >= 0 && n < len_b;             // nothing of gy beyond the row's length is read
      sa[k] = ok ? ga[ok ? n : 0] : 0.0f;
      if constexpr (PAIR) sb[k] = ok ? gb[ok ? n : 0] : 0.0f;
    }
  };
  if (t < Tb) fetch(t);
  // what does not depend on the frame: where a lane's samples go (bit-reversed position), the coefficient (w[i] / N) rw[n] of a
  // frame whose neighbours all exist, and -- one butterfly per lane and stage, N = 256 -- the stage constants; requested after
  // the first frame's samples (one round trip)
  const double inv_n = 1.0 / (double)N;
  const int reach = (N - 1) / hop;                     // frames t - reach .. t + reach can overlap frame t
  int jpos[SPL];
  double cfull[SPL];
#pragma unroll
  for (int k = 0; k < SPL; ++k) {
    const int i = lane + 64 * k;
    jpos[k] = fft_idx(fft_perm<N>(i));
    double wss = 0.0;
    for (int j = i + (N - 1 - i) / hop * hop; j >= 0; j -= hop) {      // frames in ascending order: window index descending
      const double w = fft_win<N>(j);
      wss += w * w;
    }
    cfull[k] = (fft_win<N>(i) * inv_n) * (wss > 2.2250738585072014e-308 ? 1.0 / wss : 1.0);
  }
  constexpr bool kLaneConst = (N / 4 == 64) && !FftPlan<N>::kOdd;
  FftLaneConst<kLaneConst ? N : 256> lcs;
  if constexpr (kLaneConst) fft_lane_const<N>(lane, lcs);
  // the epilogue's operands of this lane's bins
  float2 xv[FPL];
  float xnyq_re;
  [[maybe_unused]] float xnyq_im;
  [[maybe_unused]] float2 pav[FPL], pbv[FPL];
  [[maybe_unused]] float mav[FPL], mbv[FPL], manyq, mbnyq, panyq, pbnyq;
  auto fetch_ops = [&](int tt) {
    const float* xs = stft_ri + ((long)b * T + tt) * F * 2;
#pragma unroll
    for (int k = 0; k < FPL; ++k) xv[k] = *reinterpret_cast<const float2*>(xs + 2 * (lane + 64 * k));
    xnyq_re = xs[N];
    if constexpr (PHASE || MAG) xnyq_im = xs[N + 1];
    if constexpr (PHASE) {
      const float* ms0 = mask + (long)b * m_sb + (long)c0 * m_sc + (long)tt * m_st;
      const float* ms1 = mask + (long)b * m_sb + (long)c1 * m_sc + (long)tt * m_st;
      const float* pa = phase + (long)c0 * p_sc + ((long)b * T + tt) * F * 2;
      const float* pb = phase + (long)c1 * p_sc + ((long)b * T + tt) * F * 2;
#pragma unroll
      for (int k = 0; k < FPL; ++k) {
        mav[k] = ms0[(long)(lane + 64 * k) * m_sf];
        mbv[k] = ms1[(long)(lane + 64 * k) * m_sf];
        pav[k] = *reinterpret_cast<const float2*>(pa + 2 * (lane + 64 * k));
        pbv[k] = *reinterpret_cast<const float2*>(pb + 2 * (lane + 64 * k));
      }
      manyq = ms0[(long)(N / 2) * m_sf];
      mbnyq = ms1[(long)(N / 2) * m_sf];
      panyq = pa[N];
      pbnyq = pb[N];
    }
  };
  for (; t < tend; ++t) {
    float* oa = g_op + (((long)b * T + t) * F) * C;      // element (f, c) at oa[f * C + c]
    [[maybe_unused]] float* qa = PHASE ? g_phase + (((long)c0 * B + b) * T + t) * F * 2 : nullptr;
    [[maybe_unused]] float* qb = PHASE ? g_phase + (((long)c1 * B + b) * T + t) * F * 2 : nullptr;
    if (t >= Tb) {                                     // after the row's own frames: the forward read nothing of them
      for (int f = lane; f < F; f += 64) {
        oa[(long)f * C + c0] = 0.0f;
        if (has_b) oa[(long)f * C + c1] = 0.0f;
        if constexpr (PHASE) {
          *reinterpret_cast<float2*>(qa + 2 * f) = make_float2(0.f, 0.f);
          if (has_b) *reinterpret_cast<float2*>(qb + 2 * f) = make_float2(0.f, 0.f);
        }
      }
      continue;
    }
    if (t >= reach && t + reach < Tb) {                // wave-uniform: every frame that can overlap this one exists
#pragma unroll
      for (int k = 0; k < SPL; ++k) {
        re[jpos[k]] = cfull[k] * (double)sa[k];
        im[jpos[k]] = PAIR ? cfull[k] * (double)sb[k] : 0.0;
      }
    } else {                                           // an edge frame: the window terms of the frames that exist, in frame order
#pragma unroll
      for (int k = 0; k < SPL; ++k) {
        const int i = lane + 64 * k;
        int elo = (N - 1 - i) / hop, ehi = i / hop;    // frames t - elo .. t + ehi cover this sample
        elo = elo > t ? t : elo;
        ehi = t + ehi > Tb - 1 ? Tb - 1 - t : ehi;
        double wss = 0.0;
        for (int e = -elo; e <= ehi; ++e) {
          const double w = fft_win<N>(i - e * hop);
          wss += w * w;
        }
        const double cf = (fft_win<N>(i) * inv_n) * (wss > 2.2250738585072014e-308 ? 1.0 / wss : 1.0);
        re[jpos[k]] = cf * (double)sa[k];
        im[jpos[k]] = PAIR ? cf * (double)sb[k] : 0.0;
      }
    }
    if (t + 1 < tend && t + 1 < Tb) fetch(t + 1);      // lands under this frame's transform
    fetch_ops(t);
    if constexpr (kLaneConst) fft_wave<N>(re, im, lane, false, &lcs); else fft_wave<N>(re, im, lane, false);
    // bins 0 .. N/2 - 1 (the Nyquist bin follows): the LDS reads first, then the products and the stores
    double ar[FPL], ai[FPL];
    [[maybe_unused]] double br[FPL], bi[FPL];
#pragma unroll
    for (int k = 0; k < FPL; ++k) {
      const int f = lane + 64 * k, fn = (N - f) & (N - 1);
      const double zr = re[fft_idx(f)], zi = im[fft_idx(f)], nr = re[fft_idx(fn)], ni = im[fft_idx(fn)];
      const double a = f == 0 ? 0.5 : 1.0;             // a_f / 2: the sum over the mirror pair counts DC twice
      ar[k] = a * (zr + nr); ai[k] = a * (zi - ni);
      if constexpr (PAIR) { br[k] = a * (zi + ni); bi[k] = a * (nr - zr); }
    }
#pragma unroll
    for (int k = 0; k < FPL; ++k) {
      const int f = lane + 64 * k;
      const bool dc = f == 0;
      float va, vb = 0.0f;
      if constexpr (PHASE) {
        const double mag = (double)hypotf(xv[k].x, xv[k].y);
        const double par = (double)pav[k].x, pai = dc ? 0.0 : (double)pav[k].y;
        const double pbr = (double)pbv[k].x, pbi = dc ? 0.0 : (double)pbv[k].y;
        va = (float)(mag * (par * ar[k] + pai * ai[k]));
        const double sa_ = (double)mav[k] * mag;
        *reinterpret_cast<float2*>(qa + 2 * f) = make_float2((float)(sa_ * ar[k]), dc ? 0.0f : (float)(sa_ * ai[k]));
        if constexpr (PAIR) {
          vb = (float)(mag * (pbr * br[k] + pbi * bi[k]));
          const double sb_ = (double)mbv[k] * mag;
          if (has_b) *reinterpret_cast<float2*>(qb + 2 * f) = make_float2((float)(sb_ * br[k]), dc ? 0.0f : (float)(sb_ * bi[k]));
        }
      } else if constexpr (MAG) {
        const float h = hypotf(xv[k].x, xv[k].y);
        const float ux = h > 0.0f ? xv[k].x / h : 1.0f, uy = h > 0.0f ? xv[k].y / h : 0.0f;
        va = (float)((double)ux * ar[k] + (dc ? 0.0 : (double)uy) * ai[k]);
      } else {
        const double xr = (double)xv[k].x, xi = dc ? 0.0 : (double)xv[k].y;
        va = (float)(xr * ar[k] + xi * ai[k]);
        if constexpr (PAIR) vb = (float)(xr * br[k] + xi * bi[k]);
      }
      if (PAIR && v2) {
        *reinterpret_cast<float2*>(oa + 2 * f) = make_float2(va, vb);
      } else {
        oa[(long)f * C + c0] = va;
        if (PAIR && has_b) oa[(long)f * C + c1] = vb;
      }
    }
    if (lane < 2 && (lane == 0 || has_b)) {            // Z[N/2] = FFT(g_c0)[N/2] + i FFT(g_c1)[N/2], both real: lane 0 -> c0, lane 1 -> c1
      const double g = lane ? im[fft_idx(N / 2)] : re[fft_idx(N / 2)];
      float v;
      if constexpr (PHASE) {
        const double mag = (double)hypotf(xnyq_re, xnyq_im);
        v = (float)(mag * ((double)(lane ? pbnyq : panyq) * g));
        *reinterpret_cast<float2*>((lane ? qb : qa) + 2 * (N / 2)) = make_float2((float)((double)(lane ? mbnyq : manyq) * mag * g), 0.0f);
      } else if constexpr (MAG) {
        const float h = hypotf(xnyq_re, xnyq_im);
        v = (float)((double)(h > 0.0f ? xnyq_re / h : 1.0f) * g);
      } else {
        v = (float)((double)xnyq_re * g);
      }
      oa[(long)(N / 2) * C + (lane ? c1 : c0)] = v;
    }
    __builtin_amdgcn_wave_barrier();   // the next frame overwrites the buffer
  }
}

// g_out (B, C, length) contiguous; g_operand (B, T, F, C) contiguous; g_phase (C, B, T, F, 2) contiguous (PHASE only).
static int istft_backward_impl(const float* stft_ri, const float* operand, int64_t m_sb, int64_t m_sc, int64_t m_st, int64_t m_sf,
                               const float* phase, int64_t p_sc, int mode, int B, int C, int T, const int32_t* frames, int n_fft,
                               int hop, int length, const int32_t* lengths, const float* g_out, float* g_operand, float* g_phase,
                               void* stream) {
  if (mode != ISTFT_MASK && mode != ISTFT_PHASE && mode != ISTFT_MAG) return ONSSEN_E_ARG;
  if (!stft_ri || !g_out || !g_operand || B < 1 || C < 1 || T < 1 || hop < 1 || hop > n_fft || length < 1) return ONSSEN_E_ARG;
  if (n_fft != 256 && n_fft != 512 && n_fft != 1024) return ONSSEN_E_ARG;
  if ((frames == nullptr) != (lengths == nullptr)) return ONSSEN_E_ARG;
  if (mode == ISTFT_PHASE && (!operand || !phase || !g_phase)) return ONSSEN_E_ARG;
  if (reinterpret_cast<uintptr_t>(stft_ri) & 7u) return ONSSEN_E_ALIGN;               // (re, im) pairs are read as one 8-byte word
  if (mode == ISTFT_PHASE &&
      ((reinterpret_cast<uintptr_t>(phase) & 7u) || (p_sc & 1) || (reinterpret_cast<uintptr_t>(g_phase) & 7u)))
    return ONSSEN_E_ALIGN;
  ONSSEN_CLEAR_ERROR();
  const bool pair = mode != ISTFT_MAG;
  const int ny = pair ? ceil_div(C, 2) : C;
  // one wave per frame and speaker pair, `fpw` consecutive frames per wave (the per-lane constants are built once per wave, the
  // next frame's samples are fetched under this frame's butterflies); fewer frames per wave when that leaves CUs without a workgroup
  int fpw = 4;
  while (fpw > 1 && (long)B * ny * ceil_div(T, 4 * fpw) < 512) --fpw;
  const dim3 grid((unsigned)((long)B * ceil_div(T, 4 * fpw)), (unsigned)ny), block(256);
  const int v2 = C == 2 && (reinterpret_cast<uintptr_t>(g_operand) & 7u) == 0;
  hipStream_t st = (hipStream_t)stream;
#define ONSSEN_ISTFT_BWD(N_, PAIR_, MODE_)                                                                                      \
  hipLaunchKernelGGL((istft_bwd_kernel<N_, PAIR_, MODE_>), grid, block, 0, st, stft_ri, operand, (long)m_sb, (long)m_sc,       \
                     (long)m_st, (long)m_sf, phase, (long)p_sc, B, C, T, hop, length, fpw, frames, lengths, g_out, g_operand,  \
                     g_phase, v2)
#define ONSSEN_ISTFT_BWD_N(N_)                                                                                                  \
  do {                                                                                                                          \
    if (mode == ISTFT_MASK) ONSSEN_ISTFT_BWD(N_, true, ISTFT_MASK);                                                             \
    else if (mode == ISTFT_PHASE) ONSSEN_ISTFT_BWD(N_, true, ISTFT_PHASE);                                                      \
    else ONSSEN_ISTFT_BWD(N_, false, ISTFT_MAG);                                                                                \
  } while (0)
  if (n_fft == 256) ONSSEN_ISTFT_BWD_N(256);
  else if (n_fft == 512) ONSSEN_ISTFT_BWD_N(512);
  else ONSSEN_ISTFT_BWD_N(1024);
#undef ONSSEN_ISTFT_BWD_N
#undef ONSSEN_ISTFT_BWD
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}
