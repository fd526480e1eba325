// MISI half-step (part of onssen_hip.hip): from the mixture and C time-domain estimates to the C phase maps of the next
// reconstruction, in one launch.
// =================================================================================================
// Multiple input spectrogram inversion (Gunawan & Sen 2010; Wang, Le Roux, Wang, Hershey 2018) alternates two projections:
// the inverse transform of  magnitude_c * phase_c  (mask_istft_kernel's PHASE mode), and -- this kernel -- the step back:
//   d[n]   = (x[n] - sum_j s_j[n]) / C        the mixture's residual, spread evenly so that the estimates sum to the mixture
//   u_c[n] = s_c[n] + d[n]
//   p_c    = Z_c / |Z_c|,  Z_c = STFT(u_c)    only the phase is kept
// The operand is formed on load in fp64 (sum in index order), no intermediate waveform is written, the transform is fft.inc's
// (fp64 in LDS, one wave per frame, no workgroup barrier), and the quotient is taken in fp64 and rounded once.
//
// A wave transforms frame t of TWO speakers in one complex FFT (u_c0 in the real part, u_c1 in the imaginary part; both are real
// signals, so X_a[k] = (Z[k] + conj Z[N-k]) / 2, X_b[k] = (Z[k] - conj Z[N-k]) / (2i): stft_logmag_kernel's trick for two frames);
// blockIdx.y counts speaker pairs, the last pair of an odd C repeats its only speaker and drops the copy.  A wave takes `fpw`
// consecutive frames of one utterance: a frame's samples are one batch of independent loads, and the next frame's batch is
// issued before this frame's transform.
// CT = how many estimates a lane fetches per sample (2, 4 or 8 >= C): the ones past C - 1 read estimate C - 1 again (a cache
// hit) and enter the sum as 0.0, so that the loads of a batch need no branch.  CT = 2 is C = 2: the pair is the whole sum.
// Output: unit vectors (re, im), float32, (C, B, T, F, 2) -- what mask_istft_kernel's PHASE mode reads with p_sc = B T F 2;
// (1, 0) where Z = 0 (np.angle(0) = 0, the MAG mode's convention), so also for every bin of a frame whose operand is all
// zero.  DC and Nyquist have a zero imaginary part by construction.
// Ragged batch (n_per_utt): row b mirrors about its own last sample, owns frames 0 .. n_b / hop, nothing is read beyond n_b, and
// the frames after its own (silence) get (1, 0) without a transform.
// =================================================================================================
template <int N, int CT>
__global__ __launch_bounds__(256) void misi_phase_kernel(const float* __restrict__ mix, long mix_stride,
                                                         const float* __restrict__ est, long est_sb, long est_sc, int B,
                                                         int C, int n_samples, int hop, int T, int fpw,
                                                         float* __restrict__ phase, const int* __restrict__ n_per_utt) {
  __shared__ double buf_re[4][fft_buf_len<N>()], buf_im[4][fft_buf_len<N>()];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int F = N / 2 + 1;
  const int ngrp = (T + 4 * fpw - 1) / (4 * fpw), utt = (int)blockIdx.x / ngrp, grp = (int)blockIdx.x - utt * ngrp;
  int t = (grp * 4 + wave) * fpw;
  const int tend = t + fpw < T ? t + fpw : T;
  if (t >= tend) return;                               // no workgroup-wide synchronisation anywhere in this kernel
  const int c0 = 2 * (int)blockIdx.y, c1 = c0 + 1 < C ? c0 + 1 : c0;
  double* re = buf_re[wave];
  double* im = buf_im[wave];
  if (n_per_utt) {                                     // (a device value cannot be refused by the host: kept inside the row)
    const int nb = n_per_utt[utt];
    n_samples = nb > n_samples ? n_samples : nb <= N / 2 ? N / 2 + 1 : nb;
  }
  const int Tb = n_per_utt ? 1 + n_samples / hop : T;
  const float* xs = mix + (long)utt * mix_stride;
  const float* es = est + (long)utt * est_sb;
  const float* ea = es + (long)c0 * est_sc;
  const float* eb = es + (long)c1 * est_sc;
  float* pa = phase + (((long)c0 * B + utt) * T) * F * 2;
  float* pb = phase + (((long)c1 * B + utt) * T) * F * 2;
  constexpr int SPL = N / 64;                          // samples per lane
  // centred frames, reflect padding (edge sample not repeated): ONE index per sample for the mixture and every estimate
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
  if (t < Tb) fetch(t);
  // what does not depend on the frame: where a lane's samples go (bit-reversed position), their window weights, and -- one
  // butterfly per lane and stage, N = 256 -- the stage constants; requested after the first frame's samples (one round trip)
  int jpos[SPL];
  double wwin[SPL];
#pragma unroll
  for (int k = 0; k < SPL; ++k) {
    jpos[k] = fft_idx(fft_perm<N>(lane + 64 * k));
    wwin[k] = fft_win<N>(lane + 64 * k);
  }
  constexpr bool kLaneConst = (N / 4 == 64) && !FftPlan<N>::kOdd;
  FftLaneConst<kLaneConst ? N : 256> lcs;
  if constexpr (kLaneConst) fft_lane_const<N>(lane, lcs);
  const double cd = (double)C;
  const bool has_b = c1 != c0;
  for (; t < tend; ++t) {
    float* pat = pa + (long)t * F * 2;
    float* pbt = pb + (long)t * F * 2;
    if (t >= Tb) {                                     // silence after the row's own frames: Z = 0
      for (int f = lane; f < F; f += 64) {
        *reinterpret_cast<float2*>(pat + 2 * f) = make_float2(1.f, 0.f);
        if (has_b) *reinterpret_cast<float2*>(pbt + 2 * f) = make_float2(1.f, 0.f);
      }
      continue;
    }
    // A silent operand (a speaker masked off: every u of the frame is 0) has Z = 0 exactly; sharing a transform with the other
    // speaker would leave it the rounding residue of that speaker's spectrum instead (~1e-16 of it, with a phase of its own), so
    // whether the frame's operands are zero is noted here and decides the output below.
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
    if (t + 1 < tend && t + 1 < Tb) fetch(t + 1);      // lands under this frame's transform
    if constexpr (kLaneConst) fft_wave<N>(re, im, lane, false, &lcs); else fft_wave<N>(re, im, lane, false);
    // bins 0 .. N/2 - 1 (the Nyquist bin follows): the LDS reads first, then the hypot / quotient sequences and the stores
    double ar[N / 128], ai[N / 128], br[N / 128], bi[N / 128];
#pragma unroll
    for (int k = 0; k < N / 128; ++k) {
      const int f = lane + 64 * k, fn = (N - f) & (N - 1);
      const double zr = re[fft_idx(f)], zi = im[fft_idx(f)], nr = re[fft_idx(fn)], ni = im[fft_idx(fn)];
      ar[k] = 0.5 * (zr + nr); ai[k] = 0.5 * (zi - ni);
      br[k] = 0.5 * (zi + ni); bi[k] = 0.5 * (nr - zr);
    }
#pragma unroll
    for (int k = 0; k < N / 128; ++k) {
      const int f = lane + 64 * k;
      const double ha = hypot(ar[k], ai[k]);
      *reinterpret_cast<float2*>(pat + 2 * f) = ha > 0.0 && !za ? make_float2((float)(ar[k] / ha), (float)(ai[k] / ha)) : make_float2(1.f, 0.f);
      if (has_b) {
        const double hb = hypot(br[k], bi[k]);
        *reinterpret_cast<float2*>(pbt + 2 * f) = hb > 0.0 && !zb ? make_float2((float)(br[k] / hb), (float)(bi[k] / hb)) : make_float2(1.f, 0.f);
      }
    }
    if (lane < 2 && (lane == 0 || has_b)) {            // Z[N/2] = X_a[N/2] + i X_b[N/2], both real: lane 0 -> speaker a, lane 1 -> b
      const double v = lane ? im[fft_idx(N / 2)] : re[fft_idx(N / 2)];
      *reinterpret_cast<float2*>((lane ? pbt : pat) + 2 * (N / 2)) = make_float2(v < 0.0 && !(lane ? zb : za) ? -1.f : 1.f, 0.f);
    }
    __builtin_amdgcn_wave_barrier();   // the next frame overwrites the buffer
  }
}

static int misi_phase_impl(const float* mix, int64_t mix_stride, const float* est, int64_t est_sb, int64_t est_sc, int B, int C,
                           int n_samples, int n_fft, int hop, float* phase, void* stream, const int32_t* n_per_utt) {
  if (!mix || !est || !phase || B <= 0 || C < 2 || C > 8 || hop <= 0 || hop > n_fft) return ONSSEN_E_ARG;
  if (n_fft != 256 && n_fft != 512 && n_fft != 1024) return ONSSEN_E_ARG;
  if (n_samples <= n_fft / 2) return ONSSEN_E_ARG;
  if (reinterpret_cast<uintptr_t>(phase) & 7u) return ONSSEN_E_ALIGN;                   // (re, im) pairs are stored as one 8-byte word
  ONSSEN_CLEAR_ERROR();
  const int T = 1 + n_samples / hop;
  // one wave per frame and speaker pair, `fpw` consecutive frames per wave (the lane constants are built once per wave, the next
  // frame's samples are fetched under this frame's butterflies); fewer frames per wave when that leaves CUs without a workgroup
  const int npair = ceil_div(C, 2);
  int fpw = 4;
  while (fpw > 1 && (long)B * npair * ceil_div(T, 4 * fpw) < 512) --fpw;
  const dim3 grid((unsigned)((long)B * ceil_div(T, 4 * fpw)), (unsigned)npair), block(256);
  hipStream_t st = (hipStream_t)stream;
#define ONSSEN_MISI(N_, CT_)                                                                                               \
  hipLaunchKernelGGL((misi_phase_kernel<N_, CT_>), grid, block, 0, st, mix, (long)mix_stride, est, (long)est_sb, (long)est_sc, \
                     B, C, n_samples, hop, T, fpw, phase, n_per_utt)
#define ONSSEN_MISI_N(N_)                                                                                                  \
  do {                                                                                                                     \
    if (C == 2) ONSSEN_MISI(N_, 2);                                                                                        \
    else if (C <= 4) ONSSEN_MISI(N_, 4);                                                                                   \
    else ONSSEN_MISI(N_, 8);                                                                                               \
  } while (0)
  if (n_fft == 256) ONSSEN_MISI_N(256);
  else if (n_fft == 512) ONSSEN_MISI_N(512);
  else ONSSEN_MISI_N(1024);
#undef ONSSEN_MISI_N
#undef ONSSEN_MISI
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}
