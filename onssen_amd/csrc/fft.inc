// K1+K2 / K10: FFT helpers, STFT + log-magnitude, mask-apply + iSTFT (part of onssen_hip.hip).
// =================================================================================================
// K1+K2 / K10: fp64 FFT helpers.  One wavefront transforms one frame in its own LDS buffer: radix-4
// decimation-in-time stages (N = 4^k, or two half-size transforms + one radix-2 stage for N = 2*4^k), twiddles and
// the Hann window from a constant table, and NO workgroup barrier: a wave's LDS operations execute in order, so
// the stages of a frame only need the compiler to keep them in order.
// =================================================================================================
#include "fft_tables.inc"

template <int N>
struct FftPlan {
  static constexpr bool kOdd = (N == 512 || N == 128 || N == 2048);   // N = 2 * 4^k
  static constexpr int M = kOdd ? N / 2 : N;                           // radix-4 transform length
  static constexpr int DIG = M == 64 ? 3 : M == 256 ? 4 : M == 1024 ? 5 : 0;
  static_assert(DIG != 0, "FFT length must be 4^k or 2*4^k with 64 <= 4^k <= 1024");
};

// LDS position of input sample n so that the in-place stages below end in natural order
template <int N>
__device__ __forceinline__ int fft_perm(int n) {
  using P = FftPlan<N>;
  const int m = P::kOdd ? (n >> 1) : n;
  int r = 0;
#pragma unroll
  for (int d = 0; d < P::DIG; ++d) r |= ((m >> (2 * d)) & 3) << (2 * (P::DIG - 1 - d));
  return (P::kOdd ? (n & 1) * P::M : 0) + r;
}

// LDS position of logical element i: two doubles of padding per 16, so that the strided accesses of the first
// radix-4 stages (4 consecutive doubles every 16 / one double every 4) spread over all banks instead of 8
__device__ __forceinline__ int fft_idx(int i) { return i + ((i >> 4) << 1); }
template <int N>
constexpr int fft_buf_len() { return N + N / 8; }

template <int N>
__device__ __forceinline__ double fft_win(int i) { return 0.5 - 0.5 * kCos1024[i * (1024 / N)]; }   // periodic Hann

// Per-lane constants of the radix-4 stages when a wave holds exactly one butterfly per lane and stage (N / 4 == 64, i.e.
// N = 256, the wsj0-2mix transform): the three twiddles and the four LDS positions of every stage.  Round 2 fetched them
// from the global tables and recomputed the positions inside every stage of every transform -- ~18 vector loads with
// computed indices and ~100 integer instructions per transform, which is what these issue-bound kernels spent most of
// their instructions on; a wave now builds them once and reuses them for every frame it transforms (same table entries,
// same arithmetic: bit-identical results).
template <int N>
struct FftLaneConst {
  static constexpr int DIG = FftPlan<N>::DIG;
  double wr[DIG][3], wi[DIG][3];   // stage d >= 1: W^(q tk) for q = 1..3 (imaginary part without the direction's sign)
  int pos[DIG][4];                 // fft_idx of the butterfly's four elements
};
template <int N>
__device__ __forceinline__ void fft_lane_const(int lane, FftLaneConst<N>& c) {
  using P = FftPlan<N>;
  static_assert(N / 4 == 64 && !P::kOdd, "one butterfly per lane and stage");
#pragma unroll
  for (int d = 0; d < P::DIG; ++d) {
    const int Ls = 1 << (2 * d);
    const int j = lane & (Ls - 1), base = ((lane >> (2 * d)) << (2 * d + 2)) + j;
    const int tk = j * (1024 / (4 * Ls));
#pragma unroll
    for (int q = 0; q < 4; ++q) c.pos[d][q] = fft_idx(base + q * Ls);
#pragma unroll
    for (int q = 1; q < 4; ++q) {
      c.wr[d][q - 1] = d ? kCos1024[q * tk] : 1.0;
      c.wi[d][q - 1] = d ? kSin1024[q * tk] : 0.0;
    }
  }
}

// In-place FFT of the wave's frame (input at fft_perm positions, output in natural order).  inverse = conjugated
// twiddles, unscaled.  Every lane of the wave calls this.  `lc` = the lane's precomputed constants (N = 256) or null.
template <int N>
__device__ __forceinline__ void fft_wave(double* re, double* im, int lane, bool inverse, const FftLaneConst<N>* lc = nullptr) {
  using P = FftPlan<N>;
  constexpr int M = P::M;
  const double sg = inverse ? 1.0 : -1.0;   // sign of the imaginary part of the twiddles / of the +-i rotations
  if constexpr (N / 4 == 64 && !P::kOdd) {
    if (lc) {
#pragma unroll
      for (int d = 0; d < P::DIG; ++d) {
        __builtin_amdgcn_wave_barrier();
        double xr[4], xi[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double ar = re[lc->pos[d][q]], ai = im[lc->pos[d][q]];
          if (q == 0 || d == 0) {
            xr[q] = ar;
            xi[q] = ai;
          } else {
            const double wr = lc->wr[d][q - 1], wi = sg * lc->wi[d][q - 1];
            xr[q] = ar * wr - ai * wi;
            xi[q] = ar * wi + ai * wr;
          }
        }
        const double ar = xr[0] + xr[2], ai = xi[0] + xi[2], br = xr[0] - xr[2], bi = xi[0] - xi[2];
        const double cr = xr[1] + xr[3], ci = xi[1] + xi[3], dr = xr[1] - xr[3], di = xi[1] - xi[3];
        const int p0 = lc->pos[d][0], p1 = lc->pos[d][1], p2 = lc->pos[d][2], p3 = lc->pos[d][3];
        re[p0] = ar + cr;  im[p0] = ai + ci;
        re[p2] = ar - cr;  im[p2] = ai - ci;
        re[p1] = br - sg * di;  im[p1] = bi + sg * dr;
        re[p3] = br + sg * di;  im[p3] = bi - sg * dr;
      }
      __builtin_amdgcn_wave_barrier();
      return;
    }
  }
#pragma unroll
  for (int d = 0; d < P::DIG; ++d) {
    const int Ls = 1 << (2 * d);            // length of the four sub-transforms being combined
    __builtin_amdgcn_wave_barrier();
    for (int u = lane; u < N / 4; u += 64) {
      const int sub = u / (M / 4), v = u % (M / 4);
      const int j = v & (Ls - 1), base = sub * M + ((v >> (2 * d)) << (2 * d + 2)) + j;
      const int tk = j * (1024 / (4 * Ls));            // W_{4Ls}^j = table[tk]
      double xr[4], xi[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double ar = re[fft_idx(base + q * Ls)], ai = im[fft_idx(base + q * Ls)];
        if (q == 0 || d == 0) {
          xr[q] = ar;
          xi[q] = ai;
        } else {
          const double wr = kCos1024[q * tk], wi = sg * kSin1024[q * tk];
          xr[q] = ar * wr - ai * wi;
          xi[q] = ar * wi + ai * wr;
        }
      }
      // y0 = x0+x1+x2+x3, y1 = x0 + s*i*x1 - x2 - s*i*x3 (s = sg: -i forward), y2 = x0-x1+x2-x3, y3 = x0 - s*i*x1 - x2 + s*i*x3
      const double ar = xr[0] + xr[2], ai = xi[0] + xi[2], br = xr[0] - xr[2], bi = xi[0] - xi[2];
      const double cr = xr[1] + xr[3], ci = xi[1] + xi[3], dr = xr[1] - xr[3], di = xi[1] - xi[3];
      const int p0 = fft_idx(base), p1 = fft_idx(base + Ls), p2 = fft_idx(base + 2 * Ls), p3 = fft_idx(base + 3 * Ls);
      re[p0] = ar + cr;  im[p0] = ai + ci;
      re[p2] = ar - cr;  im[p2] = ai - ci;
      // s*i*(dr + i di) = s*(-di + i dr)
      re[p1] = br - sg * di;  im[p1] = bi + sg * dr;
      re[p3] = br + sg * di;  im[p3] = bi - sg * dr;
    }
  }
  if (P::kOdd) {   // X[k] = E[k] + W_N^k O[k], X[k + N/2] = E[k] - W_N^k O[k]
    __builtin_amdgcn_wave_barrier();
    for (int k = lane; k < N / 2; k += 64) {
      const double wr = kCos1024[k * (1024 / N)], wi = sg * kSin1024[k * (1024 / N)];
      const int pe = fft_idx(k), po = fft_idx(k + N / 2);
      const double er = re[pe], ei = im[pe], orr = re[po], oi = im[po];
      const double tr = orr * wr - oi * wi, ti = orr * wi + oi * wr;
      re[pe] = er + tr;  im[pe] = ei + ti;
      re[po] = er - tr;  im[po] = ei - ti;
    }
  }
  __builtin_amdgcn_wave_barrier();
}

#ifdef ONSSEN_FFT_PROFILE      // profile builds only (tools/fft_timeline.py): wave clocks at the phases of the STFT / iSTFT kernels
__device__ long long g_fft_stamps[4096 * 16];
#define ONSSEN_FFT_MARK(slot)                                                                      \
  do {                                                                                             \
    if (lane == 0 && fft_wid < 4096 && (slot) < 16) g_fft_stamps[fft_wid * 16 + (slot)] = (long long)__builtin_readcyclecounter(); \
  } while (0)
#else
#define ONSSEN_FFT_MARK(slot) do { } while (0)
#endif
// TWO frames per complex transform: frames 2p and 2p+1 of ONE utterance, a in the real part, b in the imaginary part; both
// are real signals, so
//   X_a[k] = (Z[k] + conj Z[N-k]) / 2,   X_b[k] = (Z[k] - conj Z[N-k]) / (2i)
// -- half the butterflies of one transform per frame.  grid = B x groups of 4 * ppw pairs; a wave transforms `ppw`
// consecutive pairs.  What bounded the round-2 form was neither the butterflies nor HBM but EIGHT SERIALISED global loads per
// pair (the optional frame b made every load its own basic block: load, wait, convert, store, next) and a 64-bit division
// per pair; here a pair's samples are fetched by one batch of independent loads -- the NEXT pair's batch is issued before
// this pair's transform -- and nothing in the loop divides.
template <int N>
__global__ __launch_bounds__(256) void stft_logmag_kernel(const float* __restrict__ wav, int n_samples, long wav_stride,
                                                          int hop, int T, float eps, int ppw,
                                                          float* __restrict__ logmag, float* __restrict__ stft_ri,
                                                          const int* __restrict__ n_per_utt) {
  __shared__ double buf_re[4][fft_buf_len<N>()], buf_im[4][fft_buf_len<N>()];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int F = N / 2 + 1;
  const int npair = (T + 1) >> 1;
  const int ngrp = (npair + 4 * ppw - 1) / (4 * ppw), utt = (int)blockIdx.x / ngrp, grp = (int)blockIdx.x - utt * ngrp;
  int p = (grp * 4 + wave) * ppw;
  const int pend = p + ppw < npair ? p + ppw : npair;
  if (p >= pend) return;                               // no workgroup-wide synchronisation anywhere in this kernel
  [[maybe_unused]] const int fft_wid = (int)blockIdx.x * 4 + wave;
  [[maybe_unused]] int fft_slot = 3;
  ONSSEN_FFT_MARK(0);
  double* re = buf_re[wave];
  double* im = buf_im[wave];
  const float* sig = wav + (long)utt * wav_stride;
  // ragged batch (n_per_utt): utterance `utt` has its own sample count -- its reflect padding mirrors about ITS last sample and
  // its own frames are 0 .. n / hop; the frames after them (up to the batch's T) are the transform of silence
  if (n_per_utt) n_samples = n_per_utt[utt];
  const int Tb = n_per_utt ? 1 + n_samples / hop : T;
  float* lm = logmag + (long)utt * T * F;
  float* ri = stft_ri ? stft_ri + (long)utt * T * F * 2 : nullptr;
  constexpr int SPL = N / 64;                          // samples per lane
  // centred frames, reflect padding (edge sample not repeated); an odd T's last pair reads frame T-1 twice and drops the copy
  float sa[SPL], sb[SPL];
  auto fetch = [&](int pr) {
    const int oa = 2 * pr * hop - N / 2, tb = 2 * pr + 1 < T ? 2 * pr + 1 : T - 1, ob = tb * hop - N / 2;
    if (oa >= 0 && ob + N <= n_samples) {              // wave-uniform: both frames inside the signal
#pragma unroll
      for (int k = 0; k < SPL; ++k) {
        sa[k] = sig[oa + lane + 64 * k];
        sb[k] = sig[ob + lane + 64 * k];
      }
    } else {
      const bool za = 2 * pr >= Tb, zb = tb >= Tb;      // (never in a uniform batch: Tb = T)
#pragma unroll
      for (int k = 0; k < SPL; ++k) {
        int pa = oa + lane + 64 * k, pb = ob + lane + 64 * k;
        pa = pa < 0 ? -pa : pa;
        pa = pa >= n_samples ? 2 * (n_samples - 1) - pa : pa;
        pb = pb < 0 ? -pb : pb;
        pb = pb >= n_samples ? 2 * (n_samples - 1) - pb : pb;
        sa[k] = za ? 0.0f : sig[za ? 0 : pa];
        sb[k] = zb ? 0.0f : sig[zb ? 0 : pb];
      }
    }
  };
  fetch(p);
  ONSSEN_FFT_MARK(2);
  // what does not depend on the frame: where a lane's samples go (bit-reversed position), their window weights, and -- one
  // butterfly per lane and stage, N = 256 -- the stage constants: built once per wave -- AFTER the first pair's samples
  // have been requested, so that the table loads and the sample loads are one round trip, not two.
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
  ONSSEN_FFT_MARK(1);
  for (; p < pend; ++p) {
    const int ta = 2 * p;
    const bool has_b = ta + 1 < T;
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
      re[jpos[k]] = (double)sa[k] * wwin[k];
      im[jpos[k]] = has_b ? (double)sb[k] * wwin[k] : 0.0;
    }
    ONSSEN_FFT_MARK(fft_slot); ++fft_slot;
    if (p + 1 < pend) fetch(p + 1);                    // lands under this pair's transform
    if constexpr (kLaneConst) fft_wave<N>(re, im, lane, false, &lcs); else fft_wave<N>(re, im, lane, false);
    ONSSEN_FFT_MARK(fft_slot); ++fft_slot;
    float* lma = lm + (long)ta * F;
    float* ria = ri ? ri + (long)ta * F * 2 : nullptr;
    // bins 0 .. N/2 - 1 (the Nyquist bin follows).  One straight-line body per case -- `has_b` is false only for the last pair
    // of an odd frame count -- so that the N/128 iterations' LDS reads, hypot / log10 sequences and stores interleave instead of
    // sitting in separate basic blocks
    auto outputs = [&](auto with_b) __attribute__((always_inline)) {
      constexpr bool WB = decltype(with_b)::value;
      float ar[N / 128], ai[N / 128], br[N / 128], bi[N / 128];
#pragma unroll
      for (int k = 0; k < N / 128; ++k) {
        const int f = lane + 64 * k, fn = (N - f) & (N - 1);
        const double zr = re[fft_idx(f)], zi = im[fft_idx(f)], nr = re[fft_idx(fn)], ni = im[fft_idx(fn)];
        // complex128 -> complex64 like the reference
        ar[k] = (float)(0.5 * (zr + nr)); ai[k] = (float)(0.5 * (zi - ni));
        br[k] = (float)(0.5 * (zi + ni)); bi[k] = (float)(0.5 * (nr - zr));
      }
#pragma unroll
      for (int k = 0; k < N / 128; ++k) {
        const int f = lane + 64 * k;
        lma[f] = log10f(hypotf(ar[k], ai[k]) + eps);
        if (ria) *reinterpret_cast<float2*>(ria + 2 * f) = make_float2(ar[k], ai[k]);
        if constexpr (WB) {
          lma[F + f] = log10f(hypotf(br[k], bi[k]) + eps);
          if (ria) *reinterpret_cast<float2*>(ria + 2 * (F + f)) = make_float2(br[k], bi[k]);
        }
      }
    };
    if (has_b) outputs(std::true_type{}); else outputs(std::false_type{});
    if (lane < 2 && (lane == 0 || has_b)) {            // Z[N/2] = X_a[N/2] + i X_b[N/2], both real: lane 0 -> frame a, lane 1 -> frame b
      const float v = (float)(lane ? im[fft_idx(N / 2)] : re[fft_idx(N / 2)]);
      lma[lane * F + N / 2] = log10f(fabsf(v) + eps);  // hypotf(v, 0) == |v|
      if (ria) *reinterpret_cast<float2*>(ria + 2 * (lane * F + N / 2)) = make_float2(v, 0.f);
    }
    ONSSEN_FFT_MARK(fft_slot); ++fft_slot;
    __builtin_amdgcn_wave_barrier();   // the next pair overwrites the buffer
  }
}

// FB = frames transformed per workgroup (FB/4 rounds of 4 waves); sized so that the LDS image
// (tables + 4 FFT buffers + FB windowed frames, all fp64) stays under 160 KiB.
// PAIR: two speakers per workgroup through ONE complex inverse FFT per frame: with Z = S_a + i S_b (both Hermitian),
// ifft(Z) = s_a + i s_b because s_a and s_b are real -- half the butterflies of two real transforms.  blockIdx.y then
// counts speaker pairs (the last pair of an odd C repeats its only speaker and drops the copy).
// PHASE (phase_net's reconstruction, onssen_phase_istft_f32): speaker c's operand at a bin is mask_c * |X| * (p_c.re, p_c.im) with
// the network's unit phase vector p_c instead of X * mask_c; p_c (B,T,F,2) sits at phase + c * p_sc.  |X| = hypotf(Re X, Im X) in
// float32, as the reference's np.abs of a complex64 spectrum; the phases ride in the same batch of loads as the masks.
// MAG (enhancement's reconstruction, onssen_mag_istft_f32): `mask` holds an estimated MAGNITUDE m and the operand at a bin is
// m * X / |X| -- that magnitude with the mixture's phase.  |X| = hypotf(Re X, Im X) and the two quotients are float32, the product
// with m is fp64 like PHASE's; a bin with X = 0 takes the unit vector (1, 0), as exp(i np.angle(0)) = 1.  Unpaired only (one
// estimate per input).
enum { ISTFT_MASK = 0, ISTFT_PHASE = 1, ISTFT_MAG = 2 };
__device__ const float kIstftOne = 1.0f;
template <int N, int FB, bool PAIR, int MODE>
__global__ __launch_bounds__(256) void mask_istft_kernel(const float* __restrict__ stft_ri,
                                                         const float* __restrict__ mask, long m_sb, long m_sc,
                                                         long m_st, long m_sf, int C, int T, int hop, int length,
                                                         int FR, float* __restrict__ out,
                                                         const int* __restrict__ frames, const int* __restrict__ lengths,
                                                         const float* __restrict__ phase, long p_sc) {
  constexpr bool PHASE = MODE == ISTFT_PHASE, MAG = MODE == ISTFT_MAG;
  static_assert(!(MAG && PAIR), "the magnitude form is unpaired");
  constexpr int NS = PAIR ? 2 : 1;
  __shared__ double buf_re[4][fft_buf_len<N>()], buf_im[4][fft_buf_len<N>()];
  __shared__ float fr[NS][FB][N];   // windowed time-domain frames of this chunk (the reference's istft keeps them in
                                    // float32 too); 50 KB per workgroup with the FFT buffers: three workgroups per CU
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int F = N / 2 + 1;
  const int chunk = blockIdx.x, b = blockIdx.z;
  // ragged batch: utterance b has Tb <= T frames of its own and len_b <= length output samples (zeros after them); the
  // spectrum and the output keep the batch's strides (T frames, `length` samples per row)
  const int Tb = frames ? frames[b] : T, len_b = lengths ? lengths[b] : length;
  const int c0 = PAIR ? 2 * (int)blockIdx.y : (int)blockIdx.y, c1 = (PAIR && c0 + 1 < C) ? c0 + 1 : c0;
  // output samples n in [chunk*FR*hop, +FR*hop); padded position p = n + N/2 is covered by frames
  // t with t*hop <= p < t*hop + N
  const int p0 = chunk * FR * hop + N / 2;
  int tfirst = (p0 - N + hop) / hop;  // ceil((p0 - N + 1) / hop) for p0 >= N/2 >= 1 ... clamp below
  if (p0 - N + 1 <= 0) tfirst = 0;
  const double inv_n = 1.0 / (double)N;
  constexpr int FPL = N / 128, SPL = N / 64;
  // a frame's operands: one batch of independent loads per round (round 2's form branched on `active` / `mask` / DC / Nyquist
  // around every single load and waited for each: nine serialised HBM round trips per frame), the next round's batch issued
  // before this round's transform.  A frame past the end reads frame T-1 and is zeroed by a select.
  float2 xv[FPL];
  float mav[FPL], mbv[FPL], xnyq, manyq, mbnyq;
  [[maybe_unused]] float2 pav[FPL], pbv[FPL];          // PHASE: the two speakers' phase vectors of this lane's bins
  [[maybe_unused]] float xnyq_im, panyq, pbnyq;        // PHASE: Im X[N/2] (for |X|; MAG too) and the real parts of the Nyquist phases
  auto fetch = [&](int round) {
    const int t = tfirst + round * 4 + wave, tt = t < Tb ? t : Tb - 1;
    const float* xs = stft_ri + ((long)b * T + tt) * F * 2;
#pragma unroll
    for (int k = 0; k < FPL; ++k) xv[k] = *reinterpret_cast<const float2*>(xs + 2 * (lane + 64 * k));
    xnyq = xs[N];                                        // Re X[N/2]
    // no mask: every mask load reads the same 1.0f (zero strides) -- selected with scalar arithmetic, not with a branch around
    // the loads (the compiler drains the load queue at such a branch's join)
    const float* ms0 = mask ? mask + (long)b * m_sb + (long)c0 * m_sc + (long)tt * m_st : &kIstftOne;
    const float* ms1 = mask ? mask + (long)b * m_sb + (long)c1 * m_sc + (long)tt * m_st : &kIstftOne;
    const long sf = mask ? m_sf : 0;
#pragma unroll
    for (int k = 0; k < FPL; ++k) {
      mav[k] = ms0[(long)(lane + 64 * k) * sf];
      mbv[k] = PAIR ? ms1[(long)(lane + 64 * k) * sf] : 0.f;
    }
    manyq = ms0[(long)(N / 2) * sf];
    mbnyq = PAIR ? ms1[(long)(N / 2) * sf] : 0.f;
    if constexpr (PHASE) {
      const float* pa = phase + (long)c0 * p_sc + ((long)b * T + tt) * F * 2;
      const float* pb = phase + (long)c1 * p_sc + ((long)b * T + tt) * F * 2;
#pragma unroll
      for (int k = 0; k < FPL; ++k) {
        pav[k] = *reinterpret_cast<const float2*>(pa + 2 * (lane + 64 * k));
        if constexpr (PAIR) pbv[k] = *reinterpret_cast<const float2*>(pb + 2 * (lane + 64 * k));
      }
      xnyq_im = xs[N + 1];
      panyq = pa[N];
      if constexpr (PAIR) pbnyq = pb[N];
    }
    if constexpr (MAG) xnyq_im = xs[N + 1];
  };
  fetch(0);                                            // (requested before the lane constants are built: their table loads and these are one round trip)
  constexpr bool kLaneConst = (N / 4 == 64) && !FftPlan<N>::kOdd;
  FftLaneConst<kLaneConst ? N : 256> lcs;              // stage constants of this lane, built once for the FB / 4 transforms of the wave
  if constexpr (kLaneConst) fft_lane_const<N>(lane, lcs);
  // LDS positions of bin f = lane + 64 k (f < N/2) and of its Hermitian mirror, and the output weights of this lane's
  // samples: the same for every frame
  int jf[FPL], jmir[FPL];
#pragma unroll
  for (int k = 0; k < FPL; ++k) {
    const int f = lane + 64 * k;
    jf[k] = fft_idx(fft_perm<N>(f));
    jmir[k] = fft_idx(fft_perm<N>(f > 0 ? N - f : 0));
  }
  const int jnyq = fft_idx(fft_perm<N>(N / 2));
  double wout[SPL];
#pragma unroll
  for (int k = 0; k < SPL; ++k) wout[k] = fft_win<N>(lane + 64 * k) * inv_n;
#pragma unroll 1
  for (int round = 0; round < FB / 4; ++round) {
    const int fidx = round * 4 + wave;
    const bool active = tfirst + fidx < Tb;
    double* re = buf_re[wave];
    double* im = buf_im[wave];
#pragma unroll
    for (int k = 0; k < FPL; ++k) {
      // S_a = X * m_a (and S_b = X * m_b); c2r transforms ignore the imaginary part of DC / Nyquist
      const bool dc = (k == 0 && lane == 0);
      double ar, ai, br, bi;
      if constexpr (PHASE) {         // S_c = m_c |X| p_c
        const double mag = active ? (double)hypotf(xv[k].x, xv[k].y) : 0.0;
        const double ma = mag * (double)mav[k], mb = PAIR ? mag * (double)mbv[k] : 0.0;
        ar = ma * (double)pav[k].x;
        ai = dc ? 0.0 : ma * (double)pav[k].y;
        br = PAIR ? mb * (double)pbv[k].x : 0.0;
        bi = (PAIR && !dc) ? mb * (double)pbv[k].y : 0.0;
      } else if constexpr (MAG) {    // S = m X / |X|
        const float h = hypotf(xv[k].x, xv[k].y);
        const float ux = h > 0.0f ? xv[k].x / h : 1.0f, uy = h > 0.0f ? xv[k].y / h : 0.0f;
        const double m = active ? (double)mav[k] : 0.0;
        ar = m * (double)ux;
        ai = dc ? 0.0 : m * (double)uy;
        br = 0.0; bi = 0.0;
      } else {
      const double xr = active ? (double)xv[k].x : 0.0, xi = (active && !dc) ? (double)xv[k].y : 0.0;
      const double ma = (double)mav[k], mb = (double)mbv[k];
      ar = xr * ma; ai = xi * ma; br = PAIR ? xr * mb : 0.0; bi = PAIR ? xi * mb : 0.0;
      }
      re[jf[k]] = ar - bi;           // Z[f] = S_a[f] + i S_b[f]
      im[jf[k]] = ai + br;
      if (!dc) {                     // Hermitian mirrors: Z[N-f] = conj(S_a[f]) + i conj(S_b[f])
        re[jmir[k]] = ar + bi;
        im[jmir[k]] = -ai + br;
      }
    }
    if (lane == 0) {
      if constexpr (PHASE) {
        const double mag = active ? (double)hypotf(xnyq, xnyq_im) : 0.0;
        re[jnyq] = mag * (double)manyq * (double)panyq;
        im[jnyq] = PAIR ? mag * (double)mbnyq * (double)pbnyq : 0.0;
      } else if constexpr (MAG) {
        const float h = hypotf(xnyq, xnyq_im);
        re[jnyq] = active ? (double)manyq * (double)(h > 0.0f ? xnyq / h : 1.0f) : 0.0;
        im[jnyq] = 0.0;
      } else {
      const double xr = active ? (double)xnyq : 0.0;
      re[jnyq] = xr * (double)manyq;
      im[jnyq] = PAIR ? xr * (double)mbnyq : 0.0;
      }
    }
    if (round + 1 < FB / 4) fetch(round + 1);          // lands under this round's transform
    if constexpr (kLaneConst) fft_wave<N>(re, im, lane, true, &lcs); else fft_wave<N>(re, im, lane, true);
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
      const int i = lane + 64 * k;
      const double w = active ? wout[k] : 0.0;
      fr[0][fidx][i] = (float)(w * re[fft_idx(i)]);
      if (PAIR) fr[1][fidx][i] = (float)(w * im[fft_idx(i)]);
    }
    __builtin_amdgcn_wave_barrier();   // the wave's next round overwrites its buffer
  }
  __syncthreads();
  const int exp_len = N + hop * (Tb - 1);
  for (int idx = tid; idx < FR * hop; idx += 256) {
    const int n = chunk * FR * hop + idx;
    if (n >= length) continue;
    const int pp = n + N / 2;
    double y0 = 0.0, y1 = 0.0;
    if (pp < exp_len && n < len_b) {
      int tlo = (pp - N + hop) / hop;
      if (pp - N + 1 <= 0) tlo = 0;
      int thi = pp / hop;
      if (thi > Tb - 1) thi = Tb - 1;
      double s0 = 0.0, s1 = 0.0, wss = 0.0;
      for (int t = tlo; t <= thi && t - tfirst < FB; ++t) {
        const int i = pp - t * hop;
        s0 += (double)fr[0][t - tfirst][i];
        if (PAIR) s1 += (double)fr[1][t - tfirst][i];
        const double w = fft_win<N>(i);
        wss += w * w;
      }
      // one fp64 division per sample for both speakers (s * (1 / wss) differs from s / wss by at most one fp64 ulp: nothing
      // of it survives the rounding to float32 below)
      const double rw = wss > 2.2250738585072014e-308 ? 1.0 / wss : 1.0;
      y0 = s0 * rw;
      y1 = s1 * rw;
    }
    out[((long)b * C + c0) * length + n] = (float)y0;
    if (PAIR && c1 != c0) out[((long)b * C + c1) * length + n] = (float)y1;
  }
}
