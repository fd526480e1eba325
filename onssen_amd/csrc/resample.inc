// Sample-rate conversion of the file loaders: the polyphase resampler (part of onssen_hip.hip).
// =================================================================================================
// scipy.signal.resample_poly(x, up, down) with its default window -- what the loaders called on the host for every file whose
// rate differs from the recipe's (48 kHz Edinburgh, 44.1 kHz DAPS) -- as one launch over a ragged batch:
//   up, down reduced by their gcd, M = max(up, down), half = 10 M; taps h[k], k = 0 .. 2 half:
//     g[k] = sinc((k - half) / M) I0(5 sqrt(1 - ((k - half) / half)^2)) / I0(5),   h = up g / sum g      (firwin(.., 1/M, kaiser 5))
//   n_out = ceil(n_in up / down),   y[m] = sum_n x[n] h[m down - n up + half]   over the n in [0, n_in) with a tap index in range
//   equal rates: the identity (half = 0, the one tap 1.0), as resample_poly returns a copy.
// Polyphase form: with c = m down + half, n_hi = c / up and phase p = c % up the sum is over j = 0 .. L - 1 of
//   x[n_hi - j] img[p][j],   img[p][j] = h[p + j up] (0 beyond 2 half),   L = ceil((2 half + 1) / up)
// so the workspace holds the taps PHASE-MAJOR (up rows of Ls fp64 values; Ls = L, rounded up to an even count when up > 1 so that
// every row is 16-byte aligned, the pad a zero tap): one output reads its taps contiguously, two per load.  The taps are computed
// on the host in fp64 (own I0 series; the sine's argument is reduced in integers) and copied over once per ratio.
//   resample_kernel<true, UP1>   one workgroup per (tile of outputs, row): the tile's input span goes into the LDS once, as fp64,
//                                with `sub` already subtracted (the noise = noisy - clean row of the Edinburgh recipe in the same
//                                pass) and zeros outside [0, lengths_in[b]).  The tile is `per` <= 4 BANDS of `band` outputs,
//                                band a multiple of up: outputs m and m + band have the same phase, so thread t takes outputs
//                                t, t + band, .. of the tile and loads every tap ONCE for all of them (the phase rows are
//                                scattered over the image: a lane's tap load is a cache line of its own) -- four independent
//                                fp64 chains per lane, each output's own sum in order of j.  The workgroup has `band` threads
//                                rounded up to whole waves (44.1 -> 16 kHz: band 320 = 2 x 160, five waves, tile 1280).
//                                UP1 (up = 1: 48 -> 16 kHz): one phase, every lane reads the same tap -- a uniform load
//   resample_kernel<false, .>    the same sum, one output at a time, with the inputs read where they are: ratios whose taps do
//                                not fit the staged span (down / up above ~60: one output then reads thousands of inputs), or
//                                whose band does not fit a workgroup (up > 1024)
// Products and sum fp64 in a fixed order, ONE rounding to fp32 at the store; no atomics; an output depends on its row's samples and
// on nothing else (not on B, the other rows, the strides): a row is bit for bit its batch-1 result.  Index arithmetic on m down and
// n up is 64-bit (five minutes at 44.1 kHz: m 441 > 2^31).  Nothing beyond lengths_in[b] is read; y[b] is written up to stride_out
// (zeros from lengths_out[b] on: the ragged STFT behind it reads clean padding).
// =================================================================================================
namespace rsmp {
constexpr int MAXM = 2048;       // largest reduced up or down (every pair among 8 .. 96 kHz needs 1280 at the most)
constexpr int SPAN = 4096;       // fp64 input samples a workgroup stages: 32 KB of the CU's 160 KB -> 5 workgroups per CU
constexpr int PER = 4;           // outputs a thread accumulates side by side, at the most
struct Geo {
  int up, down, half, L, Ls;       // L taps per output; Ls: the image's row stride
  int band, per, tile, threads;    // staged: tile = per bands of `band` outputs; `threads` = band rounded up to whole waves
  bool staged;
};
}  // namespace rsmp

// Reduced ratio, filter geometry and the tile of one launch; false: a ratio the library refuses.
static bool resample_geo(int up, int down, rsmp::Geo* g) {
  using namespace rsmp;
  if (up < 1 || down < 1) return false;
  int a = up, b = down;
  while (b) { const int t = a % b; a = b; b = t; }
  up /= a; down /= a;
  const int M = up > down ? up : down;
  if (M > MAXM) return false;
  g->up = up; g->down = down;
  g->half = M == 1 ? 0 : 10 * M;
  g->L = 2 * g->half / up + 1;                                       // ceil((2 half + 1) / up)
  g->Ls = up == 1 ? g->L : g->L + (g->L & 1);
  // a tile of t outputs reads at most ceil((t - 1) down / up) + Ls + 1 consecutive inputs: t_max of them fit the span
  const long t_max = SPAN - g->Ls - 2 > 0 ? (long)(SPAN - g->Ls - 2) * up / down : 0;
  long k = (256 + up / 2) / up;                                      // a band of about 256 outputs, a multiple of up
  if (k < 1) k = 1;
  if (k * up > t_max) k = t_max / up;
  g->band = (int)(k * up);
  g->per = g->band > 0 ? (int)(t_max / g->band < PER ? t_max / g->band : PER) : 0;
  g->staged = g->band > 0 && g->band <= 1024 && (long)g->band * g->per >= 64;
  if (!g->staged) { g->band = 256; g->per = 1; }
  g->tile = g->band * g->per;
  g->threads = g->staged ? (g->band + 63) / 64 * 64 : 256;
  return true;
}

// I0(x) = sum_k ((x / 2)^k / k!)^2: the terms fall below 2^-53 of the sum after ~20 of them at x <= 5
static double resample_i0(double x) {
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 64; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < 1e-20 * sum) break;
  }
  return sum;
}

// h[0 .. 2 half] of a REDUCED ratio (g from resample_geo)
static void resample_taps(const rsmp::Geo& g, double* h) {
  if (g.half == 0) { h[0] = 1.0; return; }
  const int M = g.up > g.down ? g.up : g.down, half = g.half;
  const double i0b = resample_i0(5.0);
  double sum = 0.0;
  for (int k = 0; k <= 2 * half; ++k) {
    const int j = k - half;
    double s = 1.0;                                                  // sinc(j / M) = sin(pi j / M) / (pi j / M)
    if (j != 0) {
      int r = (j < 0 ? -j : j) % (2 * M);                            // sin(pi j / M) is odd and 2 M-periodic in j: sinc is even
      double sign = 1.0;
      if (r >= M) { r -= M; sign = -1.0; }
      if (2 * r > M) r = M - r;                                      // sin(pi - a) = sin(a): the argument ends in [0, pi / 2]
      s = sign * sin(M_PI * (double)r / (double)M) / (M_PI * (double)(j < 0 ? -j : j) / (double)M);
    }
    const double u = (double)j / (double)half;
    const double rad = 1.0 - u * u;
    h[k] = s * resample_i0(5.0 * sqrt(rad > 0.0 ? rad : 0.0)) / i0b;
    sum += h[k];
  }
  for (int k = 0; k <= 2 * half; ++k) h[k] = (double)g.up * h[k] / sum;
}

template <bool STAGED, bool UP1>
__global__ __launch_bounds__(1024) void resample_kernel(const float* __restrict__ x, const float* __restrict__ sub, long stride_in,
                                                        const int* __restrict__ lengths_in, int n_in, int up, int down, int half, int Ls,
                                                        int band, int per, const double* __restrict__ img, float* __restrict__ y,
                                                        long stride_out, int* __restrict__ lengths_out) {
  using namespace rsmp;
  __shared__ double span[STAGED ? SPAN : 1];
  const int tid = threadIdx.x, nthr = blockDim.x, b = blockIdx.y, tile = band * per;
  int nb = lengths_in ? lengths_in[b] : n_in;
  nb = nb < 0 ? 0 : nb > n_in ? n_in : nb;                           // (a device-side length is input: never past the row the host sized)
  const long n_out = ((long)nb * up + down - 1) / down;
  if (blockIdx.x == 0 && tid == 0 && lengths_out) lengths_out[b] = (int)n_out;
  const long m0 = (long)blockIdx.x * tile;
  const long m1 = m0 + tile < stride_out ? m0 + tile : stride_out;   // this workgroup writes y[b][m0 .. m1)
  const long mv = m1 < n_out ? m1 : n_out;                           // ... of which [m0, mv) are samples, the rest padding
  const float* xr = x + (long)b * stride_in;
  const float* sr = sub ? sub + (long)b * stride_in : nullptr;
  float* yr = y + (long)b * stride_out;
  if constexpr (STAGED) {
    const long n_lo = (m0 * down + half) / up - (Ls - 1);
    if (mv > m0) {                                                   // (uniform over the workgroup)
      const long n_top = ((mv - 1) * down + half) / up;
      const int cnt = (int)(n_top - n_lo + 1);                       // <= SPAN by the host's choice of the tile
      for (int s = tid; s < cnt && s < SPAN; s += nthr) {
        const long n = n_lo + s;
        double v = 0.0;
        if (n >= 0 && n < nb) {
          v = (double)xr[n];
          if (sr) v -= (double)sr[n];
        }
        span[s] = v;
      }
    }
    __syncthreads();
    if (tid >= band) return;                                         // (the lanes that round the band up to whole waves)
    double acc[PER];
    const double* sp[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const long m = m0 + tid + (long)band * i;
      const long c = (i < per && m < mv ? m : m0) * down + half;     // (a slot without an output walks the tile's first one: in range)
      sp[i] = span + (c / up - n_lo);
      acc[i] = 0.0;
    }
    if (mv > m0) {
      if constexpr (UP1) {
        for (int j = 0; j < Ls; ++j) {
          const double t = img[j];
#pragma unroll
          for (int i = 0; i < PER; ++i) acc[i] += sp[i][-j] * t;
        }
      } else {
        const long c = (m0 + tid < mv ? m0 + tid : m0) * down + half;
        const double* tp = img + (c % up) * Ls;                      // the phase of ALL this thread's outputs: its taps, contiguous
        for (int j = 0; j < Ls; j += 2) {                            // (Ls is even and the rows 16-byte aligned when up > 1)
          const double2 t = *reinterpret_cast<const double2*>(tp + j);
#pragma unroll
          for (int i = 0; i < PER; ++i) {
            acc[i] += sp[i][-j] * t.x;
            acc[i] += sp[i][-j - 1] * t.y;
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const long m = m0 + tid + (long)band * i;
      if (i < per && m < m1) yr[m] = m < mv ? (float)acc[i] : 0.0f;
    }
  } else {
    for (long m = m0 + tid; m < m1; m += nthr) {
      float out = 0.0f;
      if (m < n_out) {
        const long c = m * down + half;
        const long nh = c / up;
        const double* tp = img + (c - nh * up) * Ls;
        double acc = 0.0;
        for (int j = 0; j < Ls; ++j) {
          const long n = nh - j;
          if (n >= 0 && n < nb) {
            double v = (double)xr[n];
            if (sr) v -= (double)sr[n];
            acc += v * tp[j];
          }
        }
        out = (float)acc;
      }
      yr[m] = out;
    }
  }
}

extern "C" {

int onssen_resample_geometry(int rate_in, int rate_out, int64_t n_in, int* up, int* down, int* half, int64_t* n_out) {
  rsmp::Geo g;
  if (n_in < 0 || !resample_geo(rate_out, rate_in, &g)) return ONSSEN_E_ARG;
  if (up) *up = g.up;
  if (down) *down = g.down;
  if (half) *half = g.half;
  if (n_out) *n_out = (n_in * g.up + g.down - 1) / g.down;
  return ONSSEN_OK;
}

int onssen_resample_taps_f64(int up, int down, double* taps_host) {
  rsmp::Geo g;
  if (!taps_host || !resample_geo(up, down, &g)) return ONSSEN_E_ARG;
  resample_taps(g, taps_host);
  return ONSSEN_OK;
}

size_t onssen_resample_workspace_bytes(int up, int down) {
  rsmp::Geo g;
  return resample_geo(up, down, &g) ? (size_t)g.up * g.Ls * sizeof(double) : 0;
}

int onssen_resample_prepare(int up, int down, void* ws, size_t ws_bytes, void* stream) {
  rsmp::Geo g;
  if (!ws || !resample_geo(up, down, &g) || ws_bytes < onssen_resample_workspace_bytes(up, down)) return ONSSEN_E_ARG;
  if (reinterpret_cast<uintptr_t>(ws) & 15u) return ONSSEN_E_ALIGN;
  (void)stream;                                    // a blocking copy: whatever is launched after this call sees the image
  const size_t n = (size_t)g.up * g.Ls;
  double* h = (double*)malloc((2 * (size_t)g.half + 1 + n) * sizeof(double));
  if (!h) return ONSSEN_E_ARG;
  double* img = h + 2 * g.half + 1;
  resample_taps(g, h);
  for (int p = 0; p < g.up; ++p)
    for (int j = 0; j < g.Ls; ++j) {
      const long k = p + (long)j * g.up;
      img[(size_t)p * g.Ls + j] = k <= 2L * g.half ? h[k] : 0.0;
    }
  ONSSEN_CLEAR_ERROR();
#ifdef ONSSEN_HOST_EMULATION
  memcpy(ws, img, n * sizeof(double));             // (the mock runtime's "device" memory is host memory)
  const hipError_t e = hipSuccess;
#else
  const hipError_t e = hipMemcpy(ws, img, n * sizeof(double), hipMemcpyHostToDevice);
#endif
  free(h);
  return e == hipSuccess ? ONSSEN_OK : (int)e;
}

int onssen_resample_f32(const float* x, const float* sub, int64_t stride_in, const int32_t* lengths_in, int B, int n_in, int up,
                        int down, float* y, int64_t stride_out, int32_t* lengths_out, const void* ws, size_t ws_bytes, void* stream) {
  rsmp::Geo g;
  if (!x || !y || !ws || B <= 0 || B > 65535 || n_in <= 0 || stride_in < n_in || !resample_geo(up, down, &g)) return ONSSEN_E_ARG;
  const int64_t n_out = ((int64_t)n_in * g.up + g.down - 1) / g.down;
  if (n_out > 0x7fffffffLL || stride_out < n_out || ws_bytes < onssen_resample_workspace_bytes(up, down)) return ONSSEN_E_ARG;
  const int64_t tiles = (stride_out + g.tile - 1) / g.tile;
  if (tiles > 0x7fffffffLL) return ONSSEN_E_ARG;
  if (reinterpret_cast<uintptr_t>(ws) & 15u) return ONSSEN_E_ALIGN;      // the taps are read two at a time
  ONSSEN_CLEAR_ERROR();
  const dim3 grid((unsigned)tiles, (unsigned)B);
#define ONSSEN_RESAMPLE(STAGED_, UP1_)                                                                                              \
  hipLaunchKernelGGL((resample_kernel<STAGED_, UP1_>), grid, dim3((unsigned)g.threads), 0, (hipStream_t)stream, x, sub,            \
                     (long)stride_in, (const int*)lengths_in, n_in, g.up, g.down, g.half, g.Ls, g.band, g.per, (const double*)ws, y, \
                     (long)stride_out, (int*)lengths_out)
  if (!g.staged) ONSSEN_RESAMPLE(false, false);
  else if (g.up == 1) ONSSEN_RESAMPLE(true, true);
  else ONSSEN_RESAMPLE(true, false);
#undef ONSSEN_RESAMPLE
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

}  // extern "C"
