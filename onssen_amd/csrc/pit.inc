// What the time-domain permutation-invariant losses (batch_sdr.inc, loss_sisnr.inc, loss_wa.inc) share (part of onssen_hip.hip;
// included before every loss file): row-chunk geometry, 4-float loads and stores, the scan order of the assignments, fixed-order
// fp64 sums, launch dispatchers, the workspace layout.  Theirs stay the accumulation, the table, the compare rule, the gradient.
// Not users: loss_upit.inc (its own load4; its scan decodes every index with upit::perm_nibbles) and tas_stitch_perm_kernel
// (tasnet_stitch.inc: 64 window pairs lane-parallel over base-4 codes, with its own silent-overlap tie rule).
namespace pit {
constexpr int CMAX = 4;                         // speakers at most
constexpr int NCH = 64;                         // chunks of a row at most

// ---- row geometry: a row's chunking depends on its own length only --------------------------------------------------------
// samples one workgroup takes of a row of len samples (a multiple of 4, chmin at least)
__host__ __device__ inline int chunk_len(int len, int chmin) {
  const int per = ((len + NCH - 1) / NCH + 3) & ~3;
  return per < chmin ? chmin : per;
}
__device__ __forceinline__ int row_len(const int* lengths, int b, int n) {
  const int l = lengths ? lengths[b] : n;
  return l < 1 ? 1 : l > n ? n : l;               // a device-side length cannot be refused by the host: it is clamped
}
// chunks of the longest possible row; a shorter row has no more of them (chunk_len)
static inline int chunks(int n, int chmin) { return n >= NCH * chmin ? NCH : ceil_div(n, chmin); }
// of the four samples from t, those inside the row's length
__device__ __forceinline__ int inside4(int len, long t) { return len - t >= 4 ? 4 : len - t > 0 ? (int)(len - t) : 0; }

// four consecutive floats from p + t (nv of them exist, the others read as 0): one 16-byte load where vec allows it -- the same
// samples in the same order either way.  (A template constant passed as vec folds.)
__device__ __forceinline__ void load4(const float* __restrict__ p, int t, int nv, bool vec, float (&v)[4]) {
  if (vec && nv == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p + t);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = j < nv ? p[t + j] : 0.0f;
  }
}
// the four floats o to out + t of a row of n: one 16-byte store where vec says that every such group is whole and aligned
__device__ __forceinline__ void store4(float* __restrict__ out, long t, int n, bool vec, const float (&o)[4]) {
  if (vec) {
    *reinterpret_cast<float4*>(out + t) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (t + e < n) out[t + e] = o[e];
  }
}

// ---- the K! assignments in lexicographic order, the order of itertools.permutations(range(K)) ------------------------------
// Starts at the identity; next() steps and returns false after the last; p(q): the reference of estimate q; idx: the running
// index.  Nibbles of one register (upit::perm_nibbles' format), so no run-time-indexed private array.  A scan is
//   Perms e(K); do { v = sum over q ascending of table[q][e.p(q)]; its own compare } while (e.next());
struct Perms {
  unsigned word;
  int K, idx;
  __device__ explicit Perms(int K_) : word(0x3210u), K(K_), idx(0) {}
  __device__ int p(int q) const { return (int)((word >> (4 * q)) & 15u); }
  __device__ void swap(int a, int c) { const unsigned d = ((word >> (4 * a)) ^ (word >> (4 * c))) & 15u; word ^= (d << (4 * a)) | (d << (4 * c)); }
  __device__ bool next() {
    ++idx;
    int a = K - 2;                                   // next lexicographic permutation
    while (a >= 0 && p(a) > p(a + 1)) --a;
    if (a < 0) return false;
    int c = K - 1;
    while (p(c) < p(a)) --c;
    swap(a, c);
    for (int l = a + 1, r = K - 1; l < r; ++l, --r) swap(l, r);
    return true;
  }
};

// ---- fp64 sums in a fixed order --------------------------------------------------------------------------------------------
// the wave's sum of v into red[wave][slot]; after a __syncthreads(), block_sum(red, slot) is the workgroup's (four waves)
template <int NS>
__device__ __forceinline__ void wave_put(double (&red)[4][NS], int slot, double v) {
  v = wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][slot] = v;
}
template <int NS>
__device__ __forceinline__ double block_sum(const double (&red)[4][NS], int slot) {
  return (red[0][slot] + red[1][slot]) + (red[2][slot] + red[3][slot]);
}
// what a row's value weighs in the backward pass: w_b = g_value[b] + sign g_total / N (device data, either may be absent)
__device__ __forceinline__ double row_weight(const float* g_value, const float* g_total, int b, int N, double sign) {
  return (g_value ? (double)g_value[b] : 0.0) + sign * (g_total ? (double)g_total[0] / (double)N : 0.0);
}
}  // namespace pit

// total = sign * sum_b vals[b] / N, a fixed-order sum over the rows (sign * s is exact: -1 for a loss of a score, +1 for a distance)
__global__ __launch_bounds__(64) void pit_total_kernel(const double* __restrict__ vals, int N, double sign, float* __restrict__ total) {
  double s = 0.0;
  for (int b = threadIdx.x; b < N; b += 64) s += vals[b];
  s = wave_sum_d(s);
  if (threadIdx.x == 0) total[0] = (float)(sign * s / (double)N);
}

// ---- host side -------------------------------------------------------------------------------------------------------------
namespace pit {
// f(std::integral_constant<int, k>{}) for a run-time k in 1 .. CMAX, f(std::bool_constant{}...) for run-time flags: the callers'
// generic lambdas name their kernel's instantiation with decltype(K)::value
template <class F>
static void with_k(int k, F&& f) {
  switch (k) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
  }
}
template <class F>
static void with_flag(bool a, F&& f) { a ? f(std::true_type{}) : f(std::false_type{}); }
template <class F>
static void with_flags(bool a, bool b, F&& f) { with_flag(a, [&](auto A) { with_flag(b, [&](auto B) { f(A, B); }); }); }

// The workspace of a chunked loss over N rows:  partial (N x NCH x nm fp64) | vals (N fp64) | extra (N x nx fp64) | pj (N x CMAX int)
struct Ws { double *partial, *vals, *extra; int* pj; };
static size_t ws_bytes(int N, int nm, int nx) {
  return ((size_t)N * NCH * nm + (size_t)N + (size_t)N * nx) * sizeof(double) + (size_t)N * CMAX * sizeof(int32_t);
}
static int carve(void* ws, size_t bytes, int N, int nm, int nx, Ws* w) {
  if (bytes < ws_bytes(N, nm, nx)) return ONSSEN_E_WORKSPACE;
  if ((reinterpret_cast<uintptr_t>(ws) & 7u) != 0) return ONSSEN_E_ALIGN;
  w->partial = (double*)ws;
  w->vals = w->partial + (size_t)N * NCH * nm;
  w->extra = w->vals + N;
  w->pj = (int*)(w->extra + (size_t)N * nx);
  return ONSSEN_OK;
}
}  // namespace pit
