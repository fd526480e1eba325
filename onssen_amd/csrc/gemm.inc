// GEMM kernels: exact-fp32 MFMA, split-bf16 with fp32 A, split-bf16 over x3 images (part of onssen_hip.hip).
// =================================================================================================
// K3/K7/K8/K9: exact-fp32 MFMA GEMM  C = epi(A W^T + bias)
// =================================================================================================
namespace lin {
constexpr int BM = 128, BN = 80, BK = 16;
constexpr int LD = 20;              // LDS row stride (floats) of the staged A / W tiles: 16 + 4 pad
constexpr int CLD = 84;             // LDS row stride of the C tile in the epilogue
constexpr int STAGE = 2 * (BM + BN) * LD;
constexpr int SMEM = (BM * CLD > STAGE) ? BM * CLD : STAGE;
}  // namespace lin

struct LinearArgs {
  const float* A = nullptr;
  long a_s0 = 0, a_s1 = 0;
  const float* W = nullptr;
  const float* bias = nullptr;
  const float* resid = nullptr;
  float* C = nullptr;
  long c_s0 = 0, c_s1 = 0;
  int R = 1, M = 0, N = 0, K = 0, ldw = 0, group = 0;
  float eps = 0.f;
};

__device__ __forceinline__ float f4c(const float4& v, int r) {
  return r == 0 ? v.x : (r == 1 ? v.y : (r == 2 ? v.z : v.w));
}

template <bool A_VEC, int MODE>
__global__ __launch_bounds__(256) void linear_kernel(LinearArgs p) {
  using namespace lin;
  __shared__ __attribute__((aligned(16))) float smem[SMEM];
  __shared__ long c_rowoff[BM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * BN, m0 = blockIdx.y * BM;
  float* As = smem;
  float* Bs = smem + 2 * BM * LD;

  // ---- staging coordinates: thread -> (row, 4-wide k quad) of the A tile (2 rows) and W tile (<=2 rows)
  const int kq = tid & 3;
  long a_off[2];
  bool a_ok[2];
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int m = m0 + (tid >> 2) + 64 * it;
    a_ok[it] = m < p.M;
    a_off[it] = a_ok[it] ? (long)(m / p.R) * p.a_s0 + (long)(m % p.R) * p.a_s1 : 0;
  }
  long w_off[2];
  bool w_ok[2];
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int row = (tid >> 2) + 64 * it;
    w_ok[it] = (row < BN) && (n0 + row < p.N);
    w_off[it] = w_ok[it] ? (long)(n0 + row) * p.ldw : 0;
  }

  float4 ra[2], rb[2];
  auto g_load = [&](int k0) {
    const int k = k0 + 4 * kq;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (a_ok[it]) {
        const float* src = p.A + a_off[it] + k;
        if (A_VEC) {
          if (k < p.K) v = *reinterpret_cast<const float4*>(src);
        } else {
          if (k + 0 < p.K) v.x = src[0];
          if (k + 1 < p.K) v.y = src[1];
          if (k + 2 < p.K) v.z = src[2];
          if (k + 3 < p.K) v.w = src[3];
        }
      }
      ra[it] = v;
      float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
      if (w_ok[it] && k < p.ldw) u = *reinterpret_cast<const float4*>(p.W + w_off[it] + k);
      rb[it] = u;
    }
  };
  auto s_store = [&](int buf) {
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int row = (tid >> 2) + 64 * it;
      *reinterpret_cast<float4*>(As + (buf * BM + row) * LD + 4 * kq) = ra[it];
      if (row < BN) *reinterpret_cast<float4*>(Bs + (buf * BN + row) * LD + 4 * kq) = rb[it];
    }
  };

  f32x4 acc[2][5];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < 5; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nkb = (p.K + BK - 1) / BK;
  g_load(0);
  s_store(0);
  __syncthreads();
  const int fi = lane & 15, fg = lane >> 4;
  for (int kb = 0; kb < nkb; ++kb) {
    const int cur = kb & 1;
    if (kb + 1 < nkb) g_load((kb + 1) * BK);
    const float* Ab = As + (cur * BM + wave * 32 + fi) * LD + 4 * fg;
    const float* Bb = Bs + (cur * BN + fi) * LD + 4 * fg;
    float4 av[2], bv[5];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) av[mt] = *reinterpret_cast<const float4*>(Ab + mt * 16 * LD);
#pragma unroll
    for (int nt = 0; nt < 5; ++nt) bv[nt] = *reinterpret_cast<const float4*>(Bb + nt * 16 * LD);
    // the MFMA contracts over the 4 lane groups; with one float4 per lane, step r covers
    // k = 4*group + r -- A and W use the same permutation, so the sum is the plain dot product
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 5; ++nt)
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4c(av[mt], r), f4c(bv[nt], r), acc[mt][nt], 0, 0, 0);
    if (kb + 1 < nkb) s_store(cur ^ 1);
    __syncthreads();
  }

  // ---- epilogue: accumulators (+bias) -> LDS C tile -> (residual) -> (group L2 norm) -> coalesced store
  float* Cs = smem;
#pragma unroll
  for (int nt = 0; nt < 5; ++nt) {
    const int col = nt * 16 + fi;
    const float bv1 = (n0 + col < p.N) ? p.bias[n0 + col] : 0.0f;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) Cs[(wave * 32 + mt * 16 + 4 * fg + r) * CLD + col] = acc[mt][nt][r] + bv1;
  }
  if (tid < BM) {
    const int m = m0 + tid;
    c_rowoff[tid] = (m < p.M) ? (long)(m / p.R) * p.c_s0 + (long)(m % p.R) * p.c_s1 : -1;
  }
  __syncthreads();
  if (MODE == ONSSEN_EPI_L2NORM) {
    if (p.resid) {
      for (int e = tid; e < BM * BN; e += 256) {
        const int row = e / BN, col = e % BN;
        const long off = c_rowoff[row];
        if (off >= 0 && n0 + col < p.N) Cs[row * CLD + col] += p.resid[off + n0 + col];
      }
      __syncthreads();
    }
    // 4 lanes per (row, group): strided partial sums, two xor-shuffles, in-place divide
    const int ng = BN / p.group, items = BM * ng, sub = tid & 3;
    for (int it = tid >> 2; it < items; it += 64) {
      float* v = Cs + (it / ng) * CLD + (it % ng) * p.group;
      float s = 0.0f;
      for (int d = sub; d < p.group; d += 4) s += v[d] * v[d];
      s += __shfl_xor(s, 1);
      s += __shfl_xor(s, 2);
      const float den = fmaxf(sqrtf(s), p.eps);
      for (int d = sub; d < p.group; d += 4) v[d] = v[d] / den;
    }
    __syncthreads();
  }
  for (int e = tid; e < BM * BN; e += 256) {
    const int row = e / BN, col = e % BN;
    const long off = c_rowoff[row];
    if (off >= 0 && n0 + col < p.N) {
      float v = Cs[row * CLD + col];
      if (MODE == ONSSEN_EPI_SIGMOID) v = 1.0f / (1.0f + expf(-v));
      if (MODE == ONSSEN_EPI_RELU) {
        v = fmaxf(v, 0.0f);
        if (p.resid) v *= p.resid[off + n0 + col];      // relu(A W^T + b) * gate  (enhance: restoration layer x mask)
      }
      p.C[off + n0 + col] = v;
    }
  }
}


// =================================================================================================
// K3/K7/K8/K9, split-bf16 form:  C = epi(A W^T + bias) with every fp32 product evaluated as
// a_hi*b_hi + a_hi*b_lo + a_lo*b_hi on v_mfma_f32_16x16x32_bf16 (fp32 accumulate).
// 256x160x32 tile, 8 waves (4 along M x 2 along N, 64x80 per wave = 4x5 MFMA tiles, 60 MFMAs per k-step).
// A arrives as fp32 and is split while it is staged into LDS (3 VALU ops per element, hidden behind the
// MFMAs); W is pre-split at pack time ([N][ldw] hi plane, then lo plane).  Epilogues as linear_kernel;
// the tile is 160 = 2 x lcm(16,20) columns wide so that a TF bin's 20 embedding outputs never straddle tiles.
// =================================================================================================
namespace lx3 {
constexpr int BN = 160, BK = 32;
constexpr int LD = 40;                       // LDS row stride in bf16 elements: 32 + 8 pad (80 B rows)
constexpr int QR = 64, CLD = 164;            // epilogue: 64-row slices of the C tile, padded stride
constexpr int EPI_BYTES = QR * CLD * 4;
constexpr int stage_bytes(int bm) { return (2 * bm + 2 * BN) * LD * 2; }
constexpr int smem_bytes(int bm) { return stage_bytes(bm) > EPI_BYTES ? stage_bytes(bm) : EPI_BYTES; }
}  // namespace lx3

struct LinearX3Args {
  const float* A = nullptr;
  long a_s0 = 0, a_s1 = 0;
  const unsigned short* Whi = nullptr;
  const unsigned short* Wlo = nullptr;
  const float* bias = nullptr;
  const float* resid = nullptr;
  float* C = nullptr;
  long c_s0 = 0, c_s1 = 0;
  int R = 1, M = 0, N = 0, K = 0, ldw = 0, group = 0;
  float eps = 0.f;
  int c_vec = 0;    // C rows 16-byte aligned and N % 4 == 0
  int tile_group = 4;  // N-tiles walked together (L2 blocking)
  int ablate = 0;   // profiling only (ONSSEN_X3_ABLATE): 1 no global loads, 2 no split/LDS store, 4 no MFMA, 8 no fragment reads
};

__device__ __forceinline__ unsigned pack2(unsigned short a, unsigned short b) { return (unsigned)a | ((unsigned)b << 16); }

// WM = waves along M (64 rows each): WM=4 -> 256x160 tile, 512 threads, one workgroup per CU; WM=2 -> 128x160
// tile, 256 threads, 46 KB of LDS: three workgroups per CU sit in different phases, so one's MFMAs cover
// another's staging without any intra-workgroup choreography.
template <bool A_VEC, int MODE, int WM>
__global__ __launch_bounds__(128 * WM) void linear_x3_kernel(LinearX3Args p) {
  using namespace lx3;
  constexpr int BM = 64 * WM, NTHR = 128 * WM;
  constexpr int WIT = (2 * BN * 4 + NTHR - 1) / NTHR;      // 16-byte W chunks per thread per k-step
  __shared__ __attribute__((aligned(16))) unsigned char smem_raw[smem_bytes(BM)];
  __shared__ long c_rowoff[BM];
  unsigned short* Ahi = reinterpret_cast<unsigned short*>(smem_raw);
  unsigned short* Alo = Ahi + BM * LD;
  unsigned short* Bhi = Alo + BM * LD;
  unsigned short* Blo = Bhi + BN * LD;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  // XCD-aware tile order: workgroup b is observed to run on XCD b % 8 (speed only, never correctness), so give
  // every XCD a contiguous run of tiles -- neighbours then share their A row panel in that XCD's private L2
  int n0, m0;
  {
    const int nbx = gridDim.x, nwg = nbx * gridDim.y, bid = blockIdx.y * nbx + blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    // ... and walk the tiles in column groups of GN: the group's W panels (GN x ~0.8 MB split-bf16 at K=1200)
    // stay resident in the XCD's 4 MB L2 while the row panels of A stream past them
    const int GN = p.tile_group, nby = gridDim.y;
    const int gfull = nbx / GN, nfull = gfull * GN * nby;
    int tn, tm;
    if (wg < nfull) {
      const int rem = wg % (nby * GN);
      tn = (wg / (nby * GN)) * GN + rem % GN;
      tm = rem / GN;
    } else {
      const int gl = nbx - gfull * GN, rem = wg - nfull;
      tn = gfull * GN + rem % gl;
      tm = rem / gl;
    }
    n0 = tn * BN;
    m0 = tm * BM;
  }

  // ---- staging coordinates.  A: 256 rows x 8 float4 per k-step -> 4 per thread; W: 160 rows x 4 x 16 B per plane
  const int akq = tid & 7;
  long a_off[4];
  bool a_ok[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int m = m0 + (tid >> 3) + (NTHR / 8) * it;
    a_ok[it] = m < p.M;
    a_off[it] = a_ok[it] ? (long)(m / p.R) * p.a_s0 + (long)(m % p.R) * p.a_s1 : 0;
  }
  const int wc = tid & 3;                  // 16-byte chunk within the 64-byte row of a W plane tile
  long w_off[WIT];
  bool w_ok[WIT];
  int w_row[WIT], w_plane[WIT];
#pragma unroll
  for (int it = 0; it < WIT; ++it) {
    const int idx = (tid >> 2) + (NTHR / 4) * it;   // (plane, row)
    w_plane[it] = idx >= BN;
    w_row[it] = idx - (w_plane[it] ? BN : 0);
    w_ok[it] = idx < 2 * BN && (n0 + w_row[it] < p.N);
    w_off[it] = w_ok[it] ? (long)(n0 + w_row[it]) * p.ldw : 0;
  }

  // two register sets: tile kb+2 is requested while tile kb is being multiplied, so a global load has two
  // k-steps (~2 x 60 MFMAs per wave) to land before it is split into LDS
  float4 ra0[4], ra1[4];
  u32x4 rw0[WIT], rw1[WIT];
  auto g_load = [&](float4 (&ra)[4], u32x4 (&rw)[WIT], int k0) {
    if (p.ablate & 1) return;
    const int k = k0 + 4 * akq;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (a_ok[it]) {
        const float* src = p.A + a_off[it] + k;
        if (A_VEC) {
          if (k < p.K) v = *reinterpret_cast<const float4*>(src);
        } else {
          if (k + 0 < p.K) v.x = src[0];
          if (k + 1 < p.K) v.y = src[1];
          if (k + 2 < p.K) v.z = src[2];
          if (k + 3 < p.K) v.w = src[3];
        }
      }
      ra[it] = v;
    }
#pragma unroll
    for (int it = 0; it < WIT; ++it) {
      u32x4 u = {0u, 0u, 0u, 0u};
      if (w_ok[it] && k0 + 8 * wc < p.ldw)
        u = *reinterpret_cast<const u32x4*>((w_plane[it] ? p.Wlo : p.Whi) + w_off[it] + k0 + 8 * wc);
      rw[it] = u;
    }
  };
  auto s_store = [&](const float4 (&ra)[4], const u32x4 (&rw)[WIT]) {
    if (p.ablate & 2) return;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int row = (tid >> 3) + (NTHR / 8) * it;
      unsigned short h0, l0, h1, l1, h2, l2, h3, l3;
      split_bf16(ra[it].x, h0, l0);
      split_bf16(ra[it].y, h1, l1);
      split_bf16(ra[it].z, h2, l2);
      split_bf16(ra[it].w, h3, l3);
      *reinterpret_cast<uint2*>(Ahi + row * LD + 4 * akq) = make_uint2(pack2(h0, h1), pack2(h2, h3));
      *reinterpret_cast<uint2*>(Alo + row * LD + 4 * akq) = make_uint2(pack2(l0, l1), pack2(l2, l3));
    }
#pragma unroll
    for (int it = 0; it < WIT; ++it) {
      const int idx = (tid >> 2) + (NTHR / 4) * it;
      if (idx < 2 * BN)
        *reinterpret_cast<u32x4*>((w_plane[it] ? Blo : Bhi) + w_row[it] * LD + 8 * wc) = rw[it];
    }
  };

  f32x4 acc[4][5];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < 5; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nkb = (p.K + BK - 1) / BK;
  const int fi = lane & 15, fg = lane >> 4;
  auto compute = [&]() {
    s16x8 ah[4], al[4];
    const int fsel = (p.ablate & 8) ? 0 : 1;     // profiling: all fragments from one LDS address
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const int off = fsel * ((wm * 64 + mt * 16 + fi) * LD + 8 * fg);
      ah[mt] = *reinterpret_cast<const s16x8*>(Ahi + off);
      al[mt] = *reinterpret_cast<const s16x8*>(Alo + off);
    }
#pragma unroll
    for (int nt = 0; nt < 5; ++nt) {
      const int off = fsel * ((wn * 80 + nt * 16 + fi) * LD + 8 * fg);
      const s16x8 bh = *reinterpret_cast<const s16x8*>(Bhi + off);
      const s16x8 bl = *reinterpret_cast<const s16x8*>(Blo + off);
      if (p.ablate & 4) {
        acc[0][nt][0] += (float)(bh[0] + bl[0] + ah[0][0] + al[0][0]);   // keep the reads live
        continue;
      }
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        acc[mt][nt] = mfma_bf16(al[mt], bh, acc[mt][nt]);   // small terms first
        acc[mt][nt] = mfma_bf16(ah[mt], bl, acc[mt][nt]);
        acc[mt][nt] = mfma_bf16(ah[mt], bh, acc[mt][nt]);
      }
    }
  };
  g_load(ra0, rw0, 0);
  if constexpr (WM == 4) {          // one fat workgroup per CU: prefetch two k-steps ahead
    if (nkb > 1) g_load(ra1, rw1, BK);
    for (int kb = 0; kb < nkb; kb += 2) {
      s_store(ra0, rw0);
      __syncthreads();
      if (kb + 2 < nkb) g_load(ra0, rw0, (kb + 2) * BK);
      compute();
      __syncthreads();
      if (kb + 1 < nkb) {
        s_store(ra1, rw1);
        __syncthreads();
        if (kb + 3 < nkb) g_load(ra1, rw1, (kb + 3) * BK);
        compute();
        __syncthreads();
      }
    }
  } else {                          // several workgroups per CU hide each other's latencies: one register set
    for (int kb = 0; kb < nkb; ++kb) {
      s_store(ra0, rw0);
      __syncthreads();
      if (kb + 1 < nkb) g_load(ra0, rw0, (kb + 1) * BK);
      compute();
      __syncthreads();
    }
  }

  // ---- epilogue in four 64-row quarters (a full 256x160 fp32 tile would not fit in LDS next to nothing)
  float* Cs = reinterpret_cast<float*>(smem_raw);
  if (tid < BM) {
    const int m = m0 + tid;
    c_rowoff[tid] = (m < p.M) ? (long)(m / p.R) * p.c_s0 + (long)(m % p.R) * p.c_s1 : -1;
  }
  for (int q = 0; q < WM; ++q) {
    __syncthreads();
    if (wm == q) {
#pragma unroll
      for (int nt = 0; nt < 5; ++nt) {
        const int col = wn * 80 + nt * 16 + fi;
        const float bv1 = (n0 + col < p.N) ? p.bias[n0 + col] : 0.0f;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
          for (int r = 0; r < 4; ++r) Cs[(mt * 16 + 4 * fg + r) * CLD + col] = acc[mt][nt][r] + bv1;
      }
    }
    __syncthreads();
    if (MODE == ONSSEN_EPI_L2NORM) {
      if (p.resid) {
        for (int e = tid; e < QR * BN; e += NTHR) {
          const int row = e / BN, col = e % BN;
          const long off = c_rowoff[q * QR + row];
          if (off >= 0 && n0 + col < p.N) Cs[row * CLD + col] += p.resid[off + n0 + col];
        }
        __syncthreads();
      }
      const int ng = BN / p.group, items = QR * ng, sub = tid & 3;
      for (int it = tid >> 2; it < items; it += NTHR / 4) {
        float* v = Cs + (it / ng) * CLD + (it % ng) * p.group;
        float s = 0.0f;
        for (int d = sub; d < p.group; d += 4) s += v[d] * v[d];
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        const float den = fmaxf(sqrtf(s), p.eps);
        for (int d = sub; d < p.group; d += 4) v[d] = v[d] / den;
      }
      __syncthreads();
    }
    if (p.c_vec) {   // rows 16-byte aligned and N % 4 == 0: 16-byte stores, a quarter of the store instructions
      for (int e = tid; e < QR * (BN / 4); e += NTHR) {
        const int row = e / (BN / 4), col = 4 * (e % (BN / 4));
        const long off = c_rowoff[q * QR + row];
        if (off >= 0 && n0 + col < p.N) {
          float4 v = *reinterpret_cast<const float4*>(Cs + row * CLD + col);
          if (MODE == ONSSEN_EPI_SIGMOID) {
            v.x = 1.0f / (1.0f + expf(-v.x)); v.y = 1.0f / (1.0f + expf(-v.y));
            v.z = 1.0f / (1.0f + expf(-v.z)); v.w = 1.0f / (1.0f + expf(-v.w));
          }
          *reinterpret_cast<float4*>(p.C + off + n0 + col) = v;
        }
      }
    } else {
      for (int e = tid; e < QR * BN; e += NTHR) {
        const int row = e / BN, col = e % BN;
        const long off = c_rowoff[q * QR + row];
        if (off >= 0 && n0 + col < p.N) {
          float v = Cs[row * CLD + col];
          if (MODE == ONSSEN_EPI_SIGMOID) v = 1.0f / (1.0f + expf(-v));
          p.C[off + n0 + col] = v;
        }
      }
    }
  }
}

// fp32 [N][ld_in] (K valid columns) -> split-bf16 planes [N][ld_out] hi, [N][ld_out] lo (zero beyond K)
__global__ void pack_w_bf16x3_kernel(const float* __restrict__ w, int N, int K, int ld_in, int ld_out,
                                     unsigned short* __restrict__ hi, unsigned short* __restrict__ lo) {
  const long total = (long)N * ld_out;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int n = (int)(e / ld_out), k = (int)(e % ld_out);
    unsigned short h, l;
    split_bf16(k < K ? w[(long)n * ld_in + k] : 0.0f, h, l);
    hi[e] = h;
    lo[e] = l;
  }
}


// =================================================================================================
// K3/K7/K8, split-bf16 form over PRE-SPLIT operands ("x3 images").
//
// x3 image of a row-major [rows][K] fp32 matrix:  [rows][KB][2][32] bf16, KB = ceil(K/32): for every row and
// 32-wide k block, 64 bytes of hi = bf16(x) followed by 64 bytes of lo = bf16(x - hi) (zeros beyond K).  One
// 128-byte cache line per (row, k-step), for the activations (written in this form by the recurrence epilogue
// or by x3_image_kernel) and for the weights (packed once).
//
// 256x160 tile, 256 threads = 4 waves (2 along M x 2 along N), 128x80 per wave = 8x5 MFMA tiles, 120 MFMAs per
// wave and 32-wide k-step.  Staging is a plain copy (16-byte buffer loads with out-of-range -> 0, no VALU), LDS
// is double-buffered so a k-step costs ONE barrier, and the next tile's LDS writes / the one after's global
// loads are spread between the MFMAs of the current one.  The MFMA operands are swapped (A operand = W rows,
// B operand = activation rows) so that a lane ends up with 4 CONSECUTIVE output features of one row: the
// epilogue (bias, sigmoid, grouped L2 normalisation) runs in registers and stores 16 bytes per lane.
// =================================================================================================
namespace lxp {
constexpr int BM = 256, BN = 160;
#ifndef ONSSEN_XP_RS
#define ONSSEN_XP_RS 160
#endif
// LDS row stride in bytes: 128 + 32 pad.  ds_read_b128 serves a wave in four 16-lane groups ({0-3,12-15,20-27}, {4-11,16-19,
// 28-31}, ... -- MI355X_MICROARCH.md, LDS); for a fragment read (lane -> row lane&15, 16-byte chunk lane>>4) a stride of 160
// puts the 16 lanes of every group on 16 different 16-byte bank slots; 144 (round 1) left 7 two-way conflicts per group
// (SQ_LDS_BANK_CONFLICT 21.6 M per call), 128 would leave 12.
constexpr int RS = ONSSEN_XP_RS;
constexpr int STAGE = (BM + BN) * RS;        // 66,560 B per stage, two stages
}  // namespace lxp

struct LinearXpArgs {
  const unsigned short* A = nullptr;      // x3 image [M][KB][2][32]
  const unsigned short* W = nullptr;      // x3 image [N][KB][2][32]
  const float* bias = nullptr;
  float* C = nullptr;
  long c_s0 = 0, c_s1 = 0;
  int R = 1, M = 0, N = 0, KB = 0, group = 0;
  float eps = 0.f;
  int tile_group = 4;
  int c_vec = 0;                // C rows 16-byte aligned and N % 4 == 0
  long a_bs = 0, w_bs = 0, c_bs = 0;        // BATCH instantiation: element strides of A image / W image / C between the gridDim.z problems
  float* C2 = nullptr;          // BATCH: columns n >= n_split go to C2 (row addressing c2_s0 / c2_s1 / c2_bs, column n - n_split); null: none
                                // (linear_x3q_kernel, L2NORM with group > 2: [M][N / group] reciprocal clamped norms out; null: none)
  long c2_s0 = 0, c2_s1 = 0, c2_bs = 0;
  int n_split = 0;
  int n_split_odd = 0;          // BATCH with C2: != 0 -> the odd problems write columns < n_split_odd to C2 and the rest to C (outputs change places)
  const float* resid = nullptr; // linear_x3q_kernel, L2NORM: added to A W^T + b before the normalisation; row m at resid + (m / R)*c_s0 +
  int r_mod = 1;                // ((m % R) % r_mod)*c_s1 (the same residual for r_mod-periodic row blocks: the phase head's two speakers); null: none
  const int* dest = nullptr;    // linear_x3q_kernel, L2NORM_COMPACT: [R][dest_bs] target row of every (utterance b = m % R, bin t*F + f) inside
  long dest_bs = 0;             // the utterance's compacted array C + b*c_s1 (rows of `group` floats), or -1: the group is not stored
  int F = 0;                    // ... bins per frame (t = m / R)
};

// profiling builds only (-DONSSEN_XP_ABLATE=bits; compile time, a run-time test per load would wreck the
// schedule being measured): 1 no global loads, 2 no LDS stores, 4 no MFMA, 8 no fragment reads, 16 no C stores
#ifndef ONSSEN_XP_ABLATE
#define ONSSEN_XP_ABLATE 0
#endif

// WMS = waves along M (2 waves along N always): 2 -> 4 waves x (128x80), one per SIMD; 4 -> 8 waves x (64x80), two
// per SIMD (denser MFMA issue and the hardware overlaps one wave's waits with the other's MFMAs, for 38 % more
// fragment reads)
// TERMS = 3: split-bf16 (hi*lo + lo*hi + hi*hi, fp32-grade); TERMS = 1: plain bf16 products (hi*hi only: the lo halves of
// the images are neither fetched nor staged; ~2^-9 relative per product -- BASELINE config 2's literal precision, outside
// the 1e-4 parity contract)
// BATCH: gridDim.z independent problems of the same shape (the two directions' weight-gradient GEMMs of the training path,
// which fill the chip only together); a separate instantiation so that the inference GEMM's code is untouched
template <int MODE, int WMS, int TERMS, bool BATCH = false>
__global__ __launch_bounds__(128 * WMS) void linear_x3p_kernel(LinearXpArgs p) {
  using namespace lxp;
  if constexpr (BATCH) {
    p.A += (long)blockIdx.z * p.a_bs;
    p.W += (long)blockIdx.z * p.w_bs;
    p.C += (long)blockIdx.z * p.c_bs;
    if (p.C2) p.C2 += (long)blockIdx.z * p.c2_bs;
    if (p.C2 && p.n_split_odd && (blockIdx.z & 1)) {
      // (onssen_linear_x3p_batched_split_alt: W = [h_f | x | h_r] rows, problem 0 reads [h_f | x], problem 1 [x | h_r] -- the
      //  layer input's transposed image is made once and serves both directions)
      float* tc = p.C; p.C = p.C2; p.C2 = tc;
      long t0 = p.c_s0; p.c_s0 = p.c2_s0; p.c2_s0 = t0;
      t0 = p.c_s1; p.c_s1 = p.c2_s1; p.c2_s1 = t0;
      p.n_split = p.n_split_odd;
    }
  }
  constexpr int NTHR = 128 * WMS, MT = 16 / WMS, WROWS = BM / WMS;
  constexpr int RSTEP = NTHR / 8;                                   // rows staged per pass of the workgroup
  constexpr int A_IT = BM / RSTEP, W_IT = (BN + RSTEP - 1) / RSTEP;   // 16-byte chunks per thread per k-step
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int fi = lane & 15, fg = lane >> 4;
  // XCD-aware tile order (as linear_x3_kernel): each XCD walks a contiguous run of tiles, in column groups of GN
  int n0, m0;
  {
    const int nbx = gridDim.x, nwg = nbx * gridDim.y, bid = blockIdx.y * nbx + blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    const int GN = p.tile_group, nby = gridDim.y;
    const int gfull = nbx / GN, nfull = gfull * GN * nby;
    int tn, tm;
    if (wg < nfull) {
      const int rem = wg % (nby * GN);
      tn = (wg / (nby * GN)) * GN + rem % GN;
      tm = rem / GN;
    } else {
      const int gl = nbx - gfull * GN, rem = wg - nfull;
      tn = gfull * GN + rem % gl;
      tm = rem / gl;
    }
    n0 = tn * BN;
    m0 = tm * BM;
  }
  const int pitch = p.KB * 128;                // bytes per image row
  const int a_rows = p.M - m0 < BM ? p.M - m0 : BM, w_rows = p.N - n0 < BN ? p.N - n0 : BN;
  const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(p.A + (long)m0 * p.KB * 64), 0, a_rows * pitch, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(p.W + (long)n0 * p.KB * 64), 0, w_rows * pitch, 0x00020000);
  // staging: thread -> (row = tid/8 + RSTEP*it, 16-byte chunk tid%8); rows past the matrix are out of range -> 0
  const int srow = tid >> 3, sch = tid & 7;
  // TERMS == 1: the threads of the lo half-row stay idle (their loads go out of range: no traffic, no LDS write)
  const bool stage_on = TERMS == 3 || sch < 4;
  const unsigned g_voff = stage_on ? (unsigned)(srow * pitch + sch * 16) : 0x40000000u;
  const unsigned l_off = (unsigned)(srow * RS + sch * 16);
  // two staging register sets: set (t & 1) carries tile t from its global load, issued THREE k-steps before the
  // tile is multiplied (L2 -> CU round trips under this load are longer than one k-step), to its LDS write one
  // k-step before
  constexpr int NJ = A_IT + W_IT;
  u32x4 rg[2][NJ];
  auto g_load1 = [&](auto set_c, int j, int kb) {
    constexpr int S = decltype(set_c)::value;
    if constexpr ((ONSSEN_XP_ABLATE & 1) != 0) return;
    // the k offset rides in the (range-checked) vector offset and k blocks past the matrix are sent out of range:
    // they read zeros, never memory -- so the loop needs no "is there a next tile" predicate, its body exists
    // exactly once per parity, and an odd number of k-steps is rounded up with a tile of zeros
    const unsigned koff = kb < p.KB ? (unsigned)(kb * 128) : 0x40000000u;
    if (j < A_IT) rg[S][j] = __builtin_amdgcn_raw_buffer_load_b128(ra, g_voff + (unsigned)(j * RSTEP * pitch) + koff, 0, 0);
    else rg[S][j] = __builtin_amdgcn_raw_buffer_load_b128(rw, g_voff + (unsigned)((j - A_IT) * RSTEP * pitch) + koff, 0, 0);
  };
  auto s_store1 = [&](auto set_c, int j, int stage) {
    constexpr int S = decltype(set_c)::value;
    if constexpr ((ONSSEN_XP_ABLATE & 2) != 0) return;
    unsigned char* base = smem + stage * STAGE + (j < A_IT ? j * RSTEP * RS : BM * RS + (j - A_IT) * RSTEP * RS);
    if (stage_on && (j < A_IT || (j - A_IT) * RSTEP + RSTEP <= BN || srow + (j - A_IT) * RSTEP < BN))   // last W pass may be partial
      *reinterpret_cast<u32x4*>(base + l_off) = rg[S][j];
  };

  f32x4 acc[MT][5];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < 5; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

#ifdef ONSSEN_XP_CLOCK
  const long long clk0 = clock64(), wclk0 = wall_clock64();
#endif
  const int nkb = p.KB;
  const unsigned fa_off = (unsigned)((wm * WROWS + fi) * RS + fg * 16);             // + mt*16*RS (+64 for lo)
  const unsigned fw_off = (unsigned)(BM * RS + (wn * 80 + fi) * RS + fg * 16);    // + nt*16*RS (+64 for lo)
  constexpr bool FR = (ONSSEN_XP_ABLATE & 8) == 0;
  auto frag = [&](const unsigned char* sb, unsigned off) {
    if constexpr (FR) return *reinterpret_cast<const s16x8*>(sb + off);
    else return s16x8{(short)off, 1, 2, 3, 4, 5, 6, 7};
  };
  using c0 = std::integral_constant<int, 0>;
  using c1 = std::integral_constant<int, 1>;

#pragma unroll
  for (int j = 0; j < NJ; ++j) g_load1(c0{}, j, 0);
#pragma unroll
  for (int j = 0; j < NJ; ++j) s_store1(c0{}, j, 0);
#pragma unroll
  for (int j = 0; j < NJ; ++j) g_load1(c1{}, j, 1);
#pragma unroll
  for (int j = 0; j < NJ; ++j) g_load1(c0{}, j, 2);
  __syncthreads();

  // k-step kb of parity E (tile kb sits in LDS stage E): tile kb+1 goes from staging set E^1 into stage E^1 and
  // tile kb+3 is requested into the same set, spread between the five column tiles' MFMAs.  One barrier.
  auto kstep = [&](int kb, auto e_c) {
    constexpr int E = decltype(e_c)::value;
    using eo = std::integral_constant<int, E ^ 1>;
    const unsigned char* sb = smem + E * STAGE;
    s16x8 xh[MT], xl[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      xh[mt] = frag(sb, fa_off + mt * 16 * RS);
      xl[mt] = TERMS == 3 ? frag(sb, fa_off + mt * 16 * RS + 64) : xh[mt];
    }
    s16x8 wh = frag(sb, fw_off), wl = TERMS == 3 ? frag(sb, fw_off + 64) : wh;
#pragma unroll
    for (int nt = 0; nt < 5; ++nt) {
      s16x8 wh2 = wh, wl2 = wl;
      if (nt + 1 < 5) {   // next column tile's fragments land behind this one's 24 MFMAs
        wh2 = frag(sb, fw_off + (nt + 1) * 16 * RS);
        wl2 = TERMS == 3 ? frag(sb, fw_off + (nt + 1) * 16 * RS + 64) : wh2;
      }
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        if (j >= nt * NJ / 5 && j < (nt + 1) * NJ / 5) {
          s_store1(eo{}, j, E ^ 1);
          g_load1(eo{}, j, kb + 3);
        }
      }
      if constexpr ((ONSSEN_XP_ABLATE & 4) != 0) {
        acc[0][nt][0] += (float)(wh[0] + wl[0] + xh[nt % MT][0] + xl[nt % MT][0] + xh[(nt + 3) % MT][0] + xl[(nt + 3) % MT][0]);
      } else {
        // term-major: MT independent accumulators between two MFMAs on the same one (back to back they wait for each
        // other's result: 8 passes of latency against 4 of issue); the order per accumulator -- small terms first -- is unchanged
        if constexpr (TERMS == 3) {
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) acc[mt][nt] = mfma_bf16(wh, xl[mt], acc[mt][nt]);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) acc[mt][nt] = mfma_bf16(wl, xh[mt], acc[mt][nt]);
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt][nt] = mfma_bf16(wh, xh[mt], acc[mt][nt]);
      }
      wh = wh2;
      wl = wl2;
    }
    __syncthreads();
  };
  for (int kb = 0; kb < nkb; kb += 2) {
    kstep(kb, c0{});
    kstep(kb + 1, c1{});
  }

#ifdef ONSSEN_XP_CLOCK   // profiling builds: shader clocks and 100 MHz ticks of the main loop of workgroup 0 -> C[0], C[1]
  if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
    p.C[0] = (float)(clock64() - clk0);
    p.C[1] = (float)(wall_clock64() - wclk0);
    return;
  }
#endif
  // ---- epilogue in registers: lane holds, per (mt, nt), features n = n0 + wn*80 + nt*16 + 4*fg + {0..3} of row
  //      m = m0 + wm*WROWS + mt*16 + fi
  float4 bv[5];
#pragma unroll
  for (int nt = 0; nt < 5; ++nt) {
    const int n = n0 + wn * 80 + nt * 16 + 4 * fg;
    bv[nt].x = n + 0 < p.N ? p.bias[n + 0] : 0.f;
    bv[nt].y = n + 1 < p.N ? p.bias[n + 1] : 0.f;
    bv[nt].z = n + 2 < p.N ? p.bias[n + 2] : 0.f;
    bv[nt].w = n + 3 < p.N ? p.bias[n + 3] : 0.f;
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = m0 + wm * WROWS + mt * 16 + fi;
    float4 v[5];
#pragma unroll
    for (int nt = 0; nt < 5; ++nt)
      v[nt] = make_float4(acc[mt][nt][0] + bv[nt].x, acc[mt][nt][1] + bv[nt].y, acc[mt][nt][2] + bv[nt].z,
                          acc[mt][nt][3] + bv[nt].w);
    if (MODE == ONSSEN_EPI_L2NORM) {
      // groups of p.group consecutive features (group % 4 == 0, 80 % group == 0, at most 4 groups per wave):
      // a lane's float4 never straddles a group; partial sums per group, then across the 4 lane groups
      float part[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int nt = 0; nt < 5; ++nt) {
        const int q = (nt * 16 + 4 * fg) / p.group;
        const float s4 = v[nt].x * v[nt].x + v[nt].y * v[nt].y + v[nt].z * v[nt].z + v[nt].w * v[nt].w;
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) part[qq] += (q == qq) ? s4 : 0.f;
      }
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) {
        part[qq] += __shfl_xor(part[qq], 16);
        part[qq] += __shfl_xor(part[qq], 32);
        part[qq] = 1.0f / fmaxf(sqrtf(part[qq]), p.eps);
      }
#pragma unroll
      for (int nt = 0; nt < 5; ++nt) {
        const int q = (nt * 16 + 4 * fg) / p.group;
        const float sc = q == 0 ? part[0] : q == 1 ? part[1] : q == 2 ? part[2] : part[3];
        // x / max(||x||, eps) like F.normalize: multiply by the reciprocal of the clamped norm
        v[nt].x *= sc; v[nt].y *= sc; v[nt].z *= sc; v[nt].w *= sc;
      }
    } else if (MODE == ONSSEN_EPI_SIGMOID) {
#pragma unroll
      for (int nt = 0; nt < 5; ++nt) {
        v[nt].x = 1.0f / (1.0f + expf(-v[nt].x)); v[nt].y = 1.0f / (1.0f + expf(-v[nt].y));
        v[nt].z = 1.0f / (1.0f + expf(-v[nt].z)); v[nt].w = 1.0f / (1.0f + expf(-v[nt].w));
      }
    }
    if (m < p.M && ((ONSSEN_XP_ABLATE & 16) == 0 || v[0].x == 123.456f)) {
      float* crow = p.C + (long)(m / p.R) * p.c_s0 + (long)(m % p.R) * p.c_s1;
      if constexpr (BATCH) {
        if (p.C2) {   // two dense outputs: columns below n_split to C, the rest to C2 (the gradients of W_ih and W_hh of one direction)
          float* crow2 = p.C2 + (long)(m / p.R) * p.c2_s0 + (long)(m % p.R) * p.c2_s1 - p.n_split;
#pragma unroll
          for (int nt = 0; nt < 5; ++nt) {
            const int n = n0 + wn * 80 + nt * 16 + 4 * fg;
            const float e[4] = {v[nt].x, v[nt].y, v[nt].z, v[nt].w};
#pragma unroll
            for (int q = 0; q < 4; ++q)
              if (n + q < p.N) (n + q < p.n_split ? crow : crow2)[n + q] = e[q];
          }
          continue;
        }
      }
#pragma unroll
      for (int nt = 0; nt < 5; ++nt) {
        const int n = n0 + wn * 80 + nt * 16 + 4 * fg;
        if (p.c_vec) {
          if (n < p.N) *reinterpret_cast<float4*>(crow + n) = v[nt];
        } else {
          if (n + 0 < p.N) crow[n + 0] = v[nt].x;
          if (n + 1 < p.N) crow[n + 1] = v[nt].y;
          if (n + 2 < p.N) crow[n + 2] = v[nt].z;
          if (n + 3 < p.N) crow[n + 3] = v[nt].w;
        }
      }
    }
  }
}

// -------------------------------------------------------------------------------------------------
// linear_x3t_kernel (round 4): the weight-gradient GEMM  C[m][n] = sum_k A[k][m] W[k][n]  that contracts over the ROWS of
// row-major x3 images -- dW = dP^T [h_prev | x] with dP, y and x as the kernels that produced them left them ([T*B rows][column
// blocks of 32][hi | lo][32]) -- so that no transposed image has to be made first.  linear_x3p_kernel's tile, wave layout, MFMA
// order and epilogue (the results are bit-identical to it on the transposed images); what changes is how the operands get
// from memory into MFMA fragments:
//   * a k-step's tile is 32 source rows (k) x 256 / 160 source columns: the 16-byte pieces (8 columns of one plane of one
//     row) are copied into the LDS as blocks [16-column tile][k half 4..7 | 0..3 ... ][4 k][16 columns] of 128 bytes;
//   * a fragment (8 consecutive k of one column per lane) is two ds_read_b64_tr_b16: the 16 lanes of a group address one
//     128-byte block row by row and receive it column by column (lds_read_tr16); the four groups of a wave read four
//     consecutive blocks -- 512 contiguous bytes, conflict-free; the 16-column tiles sit 1056 bytes apart so that the copies'
//     16-byte writes spread over all banks;
//   * the W operand is stitched from two column segments of two images with their own row shift (h of the step BEFORE: rows
//     k - B of y for the forward direction, k + B for the reverse one; x unshifted): per-lane 64-bit addresses, a row outside
//     the image reads a zero block instead.
// gridDim.z = 2 problems (the two directions), each with its own A column offset, segments and outputs.
// -------------------------------------------------------------------------------------------------
struct XtSeg {
  const unsigned short* img;    // row-major x3 image [K rows][pitch / 128 column blocks][2][32]
  long pitch;                   // bytes per image row
  int col0, len, shift;         // columns [col0, col0 + len) of the image, read at row k + shift (len a multiple of 8)
  int out_len;                  // columns of the segment that are stored (<= len: the rest is the image's zero padding)
};
struct LinearXtArgs {
  const unsigned short* A = nullptr;      // row-major x3 image of the [K][>= a_col0 + M] matrix whose columns are this GEMM's rows
  long a_pitch = 0;
  int a_col0[2] = {0, 0};       // per problem
  XtSeg seg[2][2] = {};              // per problem: the GEMM's columns [0, seg[z][0].len) and [seg[z][0].len, N)
  const unsigned short* zero = nullptr;   // 16 readable zero bytes
  int M = 0, N = 0, K = 0;      // K = contraction length (image rows)
  float* C[2][2] = {};          // per problem, per segment: dense output, row m at C + (m / R) * s0 + (m % R) * s1, column n - segment start
  long s0[2][2] = {}, s1[2][2] = {};
  int R = 1;
  int tile_group = 4;
};

#ifndef ONSSEN_XT_ABLATE          // profiling builds only: 1 no global loads, 2 plain ds_read_b64 instead of the transposing read, 4 no LDS stores, 8 no MFMA
#define ONSSEN_XT_ABLATE 0
#endif
template <int TERMS>
__global__ __launch_bounds__(512) void linear_x3t_kernel(LinearXtArgs p) {
  constexpr int BM = 256, BN = 160, WMS = 4, NTHR = 512, MT = 16 / WMS, WROWS = BM / WMS;
  constexpr int TS = 1056;                         // bytes between 16-column tiles of one plane (1024 + 32: see above)
  constexpr int A_PL = (BM / 16) * TS, W_PL = (BN / 16) * TS;      // one plane of the A / W tile
  constexpr int STAGE = 2 * A_PL + 2 * W_PL;       // 54 912 B
  constexpr int A_CH = BM / 8 * 2 * 32 / NTHR;     // 16-byte pieces per thread and k-step: A 2048 / 512 = 4
  constexpr int W_CH = (BN / 8 * 2 * 32 + NTHR - 1) / NTHR;        // W 1280 / 512 -> 3 (the last pass half empty)
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, z = blockIdx.z;
  const int wm = wave >> 1, wn = wave & 1;
  const int fi = lane & 15, fg = lane >> 4;
  int n0, m0;
  {   // XCD-aware tile order, as linear_x3p_kernel
    const int nbx = gridDim.x, nwg = nbx * gridDim.y, bid = blockIdx.y * nbx + blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    const int GN = p.tile_group, nby = gridDim.y;
    const int gfull = nbx / GN, nfull = gfull * GN * nby;
    int tn, tm;
    if (wg < nfull) {
      const int rem = wg % (nby * GN);
      tn = (wg / (nby * GN)) * GN + rem % GN;
      tm = rem / GN;
    } else {
      const int gl = nbx - gfull * GN, rem = wg - nfull;
      tn = gfull * GN + rem % gl;
      tm = rem / gl;
    }
    n0 = tn * BN;
    m0 = tm * BM;
  }
  // ---- staging: every thread owns A_CH + W_CH 16-byte pieces.  Per piece only a 32-bit byte offset (of its k = 0 row from its
  //      image's base: negative for a shifted row), its LDS offset and two flag bits live in registers; image base, bytes per
  //      32 rows and row shift are uniform per (problem, segment) and come from scalar registers
  constexpr int NJ = A_CH + W_CH;
  int g_off[NJ];
  unsigned l_off[NJ];
  int k_ofw[W_CH];
  unsigned flags = 0u;                             // bit j: piece j exists;  bit 8 + j: (W piece) it reads segment 1
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const bool isA = j < A_CH;
    const int pc = tid + NTHR * (isA ? j : j - A_CH);
    // piece -> (k row, plane, 8-column chunk cc): A 64 pieces per row (2 planes x 32 chunks), W 40 (2 x 20)
    const int per_row = isA ? 2 * (BM / 8) : 2 * (BN / 8);
    const int kk = pc / per_row, rest = pc % per_row, plane = rest / (per_row / 2), cc = rest % (per_row / 2);
    const int col = (isA ? m0 : n0) + 8 * cc;               // GEMM row (A) / column (W) of the piece's first element
    const bool ok = kk < 32 && col < (isA ? p.M : p.N);
    long pitch = p.a_pitch;
    int scol = p.a_col0[z] + col, shift = 0, sg = 0;
    if (!isA) {
      sg = col < p.seg[z][0].len ? 0 : 1;
      pitch = p.seg[z][sg].pitch; shift = p.seg[z][sg].shift;
      scol = p.seg[z][sg].col0 + col - (sg ? p.seg[z][0].len : 0);
      k_ofw[j - A_CH] = kk;
    }
    flags |= (ok ? 1u : 0u) << j | (unsigned)sg << (8 + j);
    g_off[j] = (int)((long)(kk + shift) * pitch + (long)(scol >> 5) * 128 + plane * 64 + (scol & 31) * 2);
    const int tcol = 8 * cc;                                // column inside the tile
    l_off[j] = (unsigned)((isA ? 0 : 2 * A_PL) + plane * (isA ? A_PL : W_PL) + (tcol >> 4) * TS +
                          (((kk >> 2) & 1) * 4 + (kk >> 3)) * 128 + (kk & 3) * 32 + (tcol & 15) * 2);
  }
  const unsigned char* zero = reinterpret_cast<const unsigned char*>(p.zero);
  const unsigned char* baseA = reinterpret_cast<const unsigned char*>(p.A);
  const unsigned char* base0 = reinterpret_cast<const unsigned char*>(p.seg[z][0].img);
  const unsigned char* base1 = reinterpret_cast<const unsigned char*>(p.seg[z][1].img);
  const long stepA = 32 * p.a_pitch, step0 = 32 * p.seg[z][0].pitch, step1 = 32 * p.seg[z][1].pitch;
  const int shift0 = p.seg[z][0].shift, shift1 = p.seg[z][1].shift;
  u32x4 rg[2][NJ];
  auto g_load1 = [&](auto set_c, int j, int kb) {
    constexpr int S = decltype(set_c)::value;
    const unsigned char* src;
    bool on = (flags >> j) & 1u;
    if (j < A_CH) {
      on = on && kb * 32 + wave + 8 * j < p.K;            // (an A piece's k row: (tid + 512 j) / 64)
      src = baseA + (long)g_off[j] + (long)kb * stepA;
    } else {
      const bool s1 = (flags >> (8 + j)) & 1u;
      const int ks = kb * 32 + k_ofw[j - A_CH] + (s1 ? shift1 : shift0);      // source row
      on = on && ks >= 0 && ks < p.K;
      src = (s1 ? base1 : base0) + (long)g_off[j] + (long)kb * (s1 ? step1 : step0);
    }
    src = on ? src : zero;                                 // (address select, not value select: no branch around the load)
    if constexpr ((ONSSEN_XT_ABLATE & 1) != 0) { rg[S][j] = u32x4{(unsigned)(size_t)src, 1u, 2u, 3u}; return; }
    rg[S][j] = *reinterpret_cast<const u32x4*>(src);
  };
  auto s_store1 = [&](auto set_c, int j, int stage) {
    constexpr int S = decltype(set_c)::value;
    if constexpr ((ONSSEN_XT_ABLATE & 4) != 0) { if (rg[S][j][0] == 0x12345u) smem[0] = 1; return; }
    if (j < A_CH || tid + NTHR * (j - A_CH) < 2 * (BN / 8) * 32)
      *reinterpret_cast<u32x4*>(smem + stage * STAGE + l_off[j]) = rg[S][j];
  };

  f32x4 acc[MT][5];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < 5; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nkb = (p.K + 31) / 32;
  // fragment (tile t of a plane, k half h): block ((t) * TS) + (h * 4 + fg) * 128, row fi / 4, 8-byte piece fi % 4
  const unsigned f_lane = (unsigned)(fg * 128 + (fi >> 2) * 32 + (fi & 3) * 8);
  const unsigned fa_off = (unsigned)((wm * (WROWS / 16)) * TS) + f_lane;                    // + mt * TS (+ A_PL for lo) (+ 512 for the second half)
  const unsigned fw_off = (unsigned)(2 * A_PL + (wn * 5) * TS) + f_lane;                   // + nt * TS (+ W_PL for lo)
  auto frag = [&](const unsigned char* sb, unsigned off) -> s16x8 {
    s16x4 a, b;
    if constexpr ((ONSSEN_XT_ABLATE & 2) != 0) {
      a = *reinterpret_cast<const s16x4*>(sb + off);
      b = *reinterpret_cast<const s16x4*>(sb + off + 512);
    } else {
      a = lds_read_tr16(reinterpret_cast<const unsigned short*>(sb + off));
      b = lds_read_tr16(reinterpret_cast<const unsigned short*>(sb + off + 512));
    }
    s16x8 r;
    r[0] = a[0]; r[1] = a[1]; r[2] = a[2]; r[3] = a[3]; r[4] = b[0]; r[5] = b[1]; r[6] = b[2]; r[7] = b[3];
    return r;
  };
  using c0 = std::integral_constant<int, 0>;
  using c1 = std::integral_constant<int, 1>;
#pragma unroll
  for (int j = 0; j < NJ; ++j) g_load1(c0{}, j, 0);
#pragma unroll
  for (int j = 0; j < NJ; ++j) s_store1(c0{}, j, 0);
#pragma unroll
  for (int j = 0; j < NJ; ++j) g_load1(c1{}, j, 1);
#pragma unroll
  for (int j = 0; j < NJ; ++j) g_load1(c0{}, j, 2);
  __syncthreads();
  auto kstep = [&](int kb, auto e_c) {
    constexpr int E = decltype(e_c)::value;
    using eo = std::integral_constant<int, E ^ 1>;
    const unsigned char* sb = smem + E * STAGE;
    s16x8 xh[MT], xl[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      xh[mt] = frag(sb, fa_off + mt * TS);
      xl[mt] = TERMS == 3 ? frag(sb, fa_off + mt * TS + A_PL) : xh[mt];
    }
    s16x8 wh = frag(sb, fw_off), wl = TERMS == 3 ? frag(sb, fw_off + W_PL) : wh;
#pragma unroll
    for (int nt = 0; nt < 5; ++nt) {
      s16x8 wh2 = wh, wl2 = wl;
      if (nt + 1 < 5) {
        wh2 = frag(sb, fw_off + (nt + 1) * TS);
        wl2 = TERMS == 3 ? frag(sb, fw_off + (nt + 1) * TS + W_PL) : wh2;
      }
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        if (j >= nt * NJ / 5 && j < (nt + 1) * NJ / 5) {
          s_store1(eo{}, j, E ^ 1);
          g_load1(eo{}, j, kb + 3);
        }
      }
      // (linear_x3p_kernel's operand roles: the A operand of the MFMA is the W fragment, so that a lane ends up with four
      //  consecutive columns n of one row m)
      if constexpr ((ONSSEN_XT_ABLATE & 8) != 0) {
        acc[0][nt][0] += (float)(wh[0] + wl[0] + xh[nt % MT][0] + xl[nt % MT][0]);
      } else {
        if constexpr (TERMS == 3) {
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) acc[mt][nt] = mfma_bf16(wh, xl[mt], acc[mt][nt]);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) acc[mt][nt] = mfma_bf16(wl, xh[mt], acc[mt][nt]);
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt][nt] = mfma_bf16(wh, xh[mt], acc[mt][nt]);
      }
      wh = wh2;
      wl = wl2;
    }
    __syncthreads();
  };
  for (int kb = 0; kb < nkb; kb += 2) {
    kstep(kb, c0{});
    kstep(kb + 1, c1{});
  }
  // ---- epilogue: lane holds, per (mt, nt), columns n = n0 + wn*80 + nt*16 + 4*fg + {0..3} of row m = m0 + wm*WROWS + mt*16 + fi
  const int split = p.seg[z][0].len, end0 = p.seg[z][0].out_len, end1 = split + p.seg[z][1].out_len;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = m0 + wm * WROWS + mt * 16 + fi;
    if (m >= p.M) continue;
    float* r0 = p.C[z][0] + (long)(m / p.R) * p.s0[z][0] + (long)(m % p.R) * p.s1[z][0];
    float* r1 = p.C[z][1] + (long)(m / p.R) * p.s0[z][1] + (long)(m % p.R) * p.s1[z][1] - split;
#pragma unroll
    for (int nt = 0; nt < 5; ++nt) {
      const int n = n0 + wn * 80 + nt * 16 + 4 * fg;
      const float e[4] = {acc[mt][nt][0], acc[mt][nt][1], acc[mt][nt][2], acc[mt][nt][3]};
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (n + q < split ? n + q < end0 : n + q < end1) (n + q < split ? r0 : r1)[n + q] = e[q];
    }
  }
}

// -------------------------------------------------------------------------------------------------
// linear_x3q_kernel: the GEMM over x3 images with 256 x 320 workgroup tiles (round 2).
//
// What the round-1 kernel (linear_x3p_kernel: 256 x 160 tile, 64 x 80 per wave) waited for was the LDS: 18 fragment reads
// + 7 staging writes per wave and k-step ~ 1 250 LDS clocks against 1 920 MFMA clocks per SIMD, in a burst after every
// barrier, plus 56 staging registers per lane.  Here
//   * a wave owns 128 x 80 of C (MT = 8, NT = 5: 26 fragment reads for 120 MFMAs instead of 18 for 60), eight waves = 2 x 4;
//   * operands go global -> LDS DIRECTLY (buffer_load_dwordx4 ... lds, 1 KiB per wave-instruction): no staging registers, no
//     ds_write, 9 instructions per wave and k-step.  An LDS-DMA instruction writes 64 consecutive 16-byte slots (8 rows of
//     128 B: hi 64 | lo 64), so rows cannot be padded; the 16-byte chunks of a row are XOR-SWIZZLED instead -- LDS slot
//     (row, c') holds chunk c' ^ (row & 7) -- the lane chooses which GLOBAL chunk it fetches, and fragment reads (lane ->
//     row lane&15, chunk lane>>4) are conflict-free in each of ds_read_b128's four 16-lane groups (brute-forced);
//   * two LDS stages as two separate __shared__ objects (so that a ds_read of one is provably independent of a DMA into
//     the other), one barrier per k-step, the next k-step's DMA issued before this one's MFMAs.
// Same operand images, epilogues and C addressing as linear_x3p_kernel; same accumulation order per output element
// (small terms first, k ascending): bit-identical results.
// -------------------------------------------------------------------------------------------------
#ifndef ONSSEN_XQ_CSTORE
#define ONSSEN_XQ_CSTORE 0      // build variants: 1 = C leaves with non-temporal stores, 2 = write-through (sc1) stores (measured in round 3, see DESIGN 'GEMM')
#endif
#ifndef ONSSEN_XQ_STAGGER
#define ONSSEN_XQ_STAGGER 0     // build variant (round 6c, measured SLOWER: layer-1 projection 0.314-0.320 -> 0.321-0.330 ms): first-round workgroups start (CU slot % PHASES) x this x 64 clocks late; see the kernel
#endif
#ifndef ONSSEN_XQ_WIDE_STORE
#define ONSSEN_XQ_WIDE_STORE 0  // build variant (round 6c): C leaves in 128-byte pieces per row and instruction (DPP half swap between neighbouring tiles)
#endif
#ifndef ONSSEN_XQ_PRIO
#define ONSSEN_XQ_PRIO 0        // build variant (round 6c): s_setprio 1 for waves 4-7 (1) or 0-3 (2) of linear_x3q_kernel before its k-loop
#endif
#ifndef ONSSEN_XQ_STAGGER_PHASES
#define ONSSEN_XQ_STAGGER_PHASES 8
#endif
#define ONSSEN_EPI_L2NORM_SIGMOID 3     // internal (onssen_linear_x3p_pair): L2NORM for columns < n_split into C, SIGMOID for the rest into C2
#define ONSSEN_EPI_L2NORM_COMPACT 4     // internal (onssen_linear_x3p_compact): L2NORM, and only the groups (TF bins) that p.dest names are stored,
                                        // each as one row of the utterance's compacted array -- the deep-clustering back end clusters the active
                                        // bins only (evaluate.py:36-37), so the embedding of the silent ones never reaches HBM
namespace lxq {
constexpr int BM_MAX = 256;
}  // namespace lxq

// BN = 320 (wave tile 128 x 80: whole groups of 20 / 40 / 80 features for the L2NORM epilogue) or 256 (128 x 64); the host
// picks the width that needs fewer rounds of 256 workgroups x tile columns (N = 2400: 10 tiles of 256 instead of 8 of 320,
// the same 2560 padded columns, but e.g. 500 instead of 400 tiles for 12 800 rows = 1.95 instead of 1.56 -> 2 rounds)
// BM = 256 (wave tile 128 rows) or 128 (64 rows): half-height tiles for shapes whose 256-row tiles would leave CUs idle (the
// training path's input-gradient GEMMs: 6 400 x 1 280 x 4 800 is 125 tiles of 256 x 256 but 250 of 128 x 256)
template <int MODE, int TERMS, bool BATCH = false, int BN = 320, int BM = 256>
__global__ __launch_bounds__(512) void linear_x3q_kernel(LinearXpArgs p) {
  using namespace lxq;
  constexpr int STAGE = (BM + BN) * 128;       // 73 728 / 65 536 B per stage, two stages (1 workgroup per CU)
  constexpr int WN = BN / 4, NQW = (BM + BN) / 64;   // columns per wave; LDS-DMA instructions per wave and k-step
  if constexpr (BATCH) {
    p.A += (long)blockIdx.z * p.a_bs;
    p.W += (long)blockIdx.z * p.w_bs;
    p.C += (long)blockIdx.z * p.c_bs;
  }
  constexpr int MT = BM / 32, NT = WN / 16, WM = BM / 2;      // row fragments per wave; rows per wave
  __shared__ __attribute__((aligned(1024))) unsigned char stage0[STAGE];
  __shared__ __attribute__((aligned(1024))) unsigned char stage1[STAGE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int fi = lane & 15, fg = lane >> 4;
#if ONSSEN_XQ_STAGGER
  // round 6c experiment: all tiles of a launch take the same time, so the chip computes in lock step and then stores C in lock step
  // (84 MB per round at once: 40-50 us of a 0.3 ms projection with the MFMA pipe idle).  Delay the FIRST round's workgroups by
  // (CU slot % PHASES) x STAGGER x 64 clocks, so that from then on the C stores of some CUs fall under the k-loops of the others.
  if (p.KB >= 16) {
    const int bl = blockIdx.y * gridDim.x + blockIdx.x;
    if (bl < 256) {
      const int ph = (bl >> 3) & (ONSSEN_XQ_STAGGER_PHASES - 1);
      for (int i = 0; i < ph; ++i) __builtin_amdgcn_s_sleep(ONSSEN_XQ_STAGGER);
    }
  }
#endif
  // XCD-aware tile order (as linear_x3p_kernel): each XCD walks a contiguous run of tiles, in column groups of GN
  int n0, m0;
  {
    const int nbx = gridDim.x, nwg = nbx * gridDim.y, bid = blockIdx.y * nbx + blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    const int GN = p.tile_group, nby = gridDim.y;
    const int gfull = nbx / GN, nfull = gfull * GN * nby;
    int tn, tm;
    if (wg < nfull) {
      const int rem = wg % (nby * GN);
      tn = (wg / (nby * GN)) * GN + rem % GN;
      tm = rem / GN;
    } else {
      const int gl = nbx - gfull * GN, rem = wg - nfull;
      tn = gfull * GN + rem % gl;
      tm = rem / gl;
    }
    n0 = tn * BN;
    m0 = tm * BM;
  }
  const int pitch = p.KB * 128;                // bytes per image row
  const int a_rows = p.M - m0 < BM ? p.M - m0 : BM, w_rows = p.N - n0 < BN ? p.N - n0 : BN;
  const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(p.A + (long)m0 * p.KB * 64), 0, a_rows * pitch, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(p.W + (long)n0 * p.KB * 64), 0, w_rows * pitch, 0x00020000);
  // ---- staging: 72 LDS-DMA instructions per k-step, 9 per wave; instruction q covers LDS rows 8q .. 8q+7 (A rows for
  //      q < 32, W rows above); lane i writes slot (row 8q + (i>>3), c' = i&7) and fetches global chunk c' ^ (i>>3)
  const unsigned dma_lane = (unsigned)((lane >> 3) * pitch + (((lane & 7) ^ (lane >> 3)) * 16));
  auto dma = [&](unsigned char* stage, int kb) {
    const unsigned koff = (unsigned)(kb * 128);
#pragma unroll
    for (int j = 0; j < NQW; ++j) {
      const int q = wave * NQW + j;                                   // wave-uniform
      if (q < BM / 8)   // rows past the matrix: out of range -> zeros land in the LDS
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, ONSSEN_LDS_PTR(stage + q * 1024), 16, dma_lane + (unsigned)(q * 8 * pitch) + koff, 0, 0, 0);
      else
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, ONSSEN_LDS_PTR(stage + q * 1024), 16, dma_lane + (unsigned)((q - BM / 8) * 8 * pitch) + koff, 0, 0, 0);
    }
  };

  f32x4 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // fragment addresses inside a stage: row * 128 + swizzled chunk; row & 7 == fi & 7 for every row a lane reads
  const unsigned ch = (unsigned)((fg ^ (fi & 7)) * 16), cl = ch ^ 64u;
  const unsigned fa_off = (unsigned)((wm * WM + fi) * 128);                  // + mt*16*128
  const unsigned fw_off = (unsigned)((BM + wn * WN + fi) * 128);             // + nt*16*128
  auto compute = [&](const unsigned char* sb) {
    s16x8 wh[NT], wl[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      wh[nt] = *reinterpret_cast<const s16x8*>(sb + fw_off + nt * 2048 + ch);
      wl[nt] = TERMS == 3 ? *reinterpret_cast<const s16x8*>(sb + fw_off + nt * 2048 + cl) : wh[nt];
    }
    s16x8 xh = *reinterpret_cast<const s16x8*>(sb + fa_off + ch);
    s16x8 xl = TERMS == 3 ? *reinterpret_cast<const s16x8*>(sb + fa_off + cl) : xh;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      s16x8 xh2 = xh, xl2 = xl;
      if (mt + 1 < MT) {   // next row tile's fragments land behind this one's 15 MFMAs
        xh2 = *reinterpret_cast<const s16x8*>(sb + fa_off + (mt + 1) * 2048 + ch);
        xl2 = TERMS == 3 ? *reinterpret_cast<const s16x8*>(sb + fa_off + (mt + 1) * 2048 + cl) : xh2;
      }
      // term-major: NT independent accumulators between two MFMAs on the same one; small terms first
      if constexpr (TERMS == 3) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = mfma_bf16(wh[nt], xl, acc[mt][nt]);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = mfma_bf16(wl[nt], xh, acc[mt][nt]);
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = mfma_bf16(wh[nt], xh, acc[mt][nt]);
      xh = xh2;
      xl = xl2;
    }
  };

  const int nkb = p.KB;
#if ONSSEN_XQ_PRIO
  // round 6c experiment (MI355X_MICROARCH.md, "static priority for the younger half"): one s_setprio for one half of the workgroup's
  // waves before the main loop -- 1: waves 4-7 (the second-dispatched wave of every SIMD), 2: waves 0-3
  if ((ONSSEN_XQ_PRIO == 1) == (wave >= 4)) __builtin_amdgcn_s_setprio(1);
#endif
  dma(stage0, 0);
  __builtin_amdgcn_s_waitcnt(0x0F70);     // vmcnt(0): this wave's DMA has landed
  __syncthreads();
  for (int kb = 0; kb < nkb; kb += 2) {
    if (kb + 1 < nkb) dma(stage1, kb + 1);
    compute(stage0);
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __syncthreads();
    if (kb + 1 < nkb) {
      if (kb + 2 < nkb) dma(stage0, kb + 2);
      compute(stage1);
      __builtin_amdgcn_s_waitcnt(0x0F70);
      __syncthreads();
    }
  }

  // ---- epilogue in registers: lane holds, per (mt, nt), features n = n0 + wn*80 + nt*16 + 4*fg + {0..3} of row
  //      m = m0 + wm*128 + mt*16 + fi
  float4 bv[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int n = n0 + wn * WN + nt * 16 + 4 * fg;
    bv[nt].x = n + 0 < p.N ? p.bias[n + 0] : 0.f;
    bv[nt].y = n + 1 < p.N ? p.bias[n + 1] : 0.f;
    bv[nt].z = n + 2 < p.N ? p.bias[n + 2] : 0.f;
    bv[nt].w = n + 3 < p.N ? p.bias[n + 3] : 0.f;
  }
  // L2NORM_COMPACT: the targets of this wave's (at most four) bins for every row tile, one 16-byte word each, all in flight
  // before the epilogue's arithmetic (five dependent 4-byte loads per row tile inside the loop made the scattering GEMM slower
  // than the one that stores everything)
  u32x4 posv[MODE == ONSSEN_EPI_L2NORM_COMPACT ? MT : 1];
  if constexpr (MODE == ONSSEN_EPI_L2NORM_COMPACT) {
    const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)p.dest, 0, (int)((long)p.R * p.dest_bs * 4 + 12), 0x00020000);   // (+12: the last row's 16-byte word may end past the map; the caller pads it)
    const int f0 = (n0 + wn * WN) / p.group;                     // first bin of the wave's columns (WN % group == 0)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int m = m0 + wm * WM + mt * 16 + fi;
      posv[mt] = __builtin_amdgcn_raw_buffer_load_b128(
          rd, m < p.M ? (unsigned)(((long)(m % p.R) * p.dest_bs + (long)(m / p.R) * p.F + f0) * 4) : 0x7ffffff0u, 0, 0);
    }
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = m0 + wm * WM + mt * 16 + fi;
    float4 v[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
      v[nt] = make_float4(acc[mt][nt][0] + bv[nt].x, acc[mt][nt][1] + bv[nt].y, acc[mt][nt][2] + bv[nt].z,
                          acc[mt][nt][3] + bv[nt].w);
    if (MODE == ONSSEN_EPI_L2NORM && p.resid && m < p.M) {   // (+ residual) before the normalisation: phase_net's "+ mix phase"
      const float* rrow = p.resid + (long)(m / p.R) * p.c_s0 + (long)((m % p.R) % p.r_mod) * p.c_s1;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int n = n0 + wn * WN + nt * 16 + 4 * fg;
        v[nt].x += n + 0 < p.N ? rrow[n + 0] : 0.f;
        v[nt].y += n + 1 < p.N ? rrow[n + 1] : 0.f;
        v[nt].z += n + 2 < p.N ? rrow[n + 2] : 0.f;
        v[nt].w += n + 3 < p.N ? rrow[n + 3] : 0.f;
      }
    }
    if (MODE == ONSSEN_EPI_L2NORM && p.group == 2) {       // pairs (re, im): both pairs of a lane's four columns are its own
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const float s0 = 1.0f / fmaxf(sqrtf(v[nt].x * v[nt].x + v[nt].y * v[nt].y), p.eps);
        const float s1 = 1.0f / fmaxf(sqrtf(v[nt].z * v[nt].z + v[nt].w * v[nt].w), p.eps);
        v[nt].x *= s0; v[nt].y *= s0; v[nt].z *= s1; v[nt].w *= s1;
      }
    } else if (MODE == ONSSEN_EPI_L2NORM || MODE == ONSSEN_EPI_L2NORM_SIGMOID || MODE == ONSSEN_EPI_L2NORM_COMPACT) {
      float part[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int q = (nt * 16 + 4 * fg) / p.group;
        const float s4 = v[nt].x * v[nt].x + v[nt].y * v[nt].y + v[nt].z * v[nt].z + v[nt].w * v[nt].w;
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) part[qq] += (q == qq) ? s4 : 0.f;
      }
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) {
        part[qq] += __shfl_xor(part[qq], 16);
        part[qq] += __shfl_xor(part[qq], 32);
        part[qq] = 1.0f / fmaxf(sqrtf(part[qq]), p.eps);
      }
      if (MODE == ONSSEN_EPI_L2NORM && p.C2 && fg == 0 && m < p.M) {
        // training forward (onssen_linear_x3p_norms): 1 / max(||x||, eps) of every group, [M][N / group] -- with it the backward
        // of the normalisation needs the normalised rows only, and the raw product is never written
        const int ng = p.N / p.group, g0 = (n0 + wn * WN) / p.group;
#pragma unroll
        for (int qq = 0; qq < 4; ++qq)
          if ((qq + 1) * p.group <= WN && g0 + qq < ng) p.C2[(long)m * ng + g0 + qq] = part[qq];
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int q = (nt * 16 + 4 * fg) / p.group;
        const float sc = q == 0 ? part[0] : q == 1 ? part[1] : q == 2 ? part[2] : part[3];
        if (MODE == ONSSEN_EPI_L2NORM_SIGMOID && n0 + wn * WN + nt * 16 + 4 * fg >= p.n_split) {   // the second head's columns
          v[nt].x = 1.0f / (1.0f + expf(-v[nt].x)); v[nt].y = 1.0f / (1.0f + expf(-v[nt].y));
          v[nt].z = 1.0f / (1.0f + expf(-v[nt].z)); v[nt].w = 1.0f / (1.0f + expf(-v[nt].w));
        } else {
          v[nt].x *= sc; v[nt].y *= sc; v[nt].z *= sc; v[nt].w *= sc;
        }
      }
    } else if (MODE == ONSSEN_EPI_SIGMOID) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        v[nt].x = 1.0f / (1.0f + expf(-v[nt].x)); v[nt].y = 1.0f / (1.0f + expf(-v[nt].y));
        v[nt].z = 1.0f / (1.0f + expf(-v[nt].z)); v[nt].w = 1.0f / (1.0f + expf(-v[nt].w));
      }
    }
    if constexpr (MODE == ONSSEN_EPI_L2NORM_COMPACT) {
      // a lane's float4 is four features of ONE group (bin): where does that bin's row go?  -1: nowhere (a silent bin).  The
      // wave's WN columns are at most four bins: their targets were fetched as ONE 16-byte word per row tile before this loop
      if (m < p.M) {
        float* cb = p.C + (long)(m % p.R) * p.c_s1;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const int n = n0 + wn * WN + nt * 16 + 4 * fg, q = (nt * 16 + 4 * fg) / p.group;
          const int pos = (int)(q == 0 ? posv[mt][0] : q == 1 ? posv[mt][1] : q == 2 ? posv[mt][2] : posv[mt][3]);
          if (n < p.N && pos >= 0) *reinterpret_cast<float4*>(cb + (long)pos * p.group + (nt * 16 + 4 * fg) % p.group) = v[nt];
        }
      }
      continue;
    }
#if ONSSEN_XQ_WIDE_STORE
    // round 6c experiment: 128 contiguous bytes per row and store instruction instead of 64.  A lane holds 16 bytes of row fi for every
    // 16-column tile: the four lanes of a row make 64 bytes per instruction.  Swapping the halves of the 16 rows between two neighbouring
    // tiles (DPP row_ror:8) lets one instruction store rows 0-7 of BOTH tiles (8 rows x 128 B) and the next one rows 8-15; the same
    // values reach the same addresses, only the instruction they ride in changes.  (Bias / sigmoid / plain L2NORM epilogues; workgroup-
    // uniform condition.)
    if (MODE != ONSSEN_EPI_L2NORM_SIGMOID && p.c_vec) {
      const int mb = m0 + wm * WM + mt * 16, r8 = fi & 7;
      const int ma = mb + r8, mc = mb + r8 + 8;                  // the rows this lane stores to: first instruction, second instruction
      float* rowa = p.C + (long)(ma / p.R) * p.c_s0 + (long)(ma % p.R) * p.c_s1;
      float* rowc = p.C + (long)(mc / p.R) * p.c_s0 + (long)(mc % p.R) * p.c_s1;
      const bool lowh = fi < 8;
      auto ror8 = [](float x) { return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x128, 0xf, 0xf, false)); };
#pragma unroll
      for (int nt = 0; nt + 1 < NT; nt += 2) {
        const float4 a = v[nt], b = v[nt + 1];
        const float4 sa = make_float4(ror8(a.x), ror8(a.y), ror8(a.z), ror8(a.w));      // tile nt of row fi ^ 8
        const float4 sb = make_float4(ror8(b.x), ror8(b.y), ror8(b.z), ror8(b.w));      // tile nt + 1 of row fi ^ 8
        const int na = n0 + wn * WN + (lowh ? nt : nt + 1) * 16 + 4 * fg;               // rows 0-7: own tile nt | row fi - 8's tile nt + 1
        const int nc = n0 + wn * WN + (lowh ? nt : nt + 1) * 16 + 4 * fg;               // rows 8-15: row fi + 8's tile nt | own tile nt + 1
        const float4 va = lowh ? a : sb, vc = lowh ? sa : b;
        if (ma < p.M && na < p.N) *reinterpret_cast<float4*>(rowa + na) = va;
        if (mc < p.M && nc < p.N) *reinterpret_cast<float4*>(rowc + nc) = vc;
      }
      if (NT & 1) {                                              // the odd last tile: 64-byte pieces as before
        const int n = n0 + wn * WN + (NT - 1) * 16 + 4 * fg;
        if (m < p.M && n < p.N) *reinterpret_cast<float4*>(p.C + (long)(m / p.R) * p.c_s0 + (long)(m % p.R) * p.c_s1 + n) = v[NT - 1];
      }
      continue;
    }
#endif
    if (m < p.M) {
      float* crow = p.C + (long)(m / p.R) * p.c_s0 + (long)(m % p.R) * p.c_s1;
      float* crow2 = MODE == ONSSEN_EPI_L2NORM_SIGMOID ? p.C2 + (long)(m / p.R) * p.c2_s0 + (long)(m % p.R) * p.c2_s1 - p.n_split : nullptr;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int n = n0 + wn * WN + nt * 16 + 4 * fg;
        if (MODE == ONSSEN_EPI_L2NORM_SIGMOID && n >= p.n_split) {      // second output: columns n - n_split of its own rows
          if (n + 0 < p.N) crow2[n + 0] = v[nt].x;
          if (n + 1 < p.N) crow2[n + 1] = v[nt].y;
          if (n + 2 < p.N) crow2[n + 2] = v[nt].z;
          if (n + 3 < p.N) crow2[n + 3] = v[nt].w;
        } else if (p.c_vec) {
#if ONSSEN_XQ_CSTORE == 1
          if (n < p.N) __builtin_nontemporal_store(f32x4{v[nt].x, v[nt].y, v[nt].z, v[nt].w}, reinterpret_cast<f32x4*>(crow + n));
#elif ONSSEN_XQ_CSTORE == 2      // write-through (sc1): nothing of C is left dirty in the L2 for the end-of-kernel write-back
          if (n < p.N) {
            const f32x4 vv = f32x4{v[nt].x, v[nt].y, v[nt].z, v[nt].w};
            asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(crow + n), "v"(vv) : "memory");
          }
#else
          if (n < p.N) *reinterpret_cast<float4*>(crow + n) = v[nt];
#endif
        } else {
          if (n + 0 < p.N) crow[n + 0] = v[nt].x;
          if (n + 1 < p.N) crow[n + 1] = v[nt].y;
          if (n + 2 < p.N) crow[n + 2] = v[nt].z;
          if (n + 3 < p.N) crow[n + 3] = v[nt].w;
        }
      }
    }
  }
}

// linear_x3r_kernel (round 6c): linear_x3q_kernel's tiles, staging and tile order with v_mfma_f32_32x32x16_bf16 instead of 16x16x32 -- the
// 32 x 32 instruction sustains 2 382 TF against 2 075 (cdna_hip_programming.md, MFMA microbenchmarks: the 16 x 16 form pays an issue bubble
// per instruction), at the same operand bytes per FLOP.  Plain bias epilogue only (the projections; onssen_linear_x3p with ONSSEN_EPI_BIAS).
// Waves 4 (M) x 2 (N): wave tile (BM / 4) x (BN / 2) = MT x NT tiles of 32 x 32, A operand = W (the accumulator's rows are features: a
// lane holds, per tile, four runs of four consecutive features -- n = 8 q + 4 (lane >> 5) + {0..3}, q = 0..3 -- of activation row
// lane & 31).  The fp32 sums are formed in another order than the 16 x 16 kernel's (16 k per instruction instead of 32): last-bit
// differences against it, so EVERY tile shape of the bias mode runs here (a row's bits must not depend on the batch it sits in).
typedef float f32x16 __attribute__((vector_size(64)));
__device__ __forceinline__ f32x16 mfma32_bf16(s16x8 a, s16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}
template <int TERMS, int BN = 320, int BM = 256>
__global__ __launch_bounds__(512) void linear_x3r_kernel(LinearXpArgs p) {
  constexpr int STAGE = (BM + BN) * 128;
  constexpr int NQW = (BM + BN) / 64;                 // LDS-DMA instructions per wave and k-step
  constexpr int WM = BM / 4, WN = BN / 2;             // wave tile
  constexpr int MT = WM / 32, NT = WN / 32;
  __shared__ __attribute__((aligned(1024))) unsigned char stage0[STAGE];
  __shared__ __attribute__((aligned(1024))) unsigned char stage1[STAGE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int r32 = lane & 31, kh = lane >> 5;
  int n0, m0;
  {   // XCD-aware tile order: as linear_x3q_kernel
    const int nbx = gridDim.x, nwg = nbx * gridDim.y, bid = blockIdx.y * nbx + blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    const int GN = p.tile_group, nby = gridDim.y;
    const int gfull = nbx / GN, nfull = gfull * GN * nby;
    int tn, tm;
    if (wg < nfull) {
      const int rem = wg % (nby * GN);
      tn = (wg / (nby * GN)) * GN + rem % GN;
      tm = rem / GN;
    } else {
      const int gl = nbx - gfull * GN, rem = wg - nfull;
      tn = gfull * GN + rem % gl;
      tm = rem / gl;
    }
    n0 = tn * BN;
    m0 = tm * BM;
  }
  const int pitch = p.KB * 128;
  const int a_rows = p.M - m0 < BM ? p.M - m0 : BM, w_rows = p.N - n0 < BN ? p.N - n0 : BN;
  const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)(p.A + (long)m0 * p.KB * 64), 0, a_rows * pitch, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)(p.W + (long)n0 * p.KB * 64), 0, w_rows * pitch, 0x00020000);
  const unsigned dma_lane = (unsigned)((lane >> 3) * pitch + (((lane & 7) ^ (lane >> 3)) * 16));
  auto dma = [&](unsigned char* stage, int kb) {
    const unsigned koff = (unsigned)(kb * 128);
#pragma unroll
    for (int j = 0; j < NQW; ++j) {
      const int q = wave * NQW + j;
      if (q < BM / 8)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, ONSSEN_LDS_PTR(stage + q * 1024), 16, dma_lane + (unsigned)(q * 8 * pitch) + koff, 0, 0, 0);
      else
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, ONSSEN_LDS_PTR(stage + q * 1024), 16, dma_lane + (unsigned)((q - BM / 8) * 8 * pitch) + koff, 0, 0, 0);
    }
  };
  f32x16 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[mt][nt][j] = 0.f;
  // a lane's fragments: image row (tile row & 31 = r32), 8 consecutive k of the 16-k slab s: global chunk 2 s + kh (hi), + 4 (lo);
  // LDS slot = chunk ^ (row & 7)
  const unsigned fa_off = (unsigned)((wm * WM + r32) * 128);                  // + mt * 32 * 128
  const unsigned fw_off = (unsigned)((BM + wn * WN + r32) * 128);             // + nt * 32 * 128
  auto compute = [&](const unsigned char* sb) {
#pragma unroll
    for (int sl = 0; sl < 2; ++sl) {
      const unsigned ch = (unsigned)((((2 * sl + kh) ^ (r32 & 7))) * 16), cl = ch ^ 64u;
      s16x8 wh[NT], wl[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        wh[nt] = *reinterpret_cast<const s16x8*>(sb + fw_off + nt * 4096 + ch);
        wl[nt] = TERMS == 3 ? *reinterpret_cast<const s16x8*>(sb + fw_off + nt * 4096 + cl) : wh[nt];
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const s16x8 xh = *reinterpret_cast<const s16x8*>(sb + fa_off + mt * 4096 + ch);
        const s16x8 xl = TERMS == 3 ? *reinterpret_cast<const s16x8*>(sb + fa_off + mt * 4096 + cl) : xh;
        if constexpr (TERMS == 3) {      // small terms first, NT independent accumulators between two MFMAs on the same one
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = mfma32_bf16(wh[nt], xl, acc[mt][nt]);
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = mfma32_bf16(wl[nt], xh, acc[mt][nt]);
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = mfma32_bf16(wh[nt], xh, acc[mt][nt]);
      }
    }
  };
  const int nkb = p.KB;
  dma(stage0, 0);
  __builtin_amdgcn_s_waitcnt(0x0F70);
  __syncthreads();
  for (int kb = 0; kb < nkb; kb += 2) {
    if (kb + 1 < nkb) dma(stage1, kb + 1);
    compute(stage0);
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __syncthreads();
    if (kb + 1 < nkb) {
      if (kb + 2 < nkb) dma(stage0, kb + 2);
      compute(stage1);
      __builtin_amdgcn_s_waitcnt(0x0F70);
      __syncthreads();
    }
  }
  // ---- epilogue: + bias, 16-byte stores (four consecutive features of one activation row)
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = m0 + wm * WM + mt * 32 + r32;
    if (m >= p.M) continue;
    float* crow = p.C + (long)(m / p.R) * p.c_s0 + (long)(m % p.R) * p.c_s1;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = n0 + wn * WN + nt * 32 + 8 * q + 4 * kh;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = acc[mt][nt][4 * q + j] + (n + j < p.N ? p.bias[n + j] : 0.f);
        if (p.c_vec) {
          if (n < p.N) *reinterpret_cast<float4*>(crow + n) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (n + j < p.N) crow[n + j] = v[j];
        }
      }
  }
}

// fp32 rows (row m at src + (m / R)*s0 + (m % R)*s1, K contiguous) -> x3 image [rows][KB][2][32]
// One thread per 8 consecutive k of a row: two 16-byte reads where the row allows it, one 16-byte store per plane (round 4; one
// element per thread with two 2-byte stores took 64 us for the 123 MB of a layer's dP).
__global__ __launch_bounds__(256) void x3_image_kernel(const float* __restrict__ src, long s0, long s1, int R, int rows, int K, int KB,
                                                       unsigned short* __restrict__ img) {
  const long total = (long)rows * KB * 4;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int q = (int)(e & 3);
    const long rb = e >> 2;                       // row * KB + kblock
    const int m = (int)(rb / KB), k0 = (int)(rb % KB) * 32 + q * 8;
    const float* row = src + (long)(m / R) * s0 + (long)(m % R) * s1;
    float v[8];
    if (k0 + 8 <= K && (reinterpret_cast<uintptr_t>(row + k0) & 15u) == 0) {
      const float4 a = *reinterpret_cast<const float4*>(row + k0), b = *reinterpret_cast<const float4*>(row + k0 + 4);
      v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = k0 + j < K ? row[k0 + j] : 0.0f;
    }
    unsigned short hi[8], lo[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) split_bf16(v[j], hi[j], lo[j]);
    u32x4 h4, l4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      h4[j] = (unsigned)hi[2 * j] | ((unsigned)hi[2 * j + 1] << 16);
      l4[j] = (unsigned)lo[2 * j] | ((unsigned)lo[2 * j + 1] << 16);
    }
    *reinterpret_cast<u32x4*>(img + rb * 64 + q * 8) = h4;
    *reinterpret_cast<u32x4*>(img + rb * 64 + 32 + q * 8) = l4;
  }
}

// x3 image of the TRANSPOSE of a row-major fp32 matrix, with an optional shift along k: image row m, element k =
// src[(k + k_shift) * ld + m] (0 where k + k_shift falls outside [0, K)).  The weight-gradient GEMMs of the training
// path contract over the T*B rows of row-major activations (dP^T x): this writes their operands without a
// transposed fp32 copy, and the shift by +-B rows turns y into "h of the step before" for either direction.
// Both x3 images of a row-major [K][M] fp32 matrix in ONE pass over it (the training path's dP: the input-gradient GEMM
// contracts over its columns -- row-major image [K][ceil(M/32)][2][32] --, the weight-gradient GEMM over its rows -- transposed
// image [M][ceil(K/32)][2][32]): the same 32 x 64 tile, read once, split once per use.
// colsum (or null): [KB][M] partial column sums of the tile's 32 rows -- the bias gradient of the layer whose output gradient
// this matrix is (its sum over k blocks, in block order, is the column sum of src: no separate pass over src)
__global__ __launch_bounds__(256) void x3_image_both_kernel(const float* __restrict__ src, long ld, int M, int K, int KB, int MB,
                                                            unsigned short* __restrict__ img_rows,
                                                            unsigned short* __restrict__ img_t, float* __restrict__ colsum) {
  __shared__ float tile[32][65];
  const int tid = threadIdx.x, m0 = blockIdx.x * 64, kb = blockIdx.y;
  {
    const int r = tid >> 6, c = tid & 63, m = m0 + c;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int kk = r + 4 * i, k = kb * 32 + kk;
      tile[kk][c] = (m < M && k < K) ? src[(long)k * ld + m] : 0.0f;
    }
  }
  __syncthreads();
  if (colsum && tid < 64 && m0 + tid < M) {
    float s = 0.f;
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) s += tile[kk][tid];
    colsum[(long)kb * M + m0 + tid] = s;
  }
  auto pack8 = [&](const float (&v)[8], unsigned short* d) {
    unsigned short hi[8], lo[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) split_bf16(v[j], hi[j], lo[j]);
    u32x4 h4, l4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      h4[j] = (unsigned)hi[2 * j] | ((unsigned)hi[2 * j + 1] << 16);
      l4[j] = (unsigned)lo[2 * j] | ((unsigned)lo[2 * j + 1] << 16);
    }
    *reinterpret_cast<u32x4*>(d) = h4;
    *reinterpret_cast<u32x4*>(d + 32) = l4;
  };
  {   // transposed image: row m, k block kb
    const int ml = tid >> 2, q = tid & 3, m = m0 + ml;
    if (m < M) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = tile[q * 8 + j][ml];
      pack8(v, img_t + ((long)m * KB + kb) * 64 + q * 8);
    }
  }
  {   // row-major image: row k, the two 32-column blocks of this tile (zeros beyond M)
    const int kk = tid >> 3, c8 = (tid & 7) * 8, k = kb * 32 + kk, mb = (m0 + c8) >> 5;
    if (k < K && mb < MB) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = tile[kk][c8 + j];
      pack8(v, img_rows + ((long)k * MB + mb) * 64 + (c8 & 31));
    }
  }
}

// One 32 (k) x 64 (m) tile per workgroup through LDS: coalesced 256-byte reads, 16-byte writes.
__global__ __launch_bounds__(256) void x3_image_t_kernel(const float* __restrict__ src, long ld, int M, int K, int KB,
                                                         int k_shift, unsigned short* __restrict__ img) {
  __shared__ float tile[32][65];
  const int tid = threadIdx.x, m0 = blockIdx.x * 64, kb = blockIdx.y;
  {
    const int r = tid >> 6, c = tid & 63, m = m0 + c;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int kk = r + 4 * i, k = kb * 32 + kk, ks = k + k_shift;
      tile[kk][c] = (m < M && k < K && ks >= 0 && ks < K) ? src[(long)ks * ld + m] : 0.0f;
    }
  }
  __syncthreads();
  const int ml = tid >> 2, q = tid & 3, m = m0 + ml;
  if (m < M) {
    unsigned short hi[8], lo[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) split_bf16(tile[q * 8 + j][ml], hi[j], lo[j]);
    unsigned short* d = img + ((long)m * KB + kb) * 64 + q * 8;
    u32x4 h4, l4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      h4[j] = (unsigned)hi[2 * j] | ((unsigned)hi[2 * j + 1] << 16);
      l4[j] = (unsigned)lo[2 * j] | ((unsigned)lo[2 * j + 1] << 16);
    }
    *reinterpret_cast<u32x4*>(d) = h4;
    *reinterpret_cast<u32x4*>(d + 32) = l4;
  }
}
