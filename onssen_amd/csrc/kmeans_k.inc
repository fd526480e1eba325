// Deep-clustering back end for K = 2 .. 4 speakers (part of onssen_hip.hip): threshold, farthest-point initialisation, Lloyd
// iterations and K-channel binary masks over the embedding slab (B, T*F, D), D <= 32.
// (egs/wsj0-2mix/deep_clustering/evaluate.py:33-44: num_spk from sig_ref, KMeans(n_clusters=num_spk), num_spk masks)
// =================================================================================================
// The launch-per-iteration form only: one assignment + partial-sum launch and one small update launch per iteration, then one
// mask launch.  No inter-workgroup waits, counters or spin loops, no float atomics; every workgroup leaves K(D+1) partial sums
// that are added in a fixed order, so two calls give the same bits.  The two-speaker kernels (labels_cluster.inc: kmeans2_*)
// are untouched; a persistent form and a compacted-row form for K > 2 do not exist (DESIGN.md section 18).
//
// The arithmetic, fixed so that tests/dc_kmeans_ref.py can restate it:
//   threshold   bin i of utterance b is active iff feature[i] >= max(feature over the utterance's own bins) - db / 20
//   init        c_0 = embedding of the loudest bin (first maximum); c_k = the active bin minimising max_{j<k} e.c_j (farthest
//               point on unit vectors), ties to the smallest bin index; no candidate: c_k = c_0
//   iteration   label = argmin_k |c_k|^2 - 2 e.c_k (ties to the smallest k); new centroid = mean of its bins, an empty cluster
//               keeps its centroid; stop at the bitwise fixed point, by sklearn's rule (kmeans2_update_kernel: summed squared
//               shift <= tol x (1 - |mean|^2) / D) or after `iters` iterations
//   masks       (B, T, F, K): channel k = 1 where the bin is active and its label under the final centroids is k; cluster k is
//               the one grown from c_k
// Workspace: [B][kmk::INFO] int32 (iterations run, converged, loudest bin, -) | 256-byte aligned: [B][stride] floats, per
// utterance [0] feature max, [1 .. K D] centroids, then kmk::NB x K x (D + 1) partial sums (first the searches' scratch).
namespace kmk {
#ifdef ONSSEN_HOST_EMULATION
constexpr int NB = 2, KT = 64;     // the host-side emulation runs every work-item as an OS thread: same code, smaller launch
#else
constexpr int NB = 64;             // workgroups per utterance of the search and assignment launches
constexpr int KT = 256;            // threads per workgroup: one bin per thread and tile
#endif
constexpr int KMAX = 4, DMAX = 32;
constexpr int INFO = 4;            // int32 words per utterance in front of the float headers
static inline long stride(int D, int K) { return 1 + (long)K * D + (long)NB * K * (D + 1); }
}

// one row of D floats into registers: 16-byte loads when the rows are 16-byte multiples (D % 4 == 0), else scalar loads (rare
// widths; the lines are shared by neighbouring lanes through the vector L1)
template <int DT>
__device__ __forceinline__ void kmeansk_load_row(const float* __restrict__ row, int D, float (&v)[DT ? DT : kmk::DMAX]) {
  constexpr int DC = DT ? DT : kmk::DMAX;
  if ((DT && (DT % 4) == 0) || (!DT && (D & 3) == 0)) {
    const float4* src = reinterpret_cast<const float4*>(row);
#pragma unroll
    for (int q = 0; q < DC / 4; ++q) {
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
      if (DT || 4 * q < D) x = src[q];
      v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w;
    }
  } else {
#pragma unroll
    for (int d = 0; d < DC; ++d) v[d] = d < D ? row[d] : 0.f;
  }
}

// Searches of the initialisation, kmk::NB workgroups per utterance, each over one contiguous chunk of the utterance's own bins:
//   kc == 0: argmax of the feature (the first maximum)
//   kc >= 1: argmin over the active bins of max_{j < kc} e.c_j (ties to the smallest bin index)
// A workgroup leaves (value, index) in the partial-sum area; kmeansk_pick_kernel takes the winner.
__global__ __launch_bounds__(kmk::KT) void kmeansk_search_kernel(const float* __restrict__ emb, const float* __restrict__ feat,
                                                                 long per_utt, int D, int K, int kc, float db,
                                                                 float* __restrict__ ws, long ws_stride,
                                                                 const int* __restrict__ frames, int F) {
  using namespace kmk;
  __shared__ float rv[KT];
  __shared__ int ri[KT];
  __shared__ float cen[(KMAX - 1) * DMAX];
  const int b = blockIdx.y, tid = threadIdx.x;
  const long nb = frames ? (long)frames[b] * F : per_utt;      // ragged batch: the padding takes no part
  const float* f = feat + (long)b * per_utt;
  const float* e = emb + (long)b * per_utt * D;
  float* w = ws + (long)b * ws_stride;
  float* part = w + 1 + K * D;
  const long chunk = (nb + NB - 1) / NB, i_lo = (long)blockIdx.x * chunk, i_hi = i_lo + chunk < nb ? i_lo + chunk : nb;
  for (int k = tid; k < kc * D; k += KT) cen[k] = w[1 + k];
  __syncthreads();
  const float thr = kc ? w[0] - db / 20.0f : 0.f;
  float best = kc ? INFINITY : -INFINITY;
  int bi = -1;                                       // "none"
  for (long i = i_lo + tid; i < i_hi; i += KT) {     // (a lane's bins ascend: a strict comparison keeps the first)
    if (kc == 0) {
      if (f[i] > best) { best = f[i]; bi = (int)i; }
    } else if (f[i] >= thr) {
      float v[DMAX];
      kmeansk_load_row<0>(e + i * D, D, v);
      float m = -INFINITY;
      for (int j = 0; j < kc; ++j) {
        float dot = 0.f;
#pragma unroll
        for (int d = 0; d < DMAX; ++d)
          if (d < D) dot += v[d] * cen[j * D + d];
        m = fmaxf(m, dot);
      }
      if (m < best) { best = m; bi = (int)i; }
    }
  }
  rv[tid] = best; ri[tid] = bi;
  __syncthreads();
  for (int s = KT / 2; s > 0; s >>= 1) {
    if (tid < s) {
      const float v2 = rv[tid + s];
      const int i2 = ri[tid + s];
      const bool better = kc ? v2 < rv[tid] : v2 > rv[tid];
      if (i2 >= 0 && (ri[tid] < 0 || better || (v2 == rv[tid] && i2 < ri[tid]))) { rv[tid] = v2; ri[tid] = i2; }
    }
    __syncthreads();
  }
  if (tid == 0) {
    part[2 * blockIdx.x] = rv[0];
    part[2 * blockIdx.x + 1] = __builtin_bit_cast(float, ri[0]);    // per_utt < 2^31
  }
}

// one small workgroup per utterance: the winner of the kmk::NB partials becomes centroid kc.  kc == 0 also leaves the feature
// maximum and starts the call's bookkeeping afresh (iterations run, converged).
__global__ __launch_bounds__(64) void kmeansk_pick_kernel(const float* __restrict__ emb, long per_utt, int D, int K, int kc,
                                                          float* __restrict__ ws, long ws_stride, int* __restrict__ info) {
  using namespace kmk;
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* e = emb + (long)b * per_utt * D;
  float* w = ws + (long)b * ws_stride;
  int* nfo = info + (long)b * INFO;
  const float* part = w + 1 + K * D;
  __shared__ int pick;
  if (tid == 0) {
    float best = kc ? INFINITY : -INFINITY;
    int bi = -1;
    for (int k = 0; k < NB; ++k) {                   // chunks are in index order: a strict comparison keeps the first
      const float v = part[2 * k];
      const int i = __builtin_bit_cast(int, part[2 * k + 1]);
      if (i >= 0 && (bi < 0 || (kc ? v < best : v > best))) { best = v; bi = i; }
    }
    if (kc == 0) {
      w[0] = bi >= 0 ? best : -INFINITY;
      nfo[0] = 0; nfo[1] = 0; nfo[2] = bi; nfo[3] = 0;
    } else if (bi < 0) {
      bi = nfo[2];                                   // no candidate: c_k = c_0
    }
    pick = bi;
  }
  __syncthreads();
  for (int d = tid; d < D; d += 64) w[1 + kc * D + d] = pick >= 0 ? e[(long)pick * D + d] : 0.f;   // (an utterance without bins)
}

// assignment + per-workgroup partial sums (MODE 0), or assignment + mask write (MODE 1).  A workgroup walks tiles of kmk::KT
// bins, one bin per thread; a thread reads its row ONCE for the K distances and the centroid sums, so an iteration streams
// the embedding and the feature from HBM once: B T F (D + 1) 4 bytes.
// DT = compile-time embedding width (20, the reference's default): centroids, running sums and the row live in registers
// (K = 4: 80 + 84 + 20).  DT = 0 = run-time D <= DMAX: the centroids stay in the LDS (every lane reads the same word: a
// broadcast), which keeps K = 4, D = 32 at 132 running sums + 32 row values per lane, without scratch.
template <int MODE, int K, int DT>
__global__ __launch_bounds__(kmk::KT) void kmeansk_assign_kernel(const float* __restrict__ emb, const float* __restrict__ feat,
                                                                 long per_utt, int D_rt, float db, float* __restrict__ ws,
                                                                 long ws_stride, const int* __restrict__ info,
                                                                 float* __restrict__ masks, const int* __restrict__ frames, int F) {
  using namespace kmk;
  constexpr int DC = DT ? DT : DMAX;
  const int D = DT ? DT : D_rt;
  __shared__ float cen[K * DC];                                    // DT == 0: the centroids, zero beyond D
  __shared__ float red[MODE == 0 ? K * (DC + 1) * 64 : 1];         // the final reduction: [K (D + 1)][64]
  const int b = blockIdx.y, tid = threadIdx.x;
  const float* f = feat + (long)b * per_utt;
  const float* e = emb + (long)b * per_utt * D;
  float* w = ws + (long)b * ws_stride;
  if (MODE == 0 && info[(long)b * INFO + 1] != 0) return;          // converged: the whole workgroup leaves before any barrier
  const float thr = w[0] - db / 20.0f;
  float c[K][DC], s[K][DC], q[K], n[K];
  if constexpr (DT == 0) {
    for (int k = tid; k < K * DC; k += KT) cen[k] = (k % DC) < D ? w[1 + (k / DC) * D + (k % DC)] : 0.f;
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    q[k] = 0.f; n[k] = 0.f;
#pragma unroll
    for (int d = 0; d < DC; ++d) {
      c[k][d] = DT ? w[1 + k * D + d] : cen[k * DC + d];           // (DT == 0: only q needs it here; the rows read the LDS)
      q[k] += c[k][d] * c[k][d];
      s[k][d] = 0.f;
    }
  }
  // ragged batch: the sums run over the utterance's own nb bins; the mask pass also writes the (zero) masks of its padding
  const long nb = frames ? (long)frames[b] * F : per_utt, span = MODE == 1 ? per_utt : nb;
  const long ntiles = (span + KT - 1) / KT;
  for (long tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
    const long i = tl * KT + tid;
    if (i >= span) continue;
    const bool active = i < nb && f[i] >= thr;
    float v[DC];
    kmeansk_load_row<DT>(e + i * D, D, v);
    int lab = 0;
    float dbest = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float dk = q[k];                      // ||e - c||^2 = ||e||^2 - 2 e.c + ||c||^2 ; ||e||^2 is common
#pragma unroll
      for (int d = 0; d < DC; ++d) {
        if (DT) dk -= 2.f * v[d] * c[k][d];
        else if (d < D) dk -= 2.f * v[d] * cen[k * DC + d];
      }
      if (k == 0 || dk < dbest) { dbest = dk; lab = k; }           // ties go to the smallest k
    }
    if (MODE == 1) {
      float m[K];
#pragma unroll
      for (int k = 0; k < K; ++k) m[k] = (active && lab == k) ? 1.0f : 0.0f;
      float* dst = masks + ((long)b * per_utt + i) * K;
      if constexpr (K == 2) *reinterpret_cast<float2*>(dst) = make_float2(m[0], m[1]);
      else if constexpr (K == 4) *reinterpret_cast<float4*>(dst) = make_float4(m[0], m[1], m[2], m[3]);
      else { dst[0] = m[0]; dst[1] = m[1]; dst[2] = m[2]; }
    } else if (active) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const float sel = lab == k ? 1.f : 0.f;
#pragma unroll
        for (int d = 0; d < DC; ++d) s[k][d] += sel * v[d];
        n[k] += sel;
      }
    }
  }
  if (MODE == 0) {
    // the K (D + 1) accumulators of the workgroup's waves are added up in the LDS, wave after wave (a fixed order), into one
    // [column][64 lanes] array; thread k then adds up column k
    const int na = K * (D + 1), lane = tid & 63;
    float* out = w + 1 + K * D + (long)blockIdx.x * na;
#pragma unroll
    for (int wv = 0; wv < KT / 64; ++wv) {
      if ((tid >> 6) == wv) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
#pragma unroll
          for (int d = 0; d < DC; ++d) {
            if (d < D) {
              float* r = red + (k * (D + 1) + d) * 64 + lane;
              *r = wv ? *r + s[k][d] : s[k][d];
            }
          }
          float* r = red + (k * (D + 1) + D) * 64 + lane;
          *r = wv ? *r + n[k] : n[k];
        }
      }
      __syncthreads();
    }
    for (int col = tid; col < na; col += KT) {
      float acc = 0.f;
      for (int j = 0; j < 64; ++j) acc += red[col * 64 + ((j + col) & 63)];   // staggered start: no bank conflict
      out[col] = acc;
    }
  }
}

// new centroids from the workgroups' partial sums (added in workgroup order, four independent quarter-sums per column, as
// kmeans2_update_kernel does); counts the iteration; marks the utterance converged at the bitwise fixed point or by sklearn's
// rule -- its remaining assignment and update launches then return at once
__global__ __launch_bounds__(kmk::KT) void kmeansk_update_kernel(int D, int K, int nblk, float* __restrict__ ws, long ws_stride,
                                                                 int* __restrict__ info, float tol) {
  using namespace kmk;
  __shared__ int changed;
  __shared__ float shift_s[KMAX * DMAX];
  __shared__ float seg[KMAX * (DMAX + 1)][4];
  float* w = ws + (long)blockIdx.x * ws_stride;
  int* nfo = info + (long)blockIdx.x * INFO;
  const int tid = threadIdx.x, na = K * (D + 1);
  if (tid == 0) changed = 0;
  __syncthreads();
  if (nfo[1] != 0) return;                   // already converged (uniform over the workgroup)
  for (int t = tid; t < 4 * na; t += KT) {
    const int o = t >> 2, qq = t & 3, per = (nblk + 3) / 4;
    float sacc = 0.f;
    for (int j = qq * per; j < (qq + 1) * per && j < nblk; ++j) sacc += w[1 + K * D + (long)j * na + o];
    seg[o][qq] = sacc;
  }
  __syncthreads();
  for (int t = tid; t < K * D; t += KT) {
    const int k = t / D, d = t % D;
    const float* sd = seg[k * (D + 1) + d];
    const float* sn = seg[k * (D + 1) + D];
    const float ssum = (sd[0] + sd[1]) + (sd[2] + sd[3]), cnt = (sn[0] + sn[1]) + (sn[2] + sn[3]);
    float sh = 0.f;
    if (cnt > 0.f) {                         // an empty cluster keeps its centroid
      const float v = ssum / cnt, old = w[1 + k * D + d];
      if (v != old) changed = 1;
      sh = (v - old) * (v - old);
      w[1 + k * D + d] = v;
    }
    shift_s[t] = sh;
  }
  __syncthreads();
  if (tid == 0) {
    nfo[0] += 1;
    bool done = !changed;
    if (!done && tol > 0.f) {                // sklearn: center_shift_tot <= tol * mean(var(X, axis=0)); unit rows: (1 - |mean|^2) / D
      float shift = 0.f, m2 = 0.f, ntot = 0.f;
      for (int t = 0; t < K * D; ++t) shift += shift_s[t];
      for (int k = 0; k < K; ++k) {
        const float* sn = seg[k * (D + 1) + D];
        ntot += (sn[0] + sn[1]) + (sn[2] + sn[3]);
      }
      for (int d = 0; d < D; ++d) {
        float tot = 0.f;
        for (int k = 0; k < K; ++k) {
          const float* sd = seg[k * (D + 1) + d];
          tot += (sd[0] + sd[1]) + (sd[2] + sd[3]);
        }
        const float m = tot / ntot;
        m2 += m * m;
      }
      const float var = 1.0f - m2 > 0.f ? (1.0f - m2) / (float)D : 0.f;
      done = shift <= tol * var;
    }
    if (done) nfo[1] = 1;
  }
}

// ---- host side: the C ABI entries -------------------------------------------------------------------------------------------
size_t onssen_dc_cluster_k_workspace_bytes(int B, int T, int F, int D, int K) {
  if (B <= 0 || T <= 0 || F <= 0 || D <= 0 || D > kmk::DMAX || K < 2 || K > kmk::KMAX || (long)T * F >= (1L << 31)) return 0;
  return align256((size_t)B * kmk::INFO * sizeof(int32_t)) + (size_t)B * kmk::stride(D, K) * sizeof(float);
}

template <int K>
static void dc_cluster_k_launch(const float* emb, const float* feature, int B, long per_utt, const int32_t* frames, int F, int D,
                                float db, int iters, float tol, float* masks, float* w, int* info, hipStream_t st) {
  const long stride = kmk::stride(D, K);
  const dim3 grid(kmk::NB, (unsigned)B), one((unsigned)B);
  for (int kc = 0; kc < K; ++kc) {
    hipLaunchKernelGGL(kmeansk_search_kernel, grid, dim3(kmk::KT), 0, st, emb, feature, per_utt, D, K, kc, db, w, stride, frames, F);
    hipLaunchKernelGGL(kmeansk_pick_kernel, one, dim3(64), 0, st, emb, per_utt, D, K, kc, w, stride, info);
  }
#define ONSSEN_KMK_ASSIGN(MODE_, OUT_)                                                                                         \
  do {                                                                                                                       \
    if (D == 20) hipLaunchKernelGGL((kmeansk_assign_kernel<MODE_, K, 20>), grid, dim3(kmk::KT), 0, st, emb, feature, per_utt, D, \
                                    db, w, stride, (const int*)info, OUT_, frames, F);                                         \
    else hipLaunchKernelGGL((kmeansk_assign_kernel<MODE_, K, 0>), grid, dim3(kmk::KT), 0, st, emb, feature, per_utt, D, db, w,  \
                            stride, (const int*)info, OUT_, frames, F);                                                        \
  } while (0)
  for (int it = 0; it < iters; ++it) {
    ONSSEN_KMK_ASSIGN(0, (float*)nullptr);
    hipLaunchKernelGGL(kmeansk_update_kernel, one, dim3(kmk::KT), 0, st, D, K, kmk::NB, w, stride, info, tol);
  }
  ONSSEN_KMK_ASSIGN(1, masks);
#undef ONSSEN_KMK_ASSIGN
}

int onssen_dc_cluster_k_f32(const float* emb, const float* feature, int B, int T, const int32_t* frames, int F, int D, int K,
                            float db_threshold, int iters, float tol, float* masks, void* ws, size_t ws_bytes, void* stream) {
  const size_t need = onssen_dc_cluster_k_workspace_bytes(B, T, F, D, K);
  if (!emb || !feature || !masks || !ws || need == 0 || ws_bytes < need || iters < 0 || !(tol >= 0.f)) return ONSSEN_E_ARG;
  if (!aligned16(emb) || !aligned16(masks) || !aligned256(ws)) return ONSSEN_E_ALIGN;
  ONSSEN_CLEAR_ERROR();
  hipStream_t st = (hipStream_t)stream;
  int* info = (int*)ws;
  float* w = (float*)((char*)ws + align256((size_t)B * kmk::INFO * sizeof(int32_t)));
  const long per_utt = (long)T * F;
  if (K == 2) dc_cluster_k_launch<2>(emb, feature, B, per_utt, frames, F, D, db_threshold, iters, tol, masks, w, info, st);
  else if (K == 3) dc_cluster_k_launch<3>(emb, feature, B, per_utt, frames, F, D, db_threshold, iters, tol, masks, w, info, st);
  else dc_cluster_k_launch<4>(emb, feature, B, per_utt, frames, F, D, db_threshold, iters, tol, masks, w, info, st);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}
