// N3 training-label features and N2 deep-clustering back end (part of onssen_hip.hip).
// =================================================================================================
// N3: training-label features from the three complex STFTs (mix, s1, s2) of a chunk
// (onssen/data/feature_utils.py:77-95 get_cos_difference / get_one_hot, wsj0_2mix.py:130-152)
// =================================================================================================
__global__ void utt_max_kernel(const float* __restrict__ x, long per_utt, float* __restrict__ out) {
  __shared__ float red[256];
  const float* p = x + (long)blockIdx.x * per_utt;
  float m = -INFINITY;
  for (long i = threadIdx.x; i < per_utt; i += 256) m = fmaxf(m, p[i]);
  red[threadIdx.x] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

__global__ void labels_kernel(const float* __restrict__ mix, const float* __restrict__ s1, const float* __restrict__ s2,
                              const float* __restrict__ feat, const float* __restrict__ fmax, long per_utt, long total,
                              float db_threshold, float* __restrict__ one_hot, float* __restrict__ mag_mix,
                              float* __restrict__ mag_s1, float* __restrict__ mag_s2, float* __restrict__ cos_s1,
                              float* __restrict__ cos_s2) {
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const float xr = mix[2 * e], xi = mix[2 * e + 1];
    const float ar = s1[2 * e], ai = s1[2 * e + 1], br = s2[2 * e], bi = s2[2 * e + 1];
    const float m1 = hypotf(ar, ai), m2 = hypotf(br, bi);
    mag_mix[e] = hypotf(xr, xi);
    mag_s1[e] = m1;
    mag_s2[e] = m2;
    // np.argmax takes the first maximum: speaker 0 on ties; bins below max(feature) - dB/20 are silent (all-zero label)
    const bool active = !(feat[e] < fmax[e / per_utt] - db_threshold / 20.0f);
    const int who = (m2 > m1) ? 1 : 0;
    one_hot[2 * e] = (active && who == 0) ? 1.0f : 0.0f;
    one_hot[2 * e + 1] = (active && who == 1) ? 1.0f : 0.0f;
    if (cos_s1) {
      const float am = atan2f(xi, xr);
      cos_s1[e] = cosf(am - atan2f(ai, ar));
      cos_s2[e] = cosf(am - atan2f(bi, br));
    }
  }
}

// The reference's stand-alone helpers (onssen/data/feature_utils.py:49-51, 77-80, 83-95), one element per lane: what the fused
// kernels above / in fft.inc compute from inside a batch, for a caller that holds ONE utterance's arrays (feature_utils.py module
// of onssen_amd.data).  Same single-precision operations, in the same order, as the fused forms.
__global__ void log_magnitude_kernel(const float* __restrict__ ri, long total, float eps, float* __restrict__ out) {
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x)
    out[e] = log10f(hypotf(ri[2 * e], ri[2 * e + 1]) + eps);
}

__global__ void cos_difference_kernel(const float* __restrict__ a, const float* __restrict__ b, long total, float* __restrict__ out) {
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x)
    out[e] = cosf(atan2f(a[2 * e + 1], a[2 * e]) - atan2f(b[2 * e + 1], b[2 * e]));
}

__global__ void one_hot_kernel(const float* __restrict__ feat, const float* __restrict__ m1, const float* __restrict__ m2,
                               const float* __restrict__ fmax, long per_utt, long total, float db_threshold,
                               float* __restrict__ one_hot) {
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const bool active = !(feat[e] < fmax[e / per_utt] - db_threshold / 20.0f);
    const int who = (m2[e] > m1[e]) ? 1 : 0;        // np.argmax: the first maximum (speaker 0) on ties
    one_hot[2 * e] = (active && who == 0) ? 1.0f : 0.0f;
    one_hot[2 * e + 1] = (active && who == 1) ? 1.0f : 0.0f;
  }
}


// =================================================================================================
// N2: deep-clustering back end on the device -- 2-means over the embeddings of the active TF bins
// (egs/wsj0-2mix/deep_clustering/evaluate.py:36-41: threshold at max - 40/20, KMeans(n_clusters=2), binary masks)
// Deterministic: farthest-point initialisation, fixed iteration count, per-block partial sums reduced in a
// fixed order (no float atomics).  Workspace per utterance: [0] feature max, [1..2D] centroids,
// then NBLK x 2 x (D+1) partial sums.
// =================================================================================================
namespace km {
constexpr int NBLK = 64, DMAX = 32;
#ifdef ONSSEN_HOST_EMULATION
constexpr int NBP = 4, LT = 128;   // the host-side emulation runs every work-item as an OS thread: same code, smaller launch
#else
constexpr int NBP = 8;     // workgroups (of LT threads) per utterance of the persistent Lloyd kernel, all on one XCD
constexpr int LT = 512;    // one workgroup per CU (up to 256 VGPRs per lane): a lane keeps 5 rows in registers, 8 x 512 x 5 = 20 480
                           // rows per utterance never leave the register file; 32 utterances (256 workgroups) per launch
#endif
constexpr int IW = 72;     // int words per utterance next to the float header: [0..63] active bins per chunk, [64] their total,
                           // [65] start-up arrivals of the Lloyd kernel, [66] iterations it ran (| 0x10000 converged, | 0x20000 parts on
                           // several XCDs), [67] / [68] max(xcc + 1) / max(16 - xcc) of its parts
}

// Initialisation: c0 = embedding of the loudest bin, c1 = active embedding farthest from c0 (smallest dot product);
// ties go to the smallest bin index.  Two argmin/argmax searches over the utterance, each NBLK workgroups wide
// (partial (value, index) pairs per block, then one small workgroup per utterance), instead of one workgroup scanning
// 51 600 bins twice.
//   PHASE 0: argmax of the feature          -> partial[blk] ; PHASE 1: argmin of e[i].c0 over active bins -> partial[blk]
// (the compacted form, onssen_dc_cluster_compact_f32, needs PHASE 0 only: its farthest-point search rides in the Lloyd launch)
template <int PHASE>
__global__ __launch_bounds__(256) void kmeans2_search_kernel(const float* __restrict__ emb, const float* __restrict__ feat,
                                                             long per_utt, int D, float db, float* __restrict__ ws,
                                                             long ws_stride, const int* __restrict__ frames, int F) {
  using namespace km;
  __shared__ float rv[256];
  __shared__ long ri[256];
  const int b = blockIdx.y, tid = threadIdx.x;
  // ragged batch: utterance b owns the first frames[b] * F bins of its per_utt-bin slab (the padding takes no part)
  const long nb = frames ? (long)frames[b] * F : per_utt;
  const float* f = feat + (long)b * per_utt;
  const float* e = emb + (long)b * per_utt * D;
  float* w = ws + (long)b * ws_stride;
  float* part = w + 1 + 2 * D;                       // scratch of the search: [NBLK][2] (value, index as float bits)
  const long chunk = (nb + NBLK - 1) / NBLK, i_lo = (long)blockIdx.x * chunk, i_hi = i_lo + chunk < nb ? i_lo + chunk : nb;
  float best = PHASE == 0 ? -INFINITY : INFINITY;
  long bi = per_utt;                                 // "none"
  const float thr = PHASE == 1 ? w[0] - db / 20.0f : 0.f;
  float c0[DMAX];
#pragma unroll
  for (int d = 0; d < DMAX; ++d) c0[d] = (PHASE == 1 && d < D) ? w[1 + d] : 0.f;
  const bool vec = (D % 4) == 0;                     // rows are 16-byte multiples
  for (long i = i_lo + tid; i < i_hi; i += 256) {
    if (PHASE == 0) {
      if (f[i] > best) { best = f[i]; bi = i; }
    } else if (f[i] >= thr) {
      float dot = 0.0f;
      if (vec) {
        const float4* src = reinterpret_cast<const float4*>(e + i * D);
#pragma unroll
        for (int q = 0; q < DMAX / 4; ++q) {
          if (4 * q < D) {
            const float4 x = src[q];
            dot += x.x * c0[4 * q] + x.y * c0[4 * q + 1] + x.z * c0[4 * q + 2] + x.w * c0[4 * q + 3];
          }
        }
      } else {
#pragma unroll
        for (int d = 0; d < DMAX; ++d)
          if (d < D) dot += e[i * D + d] * c0[d];
      }
      if (dot < best) { best = dot; bi = i; }
    }
  }
  rv[tid] = best; ri[tid] = bi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      const bool better = PHASE == 0 ? rv[tid + s] > rv[tid] : rv[tid + s] < rv[tid];
      if (better || (rv[tid + s] == rv[tid] && ri[tid + s] < ri[tid])) { rv[tid] = rv[tid + s]; ri[tid] = ri[tid + s]; }
    }
    __syncthreads();
  }
  if (tid == 0) {
    part[2 * blockIdx.x] = rv[0];
    part[2 * blockIdx.x + 1] = __builtin_bit_cast(float, (int)ri[0]);    // per_utt < 2^31
  }
}

// one small workgroup per utterance: pick the winner of the NBLK partials, copy its embedding into the centroid
template <int PHASE>
__global__ void kmeans2_pick_kernel(const float* __restrict__ emb, long per_utt, int D, float* __restrict__ ws, long ws_stride,
                                    int* __restrict__ iw) {
  using namespace km;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (PHASE == 0 && iw && tid < 8) iw[(long)b * IW + 64 + tid] = 0;      // active count, Lloyd barrier: a fresh start every call
  const float* e = emb + (long)b * per_utt * D;
  float* w = ws + (long)b * ws_stride;
  const float* part = w + 1 + 2 * D;
  __shared__ long pick;
  if (tid == 0) {
    float best = PHASE == 0 ? -INFINITY : INFINITY;
    long bi = per_utt;
    for (int k = 0; k < NBLK; ++k) {                  // blocks are in index order: strict comparison keeps the first
      const float v = part[2 * k];
      const long i = (long)__builtin_bit_cast(int, part[2 * k + 1]);
      if (i < per_utt && (PHASE == 0 ? v > best : v < best)) { best = v; bi = i; }
    }
    if (PHASE == 0) w[0] = best;
    if (PHASE == 1) {
      if (bi >= per_utt) bi = (long)__builtin_bit_cast(int, w[ws_stride - 1]);   // no active bin besides i0: c1 = c0
      w[ws_stride - 1] = 0.0f;                        // not converged yet (the slot carried i0 between the phases)
    } else {
      w[ws_stride - 1] = __builtin_bit_cast(float, (int)bi);
    }
    pick = bi;
  }
  __syncthreads();
  if (emb) for (int d = tid; d < D; d += blockDim.x) w[1 + PHASE * D + d] = e[pick * D + d];   // (compacted form, PHASE 0: kmeans2_c0_kernel)
  // the scratch of the searches becomes the Lloyd kernel's two slots of tagged partial sums: every word starts with tag 1
  // (bit 0), which is what its first iteration does not expect
  if (PHASE == 1)
    for (int k = tid; k < 2 * NBP * 2 * (D + 1); k += blockDim.x) w[1 + 2 * D + k] = __builtin_bit_cast(float, 1u);
}

// assignment + per-block partial sums (MODE 0), or assignment + mask write (MODE 1).  A workgroup walks tiles of 256
// bins, one bin per thread; a thread reads its D values ONCE (D/4 16-byte loads when the rows are 16-byte multiples,
// else through a coalesced LDS tile) for the distance test and the centroid sums, so the embedding is streamed from
// HBM once per iteration.
// DT = compile-time embedding width (20, the reference's default) or 0 = run-time D <= DMAX.
template <int MODE, int DT>
__global__ __launch_bounds__(256) void kmeans2_assign_kernel(const float* __restrict__ emb, const float* __restrict__ feat,
                                                             long per_utt, int D_rt, float db, float* __restrict__ ws,
                                                             long ws_stride, float* __restrict__ masks,
                                                             const int* __restrict__ frames, int F) {
  using namespace km;
  constexpr int DC = DT ? DT : DMAX;             // register arrays / unrolled loops
  const int D = DT ? DT : D_rt;
  const int LD = D + 1;
  __shared__ float buf[(MODE == 0 ? 2 : 1) * (DC + 1) * 256];   // tile [256][D+1]; afterwards the partial sums [2(D+1)][256]
  const int b = blockIdx.y, tid = threadIdx.x;
  const float* f = feat + (long)b * per_utt;
  const float* e = emb + (long)b * per_utt * D;
  float* w = ws + (long)b * ws_stride;
  if (MODE == 0 && w[ws_stride - 1] != 0.0f) return;   // converged: the whole workgroup leaves before any barrier
  const float thr = w[0] - db / 20.0f;
  float c0[DC], c1[DC], s0[DC], s1[DC];
  float n0 = 0.f, n1 = 0.f, q0 = 0.f, q1 = 0.f;
#pragma unroll
  for (int d = 0; d < DC; ++d) {
    c0[d] = d < D ? w[1 + d] : 0.f; c1[d] = d < D ? w[1 + D + d] : 0.f;
    q0 += c0[d] * c0[d]; q1 += c1[d] * c1[d];
    s0[d] = 0.f; s1[d] = 0.f;
  }
  // ragged batch: the sums run over the utterance's own nb bins; the mask pass also writes the (zero) masks of its padding
  const long nb = frames ? (long)frames[b] * F : per_utt, span = MODE == 1 ? per_utt : nb;
  const long ntiles = (span + 255) / 256;
  for (long tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
    const long r0 = tl * 256;
    const int nr = span - r0 < 256 ? (int)(span - r0) : 256;
    constexpr bool kDirect = DT && (DT % 4) == 0;   // rows are 16-byte multiples: every thread reads its own row with
                                                    // DT/4 float4 loads (the lines come in once; no LDS round trip)
    if (!kDirect) {
      __syncthreads();
      for (int k = tid; k < nr * D; k += 256) buf[(k / D) * LD + (k % D)] = e[r0 * D + k];
      __syncthreads();
    }
    if (tid < nr) {
      const long i = r0 + tid;
      const bool active = i < nb && f[i] >= thr;
      float v[DC];
      if (kDirect) {
        const float4* src = reinterpret_cast<const float4*>(e + i * D);
#pragma unroll
        for (int q = 0; q < DC / 4; ++q) {
          const float4 x = src[q];
          v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w;
        }
      } else {
#pragma unroll
        for (int d = 0; d < DC; ++d) v[d] = d < D ? buf[tid * LD + d] : 0.f;
      }
      float d0 = q0, d1 = q1;               // ||e - c||^2 = ||e||^2 - 2 e.c + ||c||^2 ; ||e||^2 is common
#pragma unroll
      for (int d = 0; d < DC; ++d) {
        d0 -= 2.f * v[d] * c0[d];
        d1 -= 2.f * v[d] * c1[d];
      }
      const int lab = (active && d1 < d0) ? 1 : 0;
      if (MODE == 1) {
        *reinterpret_cast<float2*>(masks + 2 * ((long)b * per_utt + i)) =
            make_float2(active ? (float)lab : 0.0f, active ? (float)(1 - lab) : 0.0f);   // mask[0] = label, mask[1] = 1 - label
      } else if (active) {
        const float sel = (float)lab;
#pragma unroll
        for (int d = 0; d < DC; ++d) { s1[d] += sel * v[d]; s0[d] += (1.f - sel) * v[d]; }
        n1 += sel;
        n0 += 1.f - sel;
      }
    }
  }
  if (MODE == 0) {
    // all 2(D+1) accumulators go to LDS at once (the tile is no longer needed); thread k then adds up column k
    float* out = w + 1 + 2 * D + (long)blockIdx.x * 2 * (D + 1);
    const int na = 2 * (D + 1);
    __syncthreads();
#pragma unroll
    for (int d = 0; d < DC; ++d) {
      if (d < D) {
        buf[d * 256 + tid] = s0[d];
        buf[(D + 1 + d) * 256 + tid] = s1[d];
      }
    }
    buf[D * 256 + tid] = n0;
    buf[(2 * D + 1) * 256 + tid] = n1;
    __syncthreads();
    if (tid < na) {
      float acc = 0.f;
      for (int j = 0; j < 256; ++j) acc += buf[tid * 256 + ((j + tid) & 255)];   // staggered start: no bank conflict
      out[tid] = acc;
    }
  }
}

// new centroids; if none of the 2D values changed (bitwise) the assignment is at its fixed point: every further
// iteration would reproduce it exactly, so the utterance is marked done and its remaining assign launches return at once
// `tol` is sklearn's stopping rule (KMeans(tol=1e-4), the reference's default: evaluate.py:38): the iterations also stop once the
// squared shift of the two centroids, summed, is <= tol x the mean per-feature variance of the clustered rows.  The rows are unit
// vectors (F.normalize, onssen/nn/deep_clustering.py:41), so that variance is (1 - |mean|^2) / D and needs the totals only.
__global__ __launch_bounds__(256) void kmeans2_update_kernel(int D, int nblk, float* __restrict__ ws, long ws_stride, float tol) {
  __shared__ int changed;
  __shared__ float shift_s[2 * km::DMAX];
  __shared__ float seg[2 * (km::DMAX + 1)][4];
  float* w = ws + (long)blockIdx.x * ws_stride;
  const int tid = threadIdx.x, na = 2 * (D + 1);
  if (tid == 0) changed = 0;
  __syncthreads();
  if (w[ws_stride - 1] != 0.0f) return;      // already converged (uniform over the workgroup)
  // 2(D+1) column sums over the blocks' partials, four independent quarter-sums each (a single chain of nblk dependent
  // L2 reads is what this kernel's time used to be)
  if (tid < 4 * na) {
    const int o = tid >> 2, q = tid & 3, per = (nblk + 3) / 4;
    float sacc = 0.f;
    for (int j = q * per; j < (q + 1) * per && j < nblk; ++j) sacc += w[1 + 2 * D + (long)j * na + o];
    seg[o][q] = sacc;
  }
  __syncthreads();
  if (tid < 2 * D) {
    const int c = tid / D, d = tid % D;
    const float* sd = seg[c * (D + 1) + d];
    const float* sn = seg[c * (D + 1) + D];
    const float ssum = (sd[0] + sd[1]) + (sd[2] + sd[3]), n = (sn[0] + sn[1]) + (sn[2] + sn[3]);
    float sh = 0.f;
    if (n > 0.f) {                           // an empty cluster keeps its centroid
      const float v = ssum / n, old = w[1 + c * D + d];
      if (v != old) changed = 1;
      sh = (v - old) * (v - old);
      w[1 + c * D + d] = v;
    }
    shift_s[tid] = sh;
  }
  __syncthreads();
  if (tid == 0) {
    bool done = !changed;
    if (!done && tol > 0.f) {                // sklearn: center_shift_tot <= tol * mean(var(X, axis=0))
      float shift = 0.f, m2 = 0.f;
      const float ntot = ((seg[D][0] + seg[D][1]) + (seg[D][2] + seg[D][3])) + ((seg[2 * D + 1][0] + seg[2 * D + 1][1]) + (seg[2 * D + 1][2] + seg[2 * D + 1][3]));
      for (int k = 0; k < 2 * D; ++k) shift += shift_s[k];
      for (int d = 0; d < D; ++d) {
        const float* a = seg[d];
        const float* b2 = seg[D + 1 + d];
        const float m = (((a[0] + a[1]) + (a[2] + a[3])) + ((b2[0] + b2[1]) + (b2[2] + b2[3]))) / ntot;
        m2 += m * m;
      }
      const float var = 1.0f - m2 > 0.f ? (1.0f - m2) / (float)D : 0.f;
      done = shift <= tol * var;
    }
    if (done) w[ws_stride - 1] = 1.0f;
  }
}


// ---- round 3: the Lloyd iterations on a COMPACTED copy of the active bins, in ONE persistent launch ------------------------
// Only the bins within `db` of the utterance's loudest bin take part (evaluate.py:36): typically a third to a half of them.
// Twenty passes over all 132 MB of embeddings (B = 32) plus forty launches were 0.68 ms; instead
//   kmeans2_count_kernel    active bins per chunk (64 chunks per utterance)
//   kmeans2_compact_kernel  order-preserving copy of the active rows into a dense [n_active][D] array per utterance (positions
//                           = chunk base + an in-block scan); the same pass finds the farthest-point second centroid
//   kmeans2_lloyd_kernel    ALL iterations: NBP workgroups per utterance stream their share of the compacted rows (2-5 MB per
//                           utterance: served by the L2 / Infinity Cache after the first pass), leave 2(D+1) partial sums each,
//                           meet at a counter; the last one to arrive adds the partials in part order (bitwise reproducible),
//                           writes the centroids and bumps the generation the others poll.  An utterance whose assignment
//                           has reached its exact fixed point stops.  Every wait is bounded (status word; the host then runs the
//                           launch-per-iteration form above, which has no inter-workgroup waits).
// PICK (compacted form): the winner of kmeans2_search_kernel<0>'s partials is picked HERE by every block for itself (one launch
// less: kmeans2_pick_kernel<0> was a 6 us launch of one thread per utterance); block 0 leaves it for the kernels behind
template <bool PICK>
__global__ __launch_bounds__(256) void kmeans2_count_kernel(const float* __restrict__ feat, long per_utt, float db,
                                                            float* __restrict__ ws, long ws_stride, int* __restrict__ iw,
                                                            const int* __restrict__ frames, int F, int D) {
  using namespace km;
  __shared__ int red[256];
  __shared__ float best_s;
  const int b = blockIdx.y, tid = threadIdx.x;
  const float* f = feat + (long)b * per_utt;
  float* w = ws + (long)b * ws_stride;
  if constexpr (PICK) {
    static_assert(NBLK == 64, "one partial per lane of the first wave");
    if (tid < 64) {                              // argmax over the NBLK partials, ties to the smallest bin index
      const float* part = w + 1 + 2 * D;
      float v = part[2 * tid];
      int i = __builtin_bit_cast(int, part[2 * tid + 1]);      // (per_utt < 2^31)
      if (i >= per_utt) v = -INFINITY;           // a block without bins
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float v2 = __shfl_xor(v, o);
        const int i2 = __builtin_bit_cast(int, __shfl_xor(__builtin_bit_cast(float, i), o));      // (a bit move)
        if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
      }
      if (tid == 0) {
        best_s = v;
        if (blockIdx.x == 0) {                   // what kmeans2_pick_kernel<0> leaves: the maximum, the loudest bin, fresh counters
          w[0] = v;
          w[ws_stride - 1] = __builtin_bit_cast(float, i);
          for (int k = 0; k < 8; ++k) iw[(long)b * IW + 64 + k] = 0;
        }
      }
    }
    __syncthreads();
  }
  const float thr = (PICK ? best_s : w[0]) - db / 20.0f;
  const long nb = frames ? (long)frames[b] * F : per_utt;
  const long chunk = (nb + NBLK - 1) / NBLK, i_lo = (long)blockIdx.x * chunk, i_hi = i_lo + chunk < nb ? i_lo + chunk : nb;
  int c = 0;
  for (long i = i_lo + tid; i < i_hi; i += 256) c += f[i] >= thr ? 1 : 0;
  red[tid] = c;
  __syncthreads();
  for (int s2 = 128; s2 > 0; s2 >>= 1) {
    if (tid < s2) red[tid] += red[tid + s2];
    __syncthreads();
  }
  if (tid == 0) iw[(long)b * IW + blockIdx.x] = red[0];
}

template <int DT>
__global__ __launch_bounds__(256) void kmeans2_compact_kernel(const float* __restrict__ emb, const float* __restrict__ feat,
                                                              long per_utt, int D_rt, float db, float* __restrict__ ws,
                                                              long ws_stride, int* __restrict__ iw, float* __restrict__ comp,
                                                              const int* __restrict__ frames, int F) {
  using namespace km;
  constexpr int DC = DT ? DT : DMAX;
  const int D = DT ? DT : D_rt;
  __shared__ int scan[256];
  __shared__ int base_s;
  __shared__ float rv[256];
  __shared__ long ri[256];
  const int b = blockIdx.y, tid = threadIdx.x;
  const float* f = feat + (long)b * per_utt;
  const float* e = emb + (long)b * per_utt * D;
  float* w = ws + (long)b * ws_stride;
  float* out = comp + (long)b * per_utt * D;
  const float thr = w[0] - db / 20.0f;
  const long nb = frames ? (long)frames[b] * F : per_utt;
  const long chunk = (nb + NBLK - 1) / NBLK, i_lo = (long)blockIdx.x * chunk, i_hi = i_lo + chunk < nb ? i_lo + chunk : nb;
  if (tid == 0) {
    int sacc = 0;
    for (int k = 0; k < (int)blockIdx.x; ++k) sacc += iw[(long)b * IW + k];
    base_s = sacc;
    if (blockIdx.x == NBLK - 1) iw[(long)b * IW + 64] = sacc + iw[(long)b * IW + NBLK - 1];   // n_active
  }
  float c0[DC];
#pragma unroll
  for (int d = 0; d < DC; ++d) c0[d] = d < D ? w[1 + d] : 0.f;
  __syncthreads();
  int base = base_s;
  float best = INFINITY;
  long bi = per_utt;
  for (long t0 = i_lo; t0 < i_hi; t0 += 256) {
    const long i = t0 + tid;
    const int act = (i < i_hi && f[i] >= thr) ? 1 : 0;
    scan[tid] = act;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {          // inclusive scan of the activity flags
      const int v = tid >= off ? scan[tid - off] : 0;
      __syncthreads();
      scan[tid] += v;
      __syncthreads();
    }
    const int pos = base + scan[tid] - act, tot = scan[255];
    if (act) {
      float v[DC];
      if (DT && (DT % 4) == 0) {
        const float4* src = reinterpret_cast<const float4*>(e + i * D);
        float4* dst = reinterpret_cast<float4*>(out + (long)pos * D);
#pragma unroll
        for (int q = 0; q < DC / 4; ++q) {
          const float4 x = src[q];
          dst[q] = x;
          v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w;
        }
      } else {
#pragma unroll
        for (int d = 0; d < DC; ++d) {
          v[d] = d < D ? e[i * D + d] : 0.f;
          if (d < D) out[(long)pos * D + d] = v[d];
        }
      }
      float dot = 0.f;
#pragma unroll
      for (int d = 0; d < DC; ++d) dot += v[d] * c0[d];
      if (dot < best) { best = dot; bi = i; }
    }
    __syncthreads();
    base += tot;
  }
  // farthest-point initialisation of the second centroid (as kmeans2_search_kernel<1>): ties go to the smallest bin
  rv[tid] = best; ri[tid] = bi;
  __syncthreads();
  for (int s2 = 128; s2 > 0; s2 >>= 1) {
    if (tid < s2) {
      if (rv[tid + s2] < rv[tid] || (rv[tid + s2] == rv[tid] && ri[tid + s2] < ri[tid])) { rv[tid] = rv[tid + s2]; ri[tid] = ri[tid + s2]; }
    }
    __syncthreads();
  }
  if (tid == 0) {
    float* part = w + 1 + 2 * D;
    part[2 * blockIdx.x] = rv[0];
    part[2 * blockIdx.x + 1] = __builtin_bit_cast(float, (int)ri[0]);
  }
}

// INIT (compacted form, round 4): the farthest-point initialisation rides in pass 0 -- the pass that adds up the totals has
// every row in registers anyway: it also finds, per part, the row with the smallest dot product with c0 (ties to the smallest
// row), the parts exchange (value, row) next to their sums (three more tagged words), and everybody fetches c1 for itself.
// c0 itself is the loudest bin's row of the compacted array (dest[i0]).  Replaces kmeans2_search_kernel<2> (a 46 MB pass) and
// kmeans2_pick_kernel<1>: two launches fewer; the slots' start-up tags are then left by kmeans2_index_kernel.
template <int DT, bool INIT = false>
__global__ __launch_bounds__(km::LT) void kmeans2_lloyd_kernel(const float* __restrict__ comp, long per_utt, int D_rt, int iters,
                                                               float* __restrict__ ws, long ws_stride, int* __restrict__ iw, int u0,
                                                               int nutt, unsigned spin_limit, unsigned* __restrict__ status,
                                                               float tol, const int* __restrict__ dest = nullptr) {
  using namespace km;
  constexpr int DC = DT ? DT : DMAX;
  const int D = DT ? DT : D_rt;
  constexpr int NX = INIT ? 3 : 0;             // extra exchanged words per part: the init candidate's dot (two halves) and row
  constexpr unsigned NOROW = 0x3fffffffu;
  __shared__ float tol_s;                      // sklearn's tolerance for this utterance: tol x mean per-feature variance (after pass 0)
  __shared__ float arg_v[LT / 64];
  __shared__ unsigned arg_i[LT / 64];
  __shared__ unsigned row1_s;
  __shared__ float buf[(DC + 1) * LT];         // cluster 1's accumulators of every lane
  __shared__ float cen[2 * DMAX];
  __shared__ float dcen[DMAX];                 // c1 - c0: a bin goes to cluster 1 when (|c1|^2 - |c0|^2) - 2 e.(c1 - c0) < 0
  __shared__ float pw[NBP * 2 * (DMAX + 1)];   // everybody's partial sums of this iteration
  __shared__ unsigned ctl[4];                  // [0] give up at start-up, [1] all parts on one XCD, [2] a bounded wait ran out
  __shared__ unsigned chg[2];                  // centroids changed in this pass (by pass parity: reset two barriers before its next use)
  const int tid = threadIdx.x;
  // workgroup -> (utterance, part): workgroup b runs on XCD b % 8, so the NBP parts of an utterance share an XCD's L2
  const int blk = blockIdx.x;
  const int ul = (blk / (8 * NBP)) * 8 + (blk & 7), j = (blk >> 3) % NBP;
  if (ul >= nutt) return;                      // whole workgroup, before any barrier
  const int u = u0 + ul;
  float* w = ws + (long)u * ws_stride;
  int* iu = iw + (long)u * IW;
  const int n = iu[64];
  const long r_lo = (long)n * j / NBP, r_hi = (long)n * (j + 1) / NBP;
  const float* e = comp + (long)u * per_utt * D;
  // ---- start-up: do all parts of this utterance sit on one XCD?  (the exchange then stays inside that XCD's L2; the words
  //      were zeroed by kmeans2_pick_kernel<0>)
  if (tid == 0) {
    const unsigned xcc = __builtin_amdgcn_s_getreg(6164) & 15u;      // hwreg(HW_REG_XCC_ID, 0, 4)
    unsigned* uw = reinterpret_cast<unsigned*>(iu);
    __hip_atomic_fetch_max(uw + 67, xcc + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(uw + 68, 16u - xcc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __hip_atomic_fetch_add(uw + 65, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned spins = 0, ab = spin_limit == 0u ? 1u : 0u;
    while (!ab && __hip_atomic_fetch_add(uw + 65, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (unsigned)NBP) {
      __builtin_amdgcn_s_sleep(8);
      if (++spins > spin_limit || __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) ab = 1;
    }
    const unsigned hi = __hip_atomic_fetch_add(uw + 67, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned lo = __hip_atomic_fetch_add(uw + 68, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ab) __hip_atomic_store(status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ctl[0] = ab;
    ctl[1] = (hi + lo == 17u) ? 1u : 0u;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  }
  if constexpr (INIT) {                          // c0 = the loudest bin's row; c1 follows after pass 0 (until then: c0)
    if (tid < D) {
      const long row0 = dest[(long)u * per_utt + (long)__builtin_bit_cast(int, w[ws_stride - 1])];
      const float c = e[row0 * D + tid];
      cen[tid] = c;
      cen[D + tid] = c;
    }
  } else {
    if (tid < 2 * D) cen[tid] = w[1 + tid];     // initial centroids: written by earlier kernels
  }
  __syncthreads();
  if (ctl[0]) return;
  const bool fast = ctl[1] != 0;
  int it_done = 0;
  bool converged = false, gave_up = false;
  bool acc0 = false;                             // this pass accumulates cluster 0 (rows with t >= 0) instead of cluster 1

  // The partial sums carry their own "ready": bit 0 of every fp32 partial (2^-24 relative) is the tag of the pass,
  // slot = pass & 1, tag = (pass >> 1) & 1 -- a slot's consecutive writes differ, and kmeans2_pick_kernel<1> left every word with
  // tag 1 (what pass 0 does NOT expect).  A part stores its D+1 sums and polls all NBP x (D+1) words of the slot until
  // they carry this pass's tag: one L2 round trip after the last store lands, no counter, no fence.  Then EVERY part adds
  // the partials in part order and updates the centroids for itself (bitwise the same everywhere).
  //   * Only ONE cluster's sums (and count) are accumulated and exchanged; the other's are the utterance totals minus them.
  //     Pass 0 puts every row into the accumulated cluster: its sums ARE the totals.  Passes 1..iters are the Lloyd iterations.
  //     Which one: the cluster that came out SMALLER in the pass before (round 4; rounds 1-3 always accumulated cluster 1 -- a
  //     cluster 0 of a few per cent of the rows then lost digits to the cancellation totals - sums, and the persistent form could
  //     label a boundary bin differently from the launch-per-iteration form, which sums both clusters).  The difference now
  //     carries the LARGER cluster, whose relative error is (small / large) x 2^-24.  Every part takes the decision from the
  //     same exchanged counts: bitwise the same everywhere.
  //   * A lane keeps its first NR rows in registers for the whole launch (5 x 8 x 512 = 20 480 rows per utterance: an
  //     iteration then touches no memory at all); rows beyond that are streamed from the L2 / Infinity Cache every pass.
#ifndef ONSSEN_KM_NR
#define ONSSEN_KM_NR 5
#endif
#ifndef ONSSEN_KM_DCEN_SGPR
#define ONSSEN_KM_DCEN_SGPR 1      // c1 - c0 in scalar registers (round 6: init + Lloyd + masks 0.110 -> 0.104 ms, bit-identical); 0 = re-read from the LDS per row
#endif
  constexpr int NR = ONSSEN_KM_NR;
  __shared__ float tot[DMAX + 1];
  float rows[NR][DC];
  bool have[NR];
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    const long r = r_lo + tid + (long)k * LT;
    have[k] = r < r_hi;
    const long rr = have[k] ? r : (r_lo < r_hi ? r_lo : 0);      // (a valid row, masked out below)
    if (DT && (DT % 4) == 0) {
      const float4* src = reinterpret_cast<const float4*>(e + rr * D);
#pragma unroll
      for (int q = 0; q < DC / 4; ++q) {
        const float4 x = (n > 0) ? src[q] : make_float4(0.f, 0.f, 0.f, 0.f);
        rows[k][4 * q] = x.x; rows[k][4 * q + 1] = x.y; rows[k][4 * q + 2] = x.z; rows[k][4 * q + 3] = x.w;
      }
    } else {
#pragma unroll
      for (int d = 0; d < DC; ++d) rows[k][d] = (d < D && n > 0) ? e[rr * D + d] : 0.f;
    }
  }
  auto run = [&](auto fast_c) __attribute__((always_inline)) {
    constexpr bool FAST = decltype(fast_c)::value;
    constexpr int LD_AUX = FAST ? 16 : 17;       // sc1: served by this XCD's L2 | sc0 sc1: coherent anywhere
    constexpr int ST_AUX = FAST ? 0 : 17;
    const int nc = D + 1 + NX, nw = NBP * nc;    // words per part / per utterance and slot
    if (tid < D) dcen[tid] = INIT ? cen[tid] : cen[D + tid] - cen[tid];      // (INIT: pass 0 measures every row against c0)
    if (tid == 0) ctl[2] = 0u;
    __syncthreads();
    for (int ps = 0; ps <= iters; ++ps) {
      // three workgroup barriers per pass (round 4; eight before): accumulators -> LDS | polled words -> LDS | new centroids
      const unsigned tag = ((unsigned)ps >> 1) & 1u;
      const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc((void*)(w + 1 + 2 * D + (ps & 1) * nw), 0, nw * 4, 0x00020000);
      float s1[DC];
      float n1 = 0.f, qd = 0.f;
#pragma unroll
      for (int d = 0; d < DC; ++d) {
        const float a0 = d < D ? cen[d] : 0.f, a1 = d < D ? cen[D + d] : 0.f;
        qd += a1 * a1 - a0 * a0;
        s1[d] = 0.f;
      }
      if (ps == 0) qd = -INFINITY;               // pass 0: every row counts (the totals)
      float best = INFINITY;
      unsigned bi = NOROW;
#if ONSSEN_KM_DCEN_SGPR
      // c1 - c0 is the same for every lane: ONE LDS read per lane and pass, then v_readlane into D scalar registers -- the dot products
      // below take them as scalar operands (round 6; rounds 3-5 re-read all D words from the LDS for every row: 100 ds_read per lane and pass)
      float dcu[DC];
      {
        const float mine = (tid & 63) < D ? dcen[tid & 63] : 0.f;
#pragma unroll
        for (int d = 0; d < DC; ++d) dcu[d] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mine), d));
      }
#endif
      auto row = [&](const float (&v)[DC], bool live, long ridx) __attribute__((always_inline)) {
#if !ONSSEN_KM_DCEN_SGPR && !defined(ONSSEN_HOST_EMULATION) && !defined(ONSSEN_KM_NOCLOB)
        asm volatile("" ::: "memory");           // keep the LDS reads inside the loop (no hoisting into D more registers)
#endif
        float dot = 0.f;                         // (summing v.dcen and doubling the sum: `2 v[d]` of the register-resident
#pragma unroll                                   //  rows is loop-invariant and would be kept in a second set of registers)
        for (int d = 0; d < DC; ++d)
#if ONSSEN_KM_DCEN_SGPR
          if (d < D) dot += v[d] * dcu[d];
#else
          if (d < D) dot += v[d] * dcen[d];
#endif
        if constexpr (INIT) {                    // pass 0: dot = e.c0 -- the farthest-point candidate of this lane (rows ascend)
          if (ps == 0 && live && dot < best) { best = dot; bi = (unsigned)ridx; }
        }
        const float t = qd - 2.f * dot;          // ||e - c1||^2 - ||e - c0||^2: the row belongs to cluster 1 when t < 0
        const float sel = (live && ((t < 0.f) != acc0)) ? 1.f : 0.f;
#pragma unroll
        for (int d = 0; d < DC; ++d) s1[d] += sel * v[d];
        n1 += sel;
      };
#pragma unroll
      for (int k = 0; k < NR; ++k) row(rows[k], have[k], r_lo + tid + (long)k * LT);
#pragma unroll 1
      for (long r = r_lo + tid + (long)NR * LT; r < r_hi; r += LT) {     // what did not fit the registers
        float v[DC];
        if (DT && (DT % 4) == 0) {
          const float4* src = reinterpret_cast<const float4*>(e + r * D);
#pragma unroll
          for (int q = 0; q < DC / 4; ++q) {
            const float4 x = src[q];
            v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w;
          }
        } else {
#pragma unroll
          for (int d = 0; d < DC; ++d) v[d] = d < D ? e[r * D + d] : 0.f;
        }
        row(v, true, r);
      }
      if constexpr (INIT) {
        if (ps == 0) {                           // the wave's candidate: smallest dot, ties to the smallest row
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) {
            const float v2 = __shfl_xor(best, o);
            const unsigned i2 = __builtin_bit_cast(unsigned, __shfl_xor(__builtin_bit_cast(float, bi), o));
            if (v2 < best || (v2 == best && i2 < bi)) { best = v2; bi = i2; }
          }
          if ((tid & 63) == 0) { arg_v[tid >> 6] = best; arg_i[tid >> 6] = bi; }
        }
      }
      // column sums through the LDS: 8 lanes per column add LT/8 values each (four independent chains), then combine across
      // the 8 lanes; the D+1 sums go to partial[slot][j][..], tagged
#pragma unroll
      for (int d = 0; d < DC; ++d)
        if (d < D) buf[d * LT + tid] = s1[d];
      buf[D * LT + tid] = n1;
      if (tid == 0) chg[ps & 1] = 0u;            // (set after the next barrier, read after the one behind it)
      __syncthreads();
      {
        const int sub = tid & 7;
        for (int col = tid >> 3; col < ((D + 1 + LT / 8 - 1) / (LT / 8)) * (LT / 8); col += LT / 8) {   // (whole 8-lane groups together)
          float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
          if (col <= D) {
            // a lane's LT/8 values are LT/8 floats apart from its neighbours': read them in an order rotated by the lane
            // number, so that the 32 lanes of a half-wave hit 32 different banks (un-rotated: ALL 64 lanes on one bank --
            // SQ_LDS_BANK_CONFLICT 12.4 M cycles per launch)
            const float* cb = buf + col * LT + sub * (LT / 8);
            const int rot = tid & 63;
#pragma unroll 4
            for (int kk = 0; kk < LT / 8; kk += 4) {
              a0 += cb[(kk + rot) & (LT / 8 - 1)]; a1 += cb[(kk + 1 + rot) & (LT / 8 - 1)];
              a2 += cb[(kk + 2 + rot) & (LT / 8 - 1)]; a3 += cb[(kk + 3 + rot) & (LT / 8 - 1)];
            }
          }
          float acc = (a0 + a1) + (a2 + a3);
          acc += __shfl_xor(acc, 1);
          acc += __shfl_xor(acc, 2);
          acc += __shfl_xor(acc, 4);
          if (col <= D && sub == 0)
            __builtin_amdgcn_raw_buffer_store_b32((__builtin_bit_cast(unsigned, acc) & ~1u) | tag, rp, (j * nc + col) * 4, 0, ST_AUX);
        }
      }
      if constexpr (INIT) {                      // the part's candidate (pass 0) rides in the three extra words, tagged like the sums
        if (tid == LT - 1) {
          float bv = INFINITY;
          unsigned bidx = NOROW;
          if (ps == 0)
            for (int k = 0; k < LT / 64; ++k)
              if (arg_v[k] < bv || (arg_v[k] == bv && arg_i[k] < bidx)) { bv = arg_v[k]; bidx = arg_i[k]; }
          const unsigned vb = __builtin_bit_cast(unsigned, bv);
          __builtin_amdgcn_raw_buffer_store_b32(((vb >> 16) << 1) | tag, rp, (j * nc + D + 1) * 4, 0, ST_AUX);
          __builtin_amdgcn_raw_buffer_store_b32(((vb & 0xffffu) << 1) | tag, rp, (j * nc + D + 2) * 4, 0, ST_AUX);
          __builtin_amdgcn_raw_buffer_store_b32((bidx << 1) | tag, rp, (j * nc + D + 3) * 4, 0, ST_AUX);
        }
      }
      // ---- poll the slot: every word must carry this pass's tag.  Each lane of the first waves owns words k, k + LT, ... and
      //      polls them by itself until they are new (bounded) -- no workgroup barrier inside the wait (rounds 1-3: two per
      //      polling round for all eight waves)
      for (int k = tid; k < nw; k += LT) {
        // (atomic loads: a buffer-load builtin is a read-only call to the compiler -- inside a spin loop without barriers it is
        //  hoisted and the loop only counts to its limit, whatever "memory" clobbers or cache-policy bits say.  Agent scope = sc1:
        //  served by this XCD's L2; system scope = sc0 sc1: coherent anywhere)
        const unsigned* wp = reinterpret_cast<const unsigned*>(w + 1 + 2 * D + (ps & 1) * nw) + k;
        unsigned v = FAST ? __hip_atomic_load(wp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                          : __hip_atomic_load(wp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        for (unsigned spins = 0; ((v ^ tag) & 1u) != 0u; ++spins) {
          if (spins > spin_limit) {              // gave up: the host re-runs the launch-per-iteration form; the code says where
            ctl[2] = 1u;
            __hip_atomic_store(status, 0x40000000u | ((unsigned)ps << 16) | ((unsigned)j << 12) | (unsigned)k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
          }
#ifdef ONSSEN_HOST_EMULATION
          __builtin_amdgcn_s_sleep(1);           // (emulated lanes are OS threads: let the producers run)
#else
          if (!FAST) __builtin_amdgcn_s_sleep(1);
#endif
          v = FAST ? __hip_atomic_load(wp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                   : __hip_atomic_load(wp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        pw[k] = __builtin_bit_cast(float, v & ~1u);
      }
      __syncthreads();
      if (ctl[2] != 0u) {                        // uniform: somebody's wait ran out (status: 0x40000000 | pass << 16 | part << 12 | word)
        gave_up = true;
        return;
      }
      // ---- every part finishes the pass for itself: partial sums added in part order (bitwise the same everywhere)
      if (ps == 0) {                             // the totals
        if (tid <= D) {
          float ssum = 0.f;
          for (int k = 0; k < NBP; ++k) ssum += pw[k * nc + tid];
          tot[tid] = ssum;
        }
        if (tid == LT - 1) {                     // sklearn's stopping rule (kmeans2_update_kernel): tol x (1 - |mean|^2) / D -- from the words
          float cnt = 0.f, m2 = 0.f;             // themselves, in the order tot[] is formed: the same bits in every part
          for (int k = 0; k < NBP; ++k) cnt += pw[k * nc + D];
          for (int d = 0; d < D; ++d) {
            float ssum = 0.f;
            for (int k = 0; k < NBP; ++k) ssum += pw[k * nc + d];
            const float m = ssum / cnt;
            m2 += m * m;
          }
          tol_s = (tol > 0.f && 1.0f - m2 > 0.f) ? tol * (1.0f - m2) / (float)D : 0.f;
        }
        if constexpr (INIT) {                    // ... and the second centroid: the row farthest from c0 over all parts (in part
          if (tid == 0) {                        // order = row order: strict comparison keeps the first), or c0 itself
            float bv = INFINITY;
            unsigned bidx = NOROW;
            for (int k = 0; k < NBP; ++k) {
              const unsigned hi = __builtin_bit_cast(unsigned, pw[k * nc + D + 1]) >> 1, lo = __builtin_bit_cast(unsigned, pw[k * nc + D + 2]) >> 1;
              const float v = __builtin_bit_cast(float, (hi << 16) | lo);
              const unsigned i = __builtin_bit_cast(unsigned, pw[k * nc + D + 3]) >> 1;
              if (i != NOROW && (v < bv || (v == bv && i < bidx))) { bv = v; bidx = i; }
            }
            row1_s = bidx;
          }
          __syncthreads();
          if (tid < D) {
            const unsigned r1 = row1_s;
            const float c1 = r1 == NOROW ? cen[tid] : e[(long)r1 * D + tid];
            cen[D + tid] = c1;
            dcen[tid] = c1 - cen[tid];
          }
        }
        __syncthreads();
        continue;
      }
      if (tid < 64) {                            // (the first wave) lane d < D: component d of both centroids and of their difference
        float sh = 0.f;
        bool moved = false;
        if (tid < D) {
          float ssum = 0.f, cnt = 0.f;
          for (int k = 0; k < NBP; ++k) {
            ssum += pw[k * nc + tid];
            cnt += pw[k * nc + D];
          }
          const float osum = tot[tid] - ssum, ocnt = tot[D] - cnt;       // the cluster that was not accumulated = everything else
          const float s0 = acc0 ? ssum : osum, n0 = acc0 ? cnt : ocnt, s1c = acc0 ? osum : ssum, n1c = acc0 ? ocnt : cnt;
          const float c0o = cen[tid], c1o = cen[D + tid];
          float c0n = c0o, c1n = c1o;
          if (n0 > 0.f) c0n = s0 / n0;           // an empty cluster keeps its centroid
          if (n1c > 0.f) c1n = s1c / n1c;
          moved = c0n != c0o || c1n != c1o;
          sh = (c0n - c0o) * (c0n - c0o) + (c1n - c1o) * (c1n - c1o);
          cen[tid] = c0n;
          cen[D + tid] = c1n;
          dcen[tid] = c1n - c0n;
        }
        // go on only if a component moved (else: the exact fixed point) AND the centroids' squared shift exceeds sklearn's
        // tolerance; summed over the lanes of this wave in a fixed order: the same decision in every part
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sh += __shfl_xor(sh, o);
        const bool any_moved = !__all(!moved);
        if (tid == 0 && any_moved && sh > tol_s) chg[ps & 1] = 1u;
      }
      it_done = ps;
      {   // the next pass accumulates the cluster that is smaller NOW (counts of this pass, the same words in every part)
        float cnt = 0.f;
        for (int k = 0; k < NBP; ++k) cnt += pw[k * nc + D];
        const float cnt1 = acc0 ? tot[D] - cnt : cnt;
        acc0 = 2.f * cnt1 > tot[D];              // cluster 1 holds more than half: accumulate cluster 0
      }
      __syncthreads();
      if (chg[ps & 1] == 0u) { converged = true; break; }   // exact fixed point: every further iteration would reproduce it
    }
  };
  if (fast) run(std::true_type{}); else run(std::false_type{});
  if (gave_up) return;
  // part 0 leaves the result for the mask pass (a later launch): centroids, done flag, iteration count (probes)
  if (j == 0) {
    if (tid < 2 * D) w[1 + tid] = cen[tid];
    if (tid == 0) {
      if (converged) w[ws_stride - 1] = 1.0f;
      iu[66] = it_done | (converged ? 0x10000 : 0) | (fast ? 0 : 0x20000);
    }
  }
}


// ---- round 4: the embedding never exists for the silent bins (onssen_dc_index_f32 -> onssen_linear_x3p_compact -> onssen_dc_cluster_compact_f32)
// Which bins are active is known from the mixture's log-magnitude BEFORE the network runs (evaluate.py:36-37), and the back end
// reads the embedding of the active ones only.  kmeans2_index_kernel turns the threshold into a target map
//   dest[b][t*F + f] = row of bin (t, f) in utterance b's compacted array, or -1 for a silent bin
// (same order-preserving positions as kmeans2_compact_kernel: chunk base + in-block scan); the fc_dc GEMM's epilogue scatters the
// normalised rows straight into the compacted array; the clustering then runs on it as before and the mask pass labels the
// active bins through the same map.  Saves the 132 MB write + 132 MB read of the full embedding and the compaction pass.
__global__ __launch_bounds__(256) void kmeans2_index_kernel(const float* __restrict__ feat, long per_utt, float db,
                                                            const float* __restrict__ ws, long ws_stride, int* __restrict__ iw,
                                                            int* __restrict__ dest, const int* __restrict__ frames, int F, int D) {
  using namespace km;
  __shared__ int scan[256];
  __shared__ int base_s;
  const int b = blockIdx.y, tid = threadIdx.x;
  const float* f = feat + (long)b * per_utt;
  int* dst = dest + (long)b * per_utt;
  const float thr = ws[(long)b * ws_stride] - db / 20.0f;
  const long nb = frames ? (long)frames[b] * F : per_utt;
  const long chunk = (nb + NBLK - 1) / NBLK, i_lo = (long)blockIdx.x * chunk, i_hi = i_lo + chunk < nb ? i_lo + chunk : nb;
  if (tid == 0) {
    int sacc = 0;
    for (int k = 0; k < (int)blockIdx.x; ++k) sacc += iw[(long)b * IW + k];
    base_s = sacc;
    if (blockIdx.x == NBLK - 1) iw[(long)b * IW + 64] = sacc + iw[(long)b * IW + NBLK - 1];   // n_active
  }
  __syncthreads();
  int base = base_s;
  for (long t0 = i_lo; t0 < i_hi; t0 += 256) {
    const long i = t0 + tid;
    const int act = (i < i_hi && f[i] >= thr) ? 1 : 0;
    scan[tid] = act;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {          // inclusive scan of the activity flags
      const int v = tid >= off ? scan[tid - off] : 0;
      __syncthreads();
      scan[tid] += v;
      __syncthreads();
    }
    if (i < i_hi) dst[i] = act ? base + scan[tid] - act : -1;
    const int tot = scan[255];
    __syncthreads();
    base += tot;
  }
  for (long i = nb + (long)blockIdx.x * 256 + tid; i < per_utt; i += (long)NBLK * 256) dst[i] = -1;   // a ragged batch's padding
  // the Lloyd kernel's two slots of tagged words (the scratch of the searches, read for the last time by the count kernel): every
  // word starts with tag 1, which is what its first pass does not expect (kmeans2_pick_kernel<1> does this in the other form)
  if (blockIdx.x == 0) {
    float* wb = const_cast<float*>(ws) + (long)b * ws_stride;
    for (int k = tid; k < 2 * NBP * (D + 4); k += 256) wb[1 + 2 * D + k] = __builtin_bit_cast(float, 1u);
  }
}

// argmax of bins [lo, hi) of f by one workgroup of NTHR threads: (-inf, none) if there is none, ties to the smallest index (rv, ri:
// NTHR words of LDS each, free again on return)
template <int NTHR>
__device__ __forceinline__ void kmeans2_block_argmax(const float* __restrict__ f, long lo, long hi, int none, float* rv, int* ri,
                                                     float& v, int& ix) {
  const int tid = threadIdx.x;
  float best = -INFINITY;
  int bi = none;
#pragma unroll 8
  for (long i = lo + tid; i < hi; i += NTHR)
    if (f[i] > best) { best = f[i]; bi = (int)i; }
  rv[tid] = best; ri[tid] = bi;
  __syncthreads();
  for (int s = NTHR / 2; s > 0; s >>= 1) {
    if (tid < s && (rv[tid + s] > rv[tid] || (rv[tid + s] == rv[tid] && ri[tid + s] < ri[tid]))) { rv[tid] = rv[tid + s]; ri[tid] = ri[tid + s]; }
    __syncthreads();
  }
  v = rv[0]; ix = ri[0];
  __syncthreads();
}

// The target map of WHOLE utterances by one workgroup of NTHR threads: what kmeans2_search_kernel<0>, kmeans2_count_kernel<true> and
// kmeans2_index_kernel leave for a uniform batch, word for word, for the utterances first, first + step, ... < B.  Called by the spare
// workgroups of the pair launch (lstm_xcd_kernel<AUX>), which lend it `lds` (NTHR * 8 + 512 bytes).  Nothing crosses workgroups, so the
// NBLK partials and chunk bases collapse: the argmax is taken over the utterance at once (same order: larger value, then smaller
// index), dest[i] is the number of active bins before bin i (what chunk base + in-block scan add up to), and a chunk's count is the
// difference of that number at its two ends.  Integers and one float compare per bin: the same bits whatever the partition.
template <int NTHR>
__device__ __forceinline__ void kmeans2_map_workgroup(const float* __restrict__ feat, long per_utt, float db, float* __restrict__ ws, long ws_stride,
                                      int* __restrict__ iw, int* __restrict__ dest, int D, int B, int first, int step, char* lds) {
  using namespace km;
  static_assert(NBLK == 64 && IW == 72, "the int words of an utterance: 64 chunk counts, then 8 counters");
  constexpr int NWV = NTHR / 64, RUN = 8;            // a thread scans RUN consecutive bins of a tile of NTHR * RUN
  float* rv = reinterpret_cast<float*>(lds);         // [NTHR] argmax values ...
  int* ri = reinterpret_cast<int*>(rv + NTHR);       // [NTHR] ... and indices
  int* wtot = ri + NTHR;                             // [2][NWV] active bins per wave of a tile (two tiles in flight)
  int* cs = wtot + 2 * NWV;                          // [NBLK] active bins before each chunk
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nb = (int)per_utt;                       // (per_utt < 2^31, as everywhere here)
  const int chunk = (nb + NBLK - 1) / NBLK;
  const int ntag = 2 * NBP * (D + 4);
  for (int b = first; b < B; b += step) {
    const float* f = feat + (long)b * per_utt;
    float* w = ws + (long)b * ws_stride;
    float* part = w + 1 + 2 * D;
    int* iwb = iw + (long)b * IW;
    int* dst = dest + (long)b * per_utt;
    float vmax;
    int imax;
    kmeans2_block_argmax<NTHR>(f, 0, nb, nb, rv, ri, vmax, imax);
    const float thr = vmax - db / 20.0f;
    int base = 0, par = 0;                           // active bins before this tile; which half of wtot it uses
    for (long t0 = 0; t0 < nb; t0 += (long)NTHR * RUN, par ^= 1) {
      const long i0 = t0 + (long)tid * RUN;
      int act[RUN], c = 0;
#pragma unroll
      for (int r = 0; r < RUN; ++r) {
        act[r] = (i0 + r < nb && f[i0 + r] >= thr) ? 1 : 0;
        c += act[r];
      }
      int incl = c;                                  // inclusive scan over the wave, then the waves before this one
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int v = __builtin_bit_cast(int, __shfl(__builtin_bit_cast(float, incl), (lane - o) & 63));      // (a bit move)
        if (lane >= o) incl += v;
      }
      if (lane == 63) wtot[par * NWV + wv] = incl;
      __syncthreads();
      int pos = base + incl - c;
#pragma unroll
      for (int k = 0; k < NWV; ++k) {
        const int t = wtot[par * NWV + k];
        if (k < wv) pos += t;
        base += t;
      }
      if (i0 < nb) {
        unsigned kc = ((unsigned)i0 + (unsigned)chunk - 1u) / (unsigned)chunk;      // the first chunk that starts at or after i0
        long cstart = (long)kc * chunk;
#pragma unroll
        for (int r = 0; r < RUN; ++r) {
          const long i = i0 + r;
          if (i < nb) {
            if (i == cstart) { cs[kc] = pos; ++kc; cstart += chunk; }
            dst[i] = act[r] ? pos : -1;
            pos += act[r];
          }
        }
      }
    }
    __syncthreads();
    if (tid < NBLK) {                                // chunks past the last bin start (and end) at the total
      const int c_lo = (long)tid * chunk < nb ? cs[tid] : base;
      const int c_hi = (tid + 1 < NBLK && (long)(tid + 1) * chunk < nb) ? cs[tid + 1] : base;
      iwb[tid] = c_hi - c_lo;
    }
    if (tid < 8) iwb[64 + tid] = tid == 0 ? base : 0;     // n_active, fresh counters
    if (tid == 0) {
      w[0] = vmax;
      w[ws_stride - 1] = __builtin_bit_cast(float, imax);
    }
    // the Lloyd kernel's tagged words cover the scratch of the searches up to word ntag; the partials of the chunks behind that
    // (a narrow embedding only: ntag >= 2 NBLK from D = 4 on) stay as the search leaves them
    for (int k = tid; k < ntag; k += NTHR) part[k] = __builtin_bit_cast(float, 1u);
    for (int k = ntag / 2; k < NBLK; ++k) {
      const long lo = (long)k * chunk, hi = lo + chunk < nb ? lo + chunk : nb;
      float v;
      int ix;
      kmeans2_block_argmax<NTHR>(f, lo, hi, nb, rv, ri, v, ix);
      if (tid == 0) {
        part[2 * k] = v;
        part[2 * k + 1] = __builtin_bit_cast(float, ix);
      }
    }
    __syncthreads();                                 // cs and wtot are the next utterance's
  }
}

// masks of the compacted form: bin i is labelled from row dest[i] of the compacted array (the arithmetic of
// kmeans2_assign_kernel<1>: same distances, same labels), silent bins get (0, 0)
template <int DT>
__global__ __launch_bounds__(256) void kmeans2_mask_compact_kernel(const float* __restrict__ comp, const int* __restrict__ dest,
                                                                   long per_utt, int D_rt, const float* __restrict__ ws,
                                                                   long ws_stride, float* __restrict__ masks) {
  using namespace km;
  constexpr int DC = DT ? DT : DMAX;
  const int D = DT ? DT : D_rt;
  const int b = blockIdx.y, tid = threadIdx.x;
  const float* e = comp + (long)b * per_utt * D;
  const int* dst = dest + (long)b * per_utt;
  const float* w = ws + (long)b * ws_stride;
  float c0[DC], c1[DC];
  float q0 = 0.f, q1 = 0.f;
#pragma unroll
  for (int d = 0; d < DC; ++d) {
    c0[d] = d < D ? w[1 + d] : 0.f; c1[d] = d < D ? w[1 + D + d] : 0.f;
    q0 += c0[d] * c0[d]; q1 += c1[d] * c1[d];
  }
  for (long i = (long)blockIdx.x * 256 + tid; i < per_utt; i += (long)gridDim.x * 256) {
    const int row = dst[i];
    int lab = 0;
    if (row >= 0) {
      float v[DC];
      if (DT && (DT % 4) == 0) {
        const float4* src = reinterpret_cast<const float4*>(e + (long)row * D);
#pragma unroll
        for (int q = 0; q < DC / 4; ++q) {
          const float4 x = src[q];
          v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w;
        }
      } else {
#pragma unroll
        for (int d = 0; d < DC; ++d) v[d] = d < D ? e[(long)row * D + d] : 0.f;
      }
      float d0 = q0, d1 = q1;               // ||e - c||^2 = ||e||^2 - 2 e.c + ||c||^2 ; ||e||^2 is common
#pragma unroll
      for (int d = 0; d < DC; ++d) {
        d0 -= 2.f * v[d] * c0[d];
        d1 -= 2.f * v[d] * c1[d];
      }
      lab = d1 < d0 ? 1 : 0;
    }
    *reinterpret_cast<float2*>(masks + 2 * ((long)b * per_utt + i)) =
        make_float2(row >= 0 ? (float)lab : 0.0f, row >= 0 ? (float)(1 - lab) : 0.0f);   // mask[0] = label, mask[1] = 1 - label
  }
}
