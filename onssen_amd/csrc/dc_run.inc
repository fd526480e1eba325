// Deep-clustering 2-means host side (part of onssen_hip.hip; after labels_cluster.inc, whose kmeans2_* kernels it launches, and
// kmeans_k.inc): ONE workspace layout (DcWs), ONE Lloyd launcher, ONE D dispatch, and the C ABI entries over them.

// ---- workspace, byte offsets from the 256-byte aligned base: [B][stride] float header (feature max, centroids, partial sums, done flag) |
// [B][km::IW] ints | status word | compacted active rows [B][T*F][D] (persistent form) | target map [B][T*F] int32 (compacted route only)
struct DcWs {
  long stride = 0;                                         // floats per utterance of the header
  size_t iw = 0, status = 0, comp = 0, dest = 0, cluster_bytes = 0, compact_bytes = 0;   // the totals: without / with the target map
  DcWs(int B, int T, int F, int D) {
    if (B <= 0 || T <= 0 || F <= 0 || D <= 0 || D > km::DMAX) return;
    stride = 1 + 2 * D + km::NBLK * 2 * (D + 1) + 1;
    iw = align256((size_t)B * stride * sizeof(float));
    status = iw + (size_t)B * km::IW * sizeof(int);
    comp = align256(status + 256);
    cluster_bytes = comp + (size_t)B * T * F * D * sizeof(float);
    dest = align256(cluster_bytes);
    compact_bytes = dest + align256((size_t)B * T * F * sizeof(int32_t) + 16);   // (+16: onssen_linear_x3p_compact reads the map in 16-byte words)
  }
  template <class T> T* at(void* ws, size_t off) const { return (T*)((char*)ws + off); }
};
size_t onssen_dc_cluster_status_offset(int B, int D) { return DcWs(B, 1, 1, D).status; }
size_t onssen_dc_cluster_workspace_bytes(int B, int T, int F, int D) { return DcWs(B, T, F, D).cluster_bytes; }
size_t onssen_dc_compact_workspace_bytes(int B, int T, int F, int D) { return DcWs(B, T, F, D).compact_bytes; }
int onssen_dc_compact_layout(int B, int T, int F, int D, size_t* comp_offset, size_t* dest_offset) {
  const DcWs l(B, T, F, D);
  if (!l.stride) return ONSSEN_E_ARG;
  if (comp_offset) *comp_offset = l.comp;
  if (dest_offset) *dest_offset = l.dest;
  return ONSSEN_OK;
}

// D -> compile-time constant: f(std::integral_constant<int, DT>), DT = 20 for the wsj0-2mix width, 0 (= D is read at run time) otherwise
template <class Fn>
static void dispatch_d(int D, Fn&& f) { D == 20 ? f(std::integral_constant<int, 20>{}) : f(std::integral_constant<int, 0>{}); }

// one workgroup per CU: as many utterances per Lloyd launch as the device has CUs / NBP (32 on a whole MI355X; fewer in a
// partitioned mode -- a launch that cannot be co-resident would only be caught by its bounded waits)
static int lloyd_utts() {
  static const int n = [] {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
    const int n = cus / km::NBP;
    return n < 1 ? 1 : n > 32 ? 32 : n;
  }();
  return n;
}

// ALL Lloyd iterations in one launch per <= lloyd_utts() utterances (a wait that gives up leaves status = 1: the host sees it and runs the
// launch-per-iteration form).  INIT: the farthest-point initialisation rides in the launch's first pass, so it runs with iters = 0 too.
template <bool INIT>
static void launch_lloyd(hipStream_t st, const DcWs& l, void* ws, int B, long per_utt, int D, int iters, float tol) {
  const unsigned spin = xcd_spin_limit();
  const int per = lloyd_utts();
  const int* dest = INIT ? l.at<const int>(ws, l.dest) : nullptr;
  for (int u0 = 0; u0 < B && (INIT || iters > 0); u0 += per) {
    const int nutt = B - u0 < per ? B - u0 : per;
    const dim3 lgrid((unsigned)(ceil_div(nutt, 8) * 8 * km::NBP));
    dispatch_d(D, [&](auto dt) { hipLaunchKernelGGL((kmeans2_lloyd_kernel<decltype(dt)::value, INIT>), lgrid, dim3(km::LT), 0, st,
                                                    l.at<const float>(ws, l.comp), per_utt, D, iters, (float*)ws, l.stride, l.at<int>(ws, l.iw),
                                                    u0, nutt, spin, l.at<unsigned>(ws, l.status), tol, dest); });
  }
}

// ---- a materialised embedding: threshold, farthest-point initialisation, Lloyd, masks -----------------------------------------
static int dc_cluster_impl(const float* emb, const float* feature, int B, int T, int F, int D, float db_threshold,
                           int iters, float tol, float* masks, void* ws, size_t ws_bytes, int flags, void* stream, const int32_t* frames) {
  if (!emb || !feature || !masks || !ws || B <= 0 || T <= 0 || F <= 0 || D <= 0 || D > km::DMAX || iters < 0 || !(tol >= 0.f))
    return ONSSEN_E_ARG;
  const DcWs l(B, T, F, D);
  if (ws_bytes < l.cluster_bytes) return ONSSEN_E_WORKSPACE;
  if (!aligned16(emb) || (reinterpret_cast<uintptr_t>(ws) & 255u)) return ONSSEN_E_ALIGN;
  ONSSEN_CLEAR_ERROR();
  hipStream_t st = (hipStream_t)stream;
  const long per_utt = (long)T * F, stride = l.stride;
  float* w = (float*)ws;
  int* iw = l.at<int>(ws, l.iw);
  const dim3 sgrid(km::NBLK, (unsigned)B);
  auto assign = [&](auto mode, float* out) {       // mode 0: the partial sums of one Lloyd iteration; 1: the masks
    dispatch_d(D, [&](auto dt) { hipLaunchKernelGGL((kmeans2_assign_kernel<decltype(mode)::value, decltype(dt)::value>), sgrid, dim3(256), 0, st,
                                                    emb, feature, per_utt, D, db_threshold, w, stride, out, frames, F); });
  };
  hipLaunchKernelGGL((kmeans2_search_kernel<0>), sgrid, dim3(256), 0, st, emb, feature, per_utt, D, db_threshold, w, stride, frames, F);
  hipLaunchKernelGGL((kmeans2_pick_kernel<0>), dim3((unsigned)B), dim3(64), 0, st, emb, per_utt, D, w, stride, iw);
  if (!(flags & ONSSEN_DC_CLUSTER_LAUNCH_PER_ITERATION)) {
    // active bins compacted once (the same pass finds the second centroid), then the persistent Lloyd launches
    hipLaunchKernelGGL((kmeans2_count_kernel<false>), sgrid, dim3(256), 0, st, feature, per_utt, db_threshold, w, stride, iw, frames, F, D);
    dispatch_d(D, [&](auto dt) { hipLaunchKernelGGL((kmeans2_compact_kernel<decltype(dt)::value>), sgrid, dim3(256), 0, st, emb, feature, per_utt,
                                                    D, db_threshold, w, stride, iw, l.at<float>(ws, l.comp), frames, F); });
    hipLaunchKernelGGL((kmeans2_pick_kernel<1>), dim3((unsigned)B), dim3(64), 0, st, emb, per_utt, D, w, stride, (int*)nullptr);
    launch_lloyd<false>(st, l, ws, B, per_utt, D, iters, tol);
  } else {
    hipLaunchKernelGGL((kmeans2_search_kernel<1>), sgrid, dim3(256), 0, st, emb, feature, per_utt, D, db_threshold, w, stride, frames, F);
    hipLaunchKernelGGL((kmeans2_pick_kernel<1>), dim3((unsigned)B), dim3(64), 0, st, emb, per_utt, D, w, stride, (int*)nullptr);
    for (int it = 0; it < iters; ++it) {
      assign(std::integral_constant<int, 0>{}, (float*)nullptr);
      hipLaunchKernelGGL(kmeans2_update_kernel, dim3((unsigned)B), dim3(256), 0, st, D, km::NBLK, w, stride, tol);
    }
  }
  assign(std::integral_constant<int, 1>{}, masks);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_dc_cluster_f32(const float* emb, const float* feature, int B, int T, int F, int D, float db_threshold,
                          int iters, float tol, float* masks, void* ws, size_t ws_bytes, int flags, void* stream) {
  return dc_cluster_impl(emb, feature, B, T, F, D, db_threshold, iters, tol, masks, ws, ws_bytes, flags, stream, nullptr);
}

int onssen_dc_cluster_ragged_f32(const float* emb, const float* feature, int B, int T, const int32_t* frames, int F, int D, float db_threshold,
                                 int iters, float tol, float* masks, void* ws, size_t ws_bytes, int flags, void* stream) {
  if (!frames) return ONSSEN_E_ARG;
  return dc_cluster_impl(emb, feature, B, T, F, D, db_threshold, iters, tol, masks, ws, ws_bytes, flags, stream, frames);
}

// ---- compacted form (round 4): index -> (the fc_dc GEMM scatters the active rows) -> cluster ---------------------------------
int onssen_dc_index_f32(const float* feature, int B, int T, const int32_t* frames, int F, int D, float db_threshold, void* ws,
                        size_t ws_bytes, void* stream) {
  if (!feature || !ws || B <= 0 || T <= 0 || F <= 0 || D <= 0 || D > km::DMAX) return ONSSEN_E_ARG;
  const DcWs l(B, T, F, D);
  if (ws_bytes < l.compact_bytes) return ONSSEN_E_WORKSPACE;
  if (reinterpret_cast<uintptr_t>(ws) & 255u) return ONSSEN_E_ALIGN;
  ONSSEN_CLEAR_ERROR();
  hipStream_t st = (hipStream_t)stream;
  const long per_utt = (long)T * F, stride = l.stride;
  float* w = (float*)ws;
  int* iw = l.at<int>(ws, l.iw);
  const dim3 sgrid(km::NBLK, (unsigned)B);
  hipLaunchKernelGGL((kmeans2_search_kernel<0>), sgrid, dim3(256), 0, st, (const float*)nullptr, feature, per_utt, D, db_threshold, w, stride, frames, F);
  hipLaunchKernelGGL((kmeans2_count_kernel<true>), sgrid, dim3(256), 0, st, feature, per_utt, db_threshold, w, stride, iw, frames, F, D);
  hipLaunchKernelGGL(kmeans2_index_kernel, sgrid, dim3(256), 0, st, feature, per_utt, db_threshold, (const float*)w, stride, iw, l.at<int>(ws, l.dest), frames, F, D);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_dc_cluster_compact_f32(int B, int T, int F, int D, int iters, float tol, float* masks, void* ws, size_t ws_bytes,
                                  int flags, void* stream) {
  if (!masks || !ws || B <= 0 || T <= 0 || F <= 0 || D <= 0 || D > km::DMAX || iters < 0 || !(tol >= 0.f)) return ONSSEN_E_ARG;
  if (flags & ONSSEN_DC_CLUSTER_LAUNCH_PER_ITERATION) return ONSSEN_E_ARG;      // the compacted form IS the persistent form
  const DcWs l(B, T, F, D);
  if (ws_bytes < l.compact_bytes) return ONSSEN_E_WORKSPACE;
  if (reinterpret_cast<uintptr_t>(ws) & 255u) return ONSSEN_E_ALIGN;
  ONSSEN_CLEAR_ERROR();
  hipStream_t st = (hipStream_t)stream;
  const long per_utt = (long)T * F;
  launch_lloyd<true>(st, l, ws, B, per_utt, D, iters, tol);
  dispatch_d(D, [&](auto dt) { hipLaunchKernelGGL((kmeans2_mask_compact_kernel<decltype(dt)::value>), dim3(km::NBLK * 4, (unsigned)B), dim3(256), 0, st,
                                                  l.at<const float>(ws, l.comp), l.at<const int>(ws, l.dest), per_utt, D, (const float*)ws, l.stride, masks); });
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}
