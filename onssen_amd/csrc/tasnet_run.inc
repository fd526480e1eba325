// Conv-TasNet: the network's launch sequence, once.  tas::run walks encoder -> bottleneck -> the R X blocks -> masks -> decoder
// over a Plan (tasnet.inc) for all four entries; it comes last because it launches kernels of tasnet.inc, tasnet_bwd.inc
// (tas_residual_out_kernel) and tasnet_stream.inc.  p.kind picks the launch of the four boundary-aware steps; the pointers pick
// the variant (u != c: tas_prelu_stats_kernel<true>, xi != xo: tas_residual_out_kernel, logits != d: tas_mask_kernel<true>),
// so an in-place run never enters a saving variant with aliased __restrict__ pointers.

namespace tas {

static int run(const Cfg& g, const void* image, const Plan& p, void* stream) {
  const Layout o = layout(g);
  ONSSEN_CLEAR_ERROR();
  hipStream_t st = (hipStream_t)stream;
  const char* im = static_cast<const char*>(image);
  auto fi = [&](size_t off) { return reinterpret_cast<const float*>(im + off); };
  auto ui = [&](size_t off) { return reinterpret_cast<const uint16_t*>(im + off); };
  const int n = p.n, T = p.T, hop = g.L / 2;
  const long M = p.M;
  const Geo* q = p.geo;
  // K1: encoder + LayerN_S (a stream's reads the staging rows [carried hop | new samples]), then the bottleneck
  const float* x = p.x;
  long x_s = p.x_stride;
  if (p.kind == STREAM) {
    x = p.stage;
    x_s = (long)(T + 1) * hop;
    hipLaunchKernelGGL(tas_stream_stage_kernel, dim3(ew_grid(n * x_s)), dim3(256), 0, st, p.x, p.x_stride, n, T, hop, p.carry_x, p.cnt,
                       p.stage);
  }
  if (p.kind == RAGGED)
    hipLaunchKernelGGL(tas_encoder_ragged_kernel, dim3((unsigned)ceil_div((int)M, 4)), dim3(256), 0, st, x, x_s, q->st, g.N, g.L,
                       fi(o.enc_w), fi(o.enc_b), fi(o.ln_g), fi(o.ln_b), p.w, p.e);
  else
    hipLaunchKernelGGL(tas_encoder_kernel, dim3((unsigned)ceil_div((int)M, 4)), dim3(256), 0, st, x, x_s, T, M, g.N, g.L, fi(o.enc_w),
                       fi(o.enc_b), fi(o.ln_g), fi(o.ln_b), p.w, p.e);
  ONSSEN_LAUNCH_CHECK();
  int rc = gemm(g, ONSSEN_TASNET_EXACT_BOTTLENECK, p.e, M, g.N, fi(o.bott_w), ui(o.bott_x3), fi(o.bott_b), g.B,
                reinterpret_cast<float*>(p.xs), p.img, stream);
  if (rc) return rc;
  const int nch = ceil_div(T, ROWS_PER_CHUNK);
  char* hist_at = p.hist;
  for (int j = 0; j < g.R * g.X; ++j) {
    const size_t k = o.blk0 + (size_t)j * o.blk_stride, k3 = o.x3_blk0 + (size_t)j * o.x3_blk_stride;
    const int dil = 1 << (j % g.X), pad_l = pad_left(g, dil);
    float *xi = reinterpret_cast<float*>(p.xs + j * p.x_step), *xo = reinterpret_cast<float*>(p.xs + (j + 1) * p.x_step);
    float *u = reinterpret_cast<float*>(p.u + j * p.blk_step), *y = reinterpret_cast<float*>(p.y + j * p.blk_step);
    double* part = reinterpret_cast<double*>(p.st + j * p.blk_step);      // gLN partial sums | cLN rows: one region
    float* rstat = reinterpret_cast<float*>(part);
    rc = gemm(g, ONSSEN_TASNET_EXACT_CONV1X1, xi, M, g.B, fi(k + o.c1_w), ui(k3 + o.c1_x3), fi(k + o.c1_b), g.H, u, p.img, stream);
    if (rc) return rc;
    if (p.kind == RAGGED) {                   // in place only
      hipLaunchKernelGGL(tas_prelu_stats_ragged_kernel, dim3((unsigned)q->st.blk[n]), dim3(256), 0, st, p.c, q->st, g.H, fi(k + o.alpha),
                         g.norm, part, rstat);
      hipLaunchKernelGGL(tas_dwconv_ragged_kernel, dim3((unsigned)q->dwc.blk[n]), dim3(256), 0, st, p.c, q->dwc, q->cs, g.H, g.P, dil,
                         pad_l, g.norm, part, rstat, fi(k + o.n_a), fi(k + o.n_b), fi(k + o.dw_w), fi(k + o.dw_b), y);
    } else {
      if (u != p.c)
        hipLaunchKernelGGL(tas_prelu_stats_kernel<true>, dim3((unsigned)nch, (unsigned)n), dim3(256), 0, st, p.c, T, g.H, fi(k + o.alpha),
                           g.norm, part, rstat, (const float*)u);
      else
        hipLaunchKernelGGL(tas_prelu_stats_kernel<false>, dim3((unsigned)nch, (unsigned)n), dim3(256), 0, st, p.c, T, g.H, fi(k + o.alpha),
                           g.norm, part, rstat, (const float*)nullptr);
      if (p.kind == STREAM) {                 // taps before the chunk come from the block's ring, refreshed behind the launch
        const int hs = stream_history(g, j);
        size_t stat_off;
        const size_t hbytes = stream_block_bytes(g, n, j, &stat_off);
        float *hist = reinterpret_cast<float*>(hist_at), *hstat = reinterpret_cast<float*>(hist_at + stat_off);
        hist_at += hbytes;
        hipLaunchKernelGGL(tas_stream_dwconv_kernel, dim3((unsigned)ceil_div(T, DW_ROWS), (unsigned)n), dim3(256), 0, st,
                           (const float*)p.c, T, g.H, g.P, dil, g.norm, (const float*)rstat, (const float*)hist, (const float*)hstat,
                           (const long long*)p.cnt, fi(k + o.n_a), fi(k + o.n_b), fi(k + o.dw_w), fi(k + o.dw_b), y);
        if (hs > 0)
          hipLaunchKernelGGL(tas_stream_history_kernel, dim3((unsigned)(T < hs ? T : hs), (unsigned)n), dim3(256), 0, st,
                             (const float*)p.c, T, g.H, hs, g.norm, (const float*)rstat, (const long long*)p.cnt, hist, hstat);
      } else {
        hipLaunchKernelGGL(tas_dwconv_kernel, dim3((unsigned)ceil_div(T, DW_ROWS), (unsigned)n), dim3(256), 0, st, p.c, T, g.H, g.P, dil,
                           pad_l, g.norm, part, nch, rstat, fi(k + o.n_a), fi(k + o.n_b), fi(k + o.dw_w), fi(k + o.dw_b), y);
      }
    }
    ONSSEN_LAUNCH_CHECK();
    rc = gemm(g, ONSSEN_TASNET_EXACT_SC_CONV, y, M, g.H, fi(k + o.sc_w), ui(k3 + o.sc_x3), fi(k + o.sc_b), g.B, p.t, p.img, stream);
    if (rc) return rc;
    if (xi != xo)
      hipLaunchKernelGGL(tas_residual_out_kernel, dim3(ew_grid(M * g.B)), dim3(256), 0, st, xo, xi, p.t, M * g.B);
    else
      hipLaunchKernelGGL(tas_residual_kernel, dim3(ew_grid(M * g.B)), dim3(256), 0, st, xi, p.t, M * g.B);
    ONSSEN_LAUNCH_CHECK();
  }
  rc = gemm(g, ONSSEN_TASNET_EXACT_MASKS, reinterpret_cast<float*>(p.xs + (size_t)(g.R * g.X) * p.x_step), M, g.B, fi(o.mask_w),
            ui(o.mask_x3), fi(o.mask_b), g.spk * g.N, p.logits, p.img, stream);
  if (rc) return rc;
  if (p.logits != p.d)
    hipLaunchKernelGGL(tas_mask_kernel<true>, dim3(ew_grid(M * g.N)), dim3(256), 0, st, p.d, p.w, M, g.N, g.spk, g.act,
                       (const float*)p.logits);
  else
    hipLaunchKernelGGL(tas_mask_kernel<false>, dim3(ew_grid(M * g.N)), dim3(256), 0, st, p.d, p.w, M, g.N, g.spk, g.act,
                       (const float*)nullptr);
  if (p.kind == RAGGED)
    hipLaunchKernelGGL(tas_decoder_ragged_kernel, dim3((unsigned)q->dec.blk[n], (unsigned)g.spk), dim3(256), 0, st, p.d, q->dec, g.N,
                       g.L, g.spk, fi(o.dec_w), fi(o.dec_b), p.out, q->out_stride);
  else if (p.kind == STREAM)
    hipLaunchKernelGGL(tas_stream_decoder_kernel, dim3((unsigned)ceil_div(T, DEC_FRAMES), (unsigned)n, (unsigned)g.spk), dim3(256), 0,
                       st, (const float*)p.d, T, g.N, g.L, g.spk, fi(o.dec_w), fi(o.dec_b), (const long long*)p.cnt, p.carry_d, p.out);
  else
    hipLaunchKernelGGL(tas_decoder_kernel, dim3((unsigned)ceil_div(T + 1, DEC_FRAMES), (unsigned)n, (unsigned)g.spk), dim3(256), 0, st,
                       p.d, T, g.N, g.L, g.spk, fi(o.dec_w), fi(o.dec_b), p.out, p.S_out);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

}  // namespace tas
