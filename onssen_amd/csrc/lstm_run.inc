// BLSTM host side (part of onssen_hip.hip; after lstm.inc, lstm_bwd.inc and gemm.inc, whose kernels and ABI entries it launches):
// ONE geometry (LstmGeo), ONE layout per workspace (BlstmWs, Pipe2Ws), ONE rows-per-group rule, ONE ug dispatch, the launchers
// of the recurrence kernels, and the entries over them -- stack forward (uniform / ragged / training), the pipelined pair,
// the backward recurrence, and the workspace and image queries.  blstm_forward_impl reads top to bottom: plan, then per layer
// "project" (input-projection GEMM) and "recur" (persistent launch or one launch per step).

// ---- geometry: everything that follows from (H, ug) -------------------------------------------------------------------
struct LstmGeo {
  int ug, Hp, NP, NU;   // hidden units per workgroup; H rounded up to it; gate columns 4 Hp; workgroups per direction Hp / ug
  int KQ;               // 16-wide k-chunks of the fp32 step kernel
  int KQ2, Hs;          // 32-wide k-chunks of the split-bf16 forms, padded row length 32 KQ2
  int KQB, NUB;         // backward: 32-wide k-chunks over the NP gate columns, 16-unit tiles over Hp
};
static bool lstm_geo(int H, int ug, LstmGeo* g) {
  if (H <= 0 || ug < 4 || ug > 24 || (ug % 4) != 0) return false;
  g->ug = ug; g->Hp = ceil_div(H, ug) * ug; g->NP = 4 * g->Hp; g->NU = g->Hp / ug;
  g->KQ = ceil_div(g->Hp, 16); g->KQ2 = ceil_div(g->Hp, 32); g->Hs = 32 * g->KQ2;
  g->KQB = ceil_div(g->NP, 32); g->NUB = ceil_div(g->Hp, 16);
  return true;
}
// the exported and the pack entries' views of it
int onssen_lstm_geometry(int H, int ug, int* Hp, int* NP, int* KQ, int64_t* whh_elems) {
  LstmGeo g;
  if (!lstm_geo(H, ug, &g)) return ONSSEN_E_ARG;
  if (Hp) *Hp = g.Hp;
  if (NP) *NP = g.NP;
  if (KQ) *KQ = g.KQ;
  if (whh_elems) *whh_elems = (int64_t)g.NU * g.KQ * (ug / 4) * 256;
  return ONSSEN_OK;
}
int onssen_lstm_geometry_x3(int H, int ug, int* KQ2, int* Hs, int64_t* whh_x3_elems) {
  LstmGeo g;
  if (!lstm_geo(H, ug, &g)) return ONSSEN_E_ARG;
  if (KQ2) *KQ2 = g.KQ2;
  if (Hs) *Hs = g.Hs;
  if (whh_x3_elems) *whh_x3_elems = (int64_t)g.NU * g.KQ2 * (ug / 4) * 1024;
  return ONSSEN_OK;
}
static bool lstm_bwd_geometry(int H, int ug, int* Hp, int* NP, int* KQB, int* NUB) {
  LstmGeo g;
  if (!lstm_geo(H, ug, &g)) return false;
  *Hp = g.Hp; *NP = g.NP; *KQB = g.KQB; *NUB = g.NUB;
  return true;
}

// ug -> compile-time constant: f(std::integral_constant<int, UG>) for the validated ug = 4, 8, .. 24.  TOP is the widest
// instantiation the site has; a ug above it runs TOP's.  (Only the persistent forward has ug = 24 kernels: the launch-per-step
// forward and the backward run their ug = 20 ones on the ug = 24 geometry -- unintended as far as anyone knows, and kept.)
template <int TOP, class F>
static int dispatch_ug(int ug, F&& f) {
  static_assert(TOP == 20 || TOP == 24, "the sites' widest instantiations");
  switch (ug < TOP ? ug : TOP) {
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    case 12: return f(std::integral_constant<int, 12>{});
    case 16: return f(std::integral_constant<int, 16>{});
    case 20: return f(std::integral_constant<int, 20>{});
    default: return f(std::integral_constant<int, TOP>{});
  }
}

// rows per exchange group of the persistent kernels, forward (every NT) and backward: the smallest of 4 / 8 / 16 that still covers
// the batch with the chip's 8 groups per launch (2 directions x 4).  Ragged batches promise every row the bits of its own batch-1
// run, which is a STACKED 4-row group: the stacked tile adds the lo x lo products that the 16-row form drops, so more than 32
// rows run as several launches of 8-row groups instead
static int xcd_rows_per_group(int B, bool ragged) {
  static const int rg_env = ONSSEN_KNOB_INT("ONSSEN_XCD_RG", 0);   // profiling: force 4 / 8 / 16
  if (ragged) return B <= 16 ? 4 : 8;
  if (rg_env == 4 || rg_env == 8 || rg_env == 16) return rg_env;
  return B <= 16 ? 4 : B <= 32 ? 8 : 16;
}

// ---- workspace layouts: byte offsets from the (256-byte aligned) base, whose first ONSSEN_BLSTM_WS_HEADER_BYTES are the sync block --
constexpr size_t WS_DEBUG_BYTES = 65536;        // the tail of both workspaces: debug timestamps
static size_t ws_gates_bytes(int T, int B, const LstmGeo& g) { return align256((size_t)T * B * 2 * g.NP * sizeof(float)); }
static size_t ws_image_bytes(int T, int B, int K) { return align256((size_t)T * B * ceil_div(K, 32) * 128); }     // x3 image [T*B][KB][2][32]
// h hand-off images: [2 slots][KQ2 chunks][2 KiB] per exchange group -- split-bf16; >= the fp32 image (2 KQ2 >= KQ)
static size_t ws_handoff_bytes(int groups, const LstmGeo& g) { return (size_t)groups * 2 * g.KQ2 * 2048; }

// the stack: header | G | ybuf (L > 1) | c | h hand-off | x3 images: layer-0 input, output A (the LAST layer's), output B (L > 1) | debug
struct BlstmWs {
  size_t g, y, c, hs, hs_bytes, img_x, img_a, img_b, dbg, total;    // hs_bytes: the images themselves, before padding to 256
};
static bool blstm_ws_layout(int B, int T, int in_dim, int L, const LstmGeo& g, BlstmWs* w) {
  if (B <= 0 || T <= 0 || L <= 0 || in_dim <= 0) return false;
  w->hs_bytes = ws_handoff_bytes(2 * ceil_div(B, 4), g);          // one group per (direction, >= 4 rows)
  w->g = ONSSEN_BLSTM_WS_HEADER_BYTES;
  w->y = w->g + ws_gates_bytes(T, B, g);
  w->c = w->y + (L > 1 ? align256((size_t)T * B * 2 * g.Hp * sizeof(float)) : 0);
  w->hs = w->c + align256((size_t)2 * B * g.Hp * sizeof(float));
  w->img_x = w->hs + align256(w->hs_bytes);
  w->img_a = w->img_x + ws_image_bytes(T, B, in_dim);
  w->img_b = w->img_a + ws_image_bytes(T, B, 2 * g.Hp);
  w->dbg = w->img_b + (L > 1 ? ws_image_bytes(T, B, 2 * g.Hp) : 0);
  w->total = w->dbg + WS_DEBUG_BYTES;
  return true;
}
// the pipelined pair: header | G0 | G1 | h hand-off of 8 groups | x3 images: input, layer-0 output, layer-1 output | debug
struct Pipe2Ws {
  size_t g0, g1, hs, img_x, img0, img1, dbg, total;
};
static bool pipe2_ws_layout(int B, int T, int in_dim, const LstmGeo& g, Pipe2Ws* w) {
  if (B <= 0 || B > 32 || T <= 0 || in_dim <= 0) return false;
  w->g0 = ONSSEN_BLSTM_WS_HEADER_BYTES;
  w->g1 = w->g0 + ws_gates_bytes(T, B, g);
  w->hs = w->g1 + ws_gates_bytes(T, B, g);
  w->img_x = w->hs + align256(ws_handoff_bytes(8, g));
  w->img0 = w->img_x + ws_image_bytes(T, B, in_dim);
  w->img1 = w->img0 + ws_image_bytes(T, B, 2 * g.Hp);
  w->dbg = w->img1 + ws_image_bytes(T, B, 2 * g.Hp);
  w->total = w->dbg + WS_DEBUG_BYTES;
  return true;
}

size_t onssen_blstm_workspace_bytes(int B, int T, int in_dim, int H, int L, int ug) {
  LstmGeo g;
  BlstmWs w;
  return lstm_geo(H, ug, &g) && blstm_ws_layout(B, T, in_dim, L, g, &w) ? w.total : 0;
}
int onssen_blstm_y_image(int B, int T, int in_dim, int H, int L, int ug, size_t* offset_bytes, int* KB) {
  LstmGeo g;
  BlstmWs w;
  if (!lstm_geo(H, ug, &g) || !blstm_ws_layout(B, T, in_dim, L, g, &w)) return ONSSEN_E_ARG;
  if (offset_bytes) *offset_bytes = w.img_a;
  if (KB) *KB = ceil_div(2 * g.Hp, 32);
  return ONSSEN_OK;
}
int onssen_blstm_x_image(int B, int T, int in_dim, int H, int L, int ug, size_t* offset_bytes, int* KB) {
  LstmGeo g;
  BlstmWs w;
  if (!lstm_geo(H, ug, &g) || !blstm_ws_layout(B, T, in_dim, L, g, &w)) return ONSSEN_E_ARG;
  if (offset_bytes) *offset_bytes = w.img_x;
  if (KB) *KB = ceil_div(in_dim, 32);
  return ONSSEN_OK;
}
size_t onssen_blstm_pipe2_workspace_bytes(int B, int T, int in_dim, int H, int ug) {
  LstmGeo g;
  Pipe2Ws w;
  return lstm_geo(H, ug, &g) && pipe2_ws_layout(B, T, in_dim, g, &w) ? w.total : 0;
}
int onssen_blstm_pipe2_y_image(int B, int T, int in_dim, int H, int ug, size_t* offset_bytes, int* KB) {
  LstmGeo g;
  Pipe2Ws w;
  if (!lstm_geo(H, ug, &g) || !pipe2_ws_layout(B, T, in_dim, g, &w)) return ONSSEN_E_ARG;
  if (offset_bytes) *offset_bytes = w.img1;
  if (KB) *KB = ceil_div(2 * g.Hp, 32);
  return ONSSEN_OK;
}

// ---- launchers ------------------------------------------------------------------------------------------------------
// what the stack's and the pair's persistent launches share: geometry, sync block, hand-off images, spin limit, ablation
static XcdArgs xcd_args(const LstmGeo& g, void* ws, size_t hs_offset, int B, int flags) {
  XcdArgs xa;
  xa.sync = (unsigned*)ws; xa.hx = (unsigned short*)((char*)ws + hs_offset); xa.B = B;
  xa.Hp = g.Hp; xa.NP = g.NP; xa.KQ2 = g.KQ2; xa.NU = g.NU; xa.KBI = ceil_div(2 * g.Hp, 32);
  xa.spin_limit = xcd_spin_limit(); xa.ablate = (flags >> 8) & 8;
  return xa;
}

// One layer on the persistent kernel: <= 4 batch groups per launch (2 directions x 4 = the chip's 8 XCDs).
// NT = 6 (ug = 24, 640 < H <= 768, round 4: 32 members = every CU of the XCD, W_hh takes 144 of the 256 registers) exists for the
// plain split-bf16 recurrence only: stacked / unstacked / ragged, and the training forward with saved state
template <int NT>
static int launch_xcd(XcdArgs xa, hipStream_t st) {
  const bool fz = xa.KC0 > 0;
  if (NT == 6 && (xa.terms != 3 || fz || (xa.save_c && xa.frames))) return ONSSEN_E_ARG;
  xa.RG = xcd_rows_per_group(xa.B, xa.frames != nullptr);
  static const int stack_env = ONSSEN_KNOB_INT("ONSSEN_XCD_STACK", 1);   // profiling: 0 = never stack
  const bool stack = xa.RG <= 8 && xa.terms == 3 && stack_env != 0;
  if (xa.frames && !stack) return ONSSEN_E_ARG;
  const dim3 grid((unsigned)(8 * xa.NU));
#define ONSSEN_XCD_LAUNCH(FZ_, TERMS_, STACK_, SAVE_, RAGGED_) \
  hipLaunchKernelGGL((lstm_xcd_kernel<NT, 8, FZ_, TERMS_, STACK_, SAVE_, RAGGED_>), grid, dim3(512), 0, st, xa)
  for (int r0 = 0; r0 < xa.B; r0 += 4 * xa.RG) {
    const int rows = xa.B - r0 < 4 * xa.RG ? xa.B - r0 : 4 * xa.RG;
    xa.row0 = r0;
    xa.nbg = ceil_div(rows, xa.RG);
    if (xa.frames) {               // ragged batch of whole utterances (split-bf16, unfused, inference)
      ONSSEN_XCD_LAUNCH(false, 3, true, false, true);
    } else if (xa.save_c) {        // training forward: keeps gates and cell states for the backward kernels
      if (stack) ONSSEN_XCD_LAUNCH(false, 3, true, true, false); else ONSSEN_XCD_LAUNCH(false, 3, false, true, false);
    } else if (xa.terms == 3 && !fz) {
      if (stack) ONSSEN_XCD_LAUNCH(false, 3, true, false, false); else ONSSEN_XCD_LAUNCH(false, 3, false, false, false);
    } else if constexpr (NT < 6) {
      if (xa.terms == 0) {         // exact fp32 (no ONSSEN_BLSTM_BF16X3)
        ONSSEN_XCD_LAUNCH(false, 0, false, false, false);
      } else if (xa.terms == 1) {  // plain bf16 products (ONSSEN_BLSTM_BF16)
        if (fz) ONSSEN_XCD_LAUNCH(true, 1, false, false, false); else ONSSEN_XCD_LAUNCH(false, 1, false, false, false);
      } else {                     // fused first layer
        if (stack) ONSSEN_XCD_LAUNCH(true, 3, true, false, false); else ONSSEN_XCD_LAUNCH(true, 3, false, false, false);
      }
    }
  }
#undef ONSSEN_XCD_LAUNCH
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? ONSSEN_OK : (int)e;
}

// PAIR launch (XcdArgs::nbg_a): two plain split-bf16 recurrences over the same B <= 32 rows in ONE launch, each on its own half of
// the XCDs.  Its rows per group are NOT xcd_rows_per_group's: each recurrence has 4 of the 8 groups (2 directions x 2), so 16
// rows already need 8-row groups (stacked) and more need 16-row groups (the unstacked three-term tile)
template <int NT>
static int launch_xcd_pair(XcdArgs xa, hipStream_t st) {
  if (xa.B > 32 || xa.terms != 3 || xa.KC0 > 0 || xa.save_c || !xa.G_b || !xa.whh_b || !xa.yimg_b) return ONSSEN_E_ARG;
  // ragged rows promise the bits of their own batch-1 run, which is a stacked tile: <= 16 rows (8-row groups), both halves ragged
  if ((xa.frames != nullptr) != (xa.frames_b != nullptr) || (xa.frames && xa.B > 16)) return ONSSEN_E_ARG;
  xa.RG = xa.B <= 16 ? 8 : 16;
  xa.row0 = 0;
  xa.nbg_a = ceil_div(xa.B, xa.RG);
  xa.nbg = 2 * xa.nbg_a;
  // aux workgroups (uniform pairs only): at the END of the grid, so that the dispatcher hands them out after every member
  if (xa.aux_n < 0 || (xa.aux_n > 0 && xa.frames)) return ONSSEN_E_ARG;
  const dim3 grid((unsigned)(8 * xa.NU + xa.aux_n));
  if (xa.frames) hipLaunchKernelGGL((lstm_xcd_kernel<NT, 8, false, 3, true, false, true>), grid, dim3(512), 0, st, xa);
  else if (xa.aux_n > 0 && xa.RG == 8) hipLaunchKernelGGL((lstm_xcd_kernel<NT, 8, false, 3, true, false, false, true>), grid, dim3(512), 0, st, xa);
  else if (xa.aux_n > 0) hipLaunchKernelGGL((lstm_xcd_kernel<NT, 8, false, 3, false, false, false, true>), grid, dim3(512), 0, st, xa);
  else if (xa.RG == 8) hipLaunchKernelGGL((lstm_xcd_kernel<NT, 8, false, 3, true, false>), grid, dim3(512), 0, st, xa);
  else hipLaunchKernelGGL((lstm_xcd_kernel<NT, 8, false, 3, false, false>), grid, dim3(512), 0, st, xa);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? ONSSEN_OK : (int)e;
}

// ---- the stack forward ------------------------------------------------------------------------------------------------
struct BlstmRun {      // one call: what the caller passed, and what validation and the layout made of it
  const float* x; int64_t xs_b, xs_t; int B, T, in_dim, L, flags;
  const float* const* wih; const float* const* whh; const float* const* bias;
  float *y, *save_g, *save_c; const int32_t* frames; void* stream;
  LstmGeo g; BlstmWs o; char* ws;
  float *G, *ybuf; uint16_t *img_x, *img_ab[2]; long long* dbg;
  bool x3, xcd;
  bool images;      // XCD form: activations travel between the layers (and on to the heads) as x3 images written by the recurrence
                    // epilogue; wih[l] is then the x3 image of the [2*NP][K_l] input-projection matrix
  bool bf16_only;   // plain bf16 products instead of the three-term split
  // the first layer's input projection is computed inside its recurrence launch: no G, no GEMM
  bool fuse0(int l) const { return images && l == 0 && (flags & ONSSEN_BLSTM_FUSE_IN0); }
  // the last layer writes `y`; the layers before it alternate so that each reads what the previous wrote
  float* yout(int l) const { return (L - 1 - l) % 2 == 0 ? y : ybuf; }
  const float* yin(int l) const { return (L - 1 - l) % 2 == 0 ? ybuf : y; }
};

// validation and layout
static int blstm_plan(BlstmRun& r, int H, int ug, void* ws, size_t ws_bytes) {
  const int flags = r.flags;
  if (!lstm_geo(H, ug, &r.g)) return ONSSEN_E_ARG;
  if (!r.x || !ws || !r.wih || !r.whh || !r.bias || !blstm_ws_layout(r.B, r.T, r.in_dim, r.L, r.g, &r.o)) return ONSSEN_E_ARG;
  // y may be NULL only in the XCD form, whose consumers can take the x3 image of the output instead
  if (!r.y && !((flags & ONSSEN_BLSTM_XCD) && (flags & ONSSEN_BLSTM_BF16X3))) return ONSSEN_E_ARG;
  // ragged batches: the persistent form exists for the plain split-bf16 inference recurrence (no fused first layer, no
  // bf16-only products, no saved state); the launch-per-step form takes them in both precisions
  if (r.frames && (flags & ONSSEN_BLSTM_XCD) &&
      (!(flags & ONSSEN_BLSTM_BF16X3) || (flags & (ONSSEN_BLSTM_FUSE_IN0 | ONSSEN_BLSTM_BF16)) || r.save_g || r.save_c))
    return ONSSEN_E_ARG;
  if (ws_bytes < r.o.total) return ONSSEN_E_WORKSPACE;
  if (!aligned256(ws) || (r.y && !aligned16(r.y))) return ONSSEN_E_ALIGN;
  r.x3 = (flags & ONSSEN_BLSTM_BF16X3) != 0;
  r.xcd = (flags & ONSSEN_BLSTM_XCD) != 0;
  if (r.x3 && !r.xcd && r.g.KQ2 > 4 * rec::QB3) return ONSSEN_E_ARG;   // H <= 640 in the launch-per-step split-bf16 form
  r.images = r.x3 && r.xcd;
  r.bf16_only = r.images && (flags & ONSSEN_BLSTM_BF16);
  r.ws = (char*)ws;
  r.G = (float*)(r.ws + r.o.g);
  r.ybuf = r.L > 1 ? (float*)(r.ws + r.o.y) : nullptr;
  r.img_x = (uint16_t*)(r.ws + r.o.img_x);
  r.img_ab[0] = (uint16_t*)(r.ws + r.o.img_a);
  r.img_ab[1] = (uint16_t*)(r.ws + r.o.img_b);
  r.dbg = ((flags >> 8) & 32) && r.T * 8 * sizeof(long long) <= WS_DEBUG_BYTES ? (long long*)(r.ws + r.o.dbg) : nullptr;
  return ONSSEN_OK;
}

// ONSSEN_BLSTM_WS_DIRTY: the k padding of a recurrence output image (columns 2*Hp .. 32*KB - 1 of every row) is never written by
// the recurrence; a workspace that was not zeroed for this shape gets it cleared here (stale bits there could be bf16 NaNs,
// and NaN x 0-weight = NaN in the next GEMM)
extern "C" __global__ void x3_pad_zero_kernel(unsigned short* __restrict__ img, long rows, int KB, int K) {
  const int k0 = K & 31;                         // first padding column inside the last k block (0: no padding)
  if (k0 == 0) return;
  const int per = 32 - k0;
  const long total = rows * 2 * per;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const long row = e / (2 * per);
    const int r = (int)(e - row * 2 * per), hl = r / per, kk = k0 + r % per;
    img[(row * KB + (KB - 1)) * 64 + hl * 32 + kk] = 0;
  }
}

// layer l's input projection G = in_l W_ih^T + b, by the GEMM of the call's form
static int blstm_project(const BlstmRun& r, int l) {
  const int B = r.B, T = r.T, in_dim = r.in_dim, Hp = r.g.Hp, NP = r.g.NP;
  const bool fuse0 = r.fuse0(l);
  // the fused projection keeps <= 4 k-chunks of W_ih fragments in the LDS: in_dim <= 128, or 32k + 1 <= 129 with FUSE_TAIL
  if (fuse0 && !(in_dim <= 128 || (in_dim == 129 && (r.flags & ONSSEN_BLSTM_FUSE_TAIL)))) return ONSSEN_E_ARG;
  if ((r.flags & ONSSEN_BLSTM_G_READY) && !fuse0) return ONSSEN_OK;   // profiling: G of this layer is what an earlier call left in the workspace
  if (r.images) {
    if (l == 0) {
      const int rc = onssen_x3_image_f32(r.x, r.xs_t, r.xs_b, B, T * B, in_dim, r.img_x, r.stream);
      if (rc != ONSSEN_OK || fuse0) return rc;
    }
    const uint16_t* a_img = l == 0 ? r.img_x : r.img_ab[(r.L - l) % 2];   // layer l-1 wrote buffer (L-1-(l-1)) % 2
    return onssen_linear_x3p(a_img, T * B, l == 0 ? in_dim : 2 * Hp, (const uint16_t*)r.wih[l], r.bias[l], 2 * NP,
                             ONSSEN_EPI_BIAS | (r.bf16_only ? ONSSEN_EPI_BF16 : 0), 0, 0.f, r.G, B, (int64_t)B * 2 * NP, 2 * NP, r.stream);
  }
  if (r.x3) {   // wih[l]: split-bf16 planes [2][2*NP][ld], ld = K rounded up to 32
    const int K = l == 0 ? in_dim : 2 * Hp, ld = ceil_div(K, 32) * 32;
    return onssen_linear_bf16x3(l == 0 ? r.x : r.yin(l), l == 0 ? r.xs_t : (int64_t)B * 2 * Hp, l == 0 ? r.xs_b : 2 * Hp, B, T * B, K,
                                (const uint16_t*)r.wih[l], ld, r.bias[l], 2 * NP, ONSSEN_EPI_BIAS, 0, 0.f, nullptr, r.G,
                                (int64_t)B * 2 * NP, 2 * NP, r.stream);
  }
  if (l == 0)
    return onssen_linear_f32(r.x, r.xs_t, r.xs_b, B, T * B, in_dim, r.wih[0], ceil_div(in_dim, 4) * 4, r.bias[0], 2 * NP, ONSSEN_EPI_BIAS,
                             0, 0.f, nullptr, r.G, (int64_t)B * 2 * NP, 2 * NP, r.stream);
  return onssen_linear_f32(r.yin(l), (int64_t)B * 2 * Hp, 2 * Hp, B, T * B, 2 * Hp, r.wih[l], 2 * Hp, r.bias[l], 2 * NP, ONSSEN_EPI_BIAS, 0,
                           0.f, nullptr, r.G, (int64_t)B * 2 * NP, 2 * NP, r.stream);
}

// layer l, one launch per time step.  The kernel takes G, c and the hand-off images as 256-byte offsets from the workspace base
template <int MT, int NT>
static int launch_steps(const BlstmRun& r, int l) {
  const dim3 grid((unsigned)r.g.NU, 2, (unsigned)ceil_div(r.B, 16 * MT)), block(256);
  const unsigned g_off = (unsigned)(r.o.g / 256), c_off = (unsigned)(r.o.c / 256), hs_off = (unsigned)(r.o.hs / 256);
  const int ablate = (r.flags >> 8) & 63;
  const bool dbg_form = ablate || r.dbg || r.frames || r.save_g;   // the instantiations that read the arguments past the preloaded ones
  const void* w = r.whh[l];
  hipStream_t st = (hipStream_t)r.stream;
  ONSSEN_CLEAR_ERROR();
#define ONSSEN_STEP_LAUNCH(X3_, DBG_)                                                                                      \
  hipLaunchKernelGGL((lstm_step_kernel<MT, NT, X3_, DBG_>), grid, block, 0, st, w, r.ws, r.yout(l), s, r.B, r.g.NU, r.T, g_off, c_off, \
                     hs_off, ablate, r.dbg, r.frames, r.save_g, r.save_c)
  for (int s = 0; s < r.T; ++s) {
    if (dbg_form) {
      if (r.x3) ONSSEN_STEP_LAUNCH(true, true); else ONSSEN_STEP_LAUNCH(false, true);
    } else {
      if (r.x3) ONSSEN_STEP_LAUNCH(true, false); else ONSSEN_STEP_LAUNCH(false, false);
    }
  }
#undef ONSSEN_STEP_LAUNCH
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? ONSSEN_OK : (int)e;
}

// layer l's recurrence over G: the persistent launch, or one launch per step
static int blstm_recur(const BlstmRun& r, int l) {
  const LstmGeo& g = r.g;
  if (!r.xcd) {
    const int mt = (r.B > 16 && !(r.flags & ONSSEN_BLSTM_SPLIT_ROWS)) ? 2 : 1;
    return dispatch_ug<20>(g.ug, [&](auto ugc) {
      constexpr int NT = decltype(ugc)::value / 4;
      return mt == 1 ? launch_steps<1, NT>(r, l) : launch_steps<2, NT>(r, l);
    });
  }
  // without ONSSEN_BLSTM_BF16X3: the exact-fp32 instantiation (whh[l] = the fp32 fragment image of onssen_lstm_pack_f32, G from
  // the exact-fp32 GEMM, fp32 rows between the layers).  split-bf16: H <= 768 (ug = 24: 32 members of 24 units = every CU of an
  // XCD; round 4), exact fp32 and the forms that fuse the first layer / save state: H <= 640 (ug <= 20)
  const bool fuse0 = r.fuse0(l);
  if (g.NU > 32 || g.KQ2 > 24 || (!r.x3 && (r.save_g || r.save_c))) return ONSSEN_E_ARG;
  if (g.ug > 20 && (!r.x3 || fuse0 || (r.flags & ONSSEN_BLSTM_BF16))) return ONSSEN_E_ARG;
  XcdArgs xa = xcd_args(g, r.ws, r.o.hs, r.B, r.flags);
  xa.G = r.G; xa.whh = (const unsigned short*)r.whh[l]; xa.T = r.T; xa.frames = r.frames; xa.dbg = r.dbg;
  // fp32 rows only where somebody reads them (the caller's y); every layer leaves its x3 image
  xa.y = r.x3 ? (l == r.L - 1 ? r.y : nullptr) : r.yout(l);
  xa.yimg = r.x3 ? r.img_ab[(r.L - 1 - l) % 2] : nullptr;
  xa.terms = !r.x3 ? 0 : r.bf16_only ? 1 : 3;
  xa.save_g = r.save_g; xa.save_c = r.save_c;
  xa.ximg = r.img_x; xa.bias0 = r.bias[0]; xa.x0 = r.x; xa.xs_b = (long)r.xs_b; xa.xs_t = (long)r.xs_t;
  if (fuse0) {
    xa.wih0 = (const unsigned short*)r.wih[0];
    xa.KC0 = xa.KCM = ceil_div(r.in_dim, 32);
    // in_dim = 32k + 1 (F = 129): the lone last column goes to the VALU; its weights follow the bias (FUSE_TAIL)
    if ((r.flags & ONSSEN_BLSTM_FUSE_TAIL) && (r.in_dim % 32) == 1 && r.in_dim > 1) {
      xa.KCM = xa.KC0 - 1;
      xa.wtail = r.bias[0] + 2 * g.NP;
    }
  }
  ONSSEN_CLEAR_ERROR();
  return dispatch_ug<24>(g.ug, [&](auto ugc) { return launch_xcd<decltype(ugc)::value / 4>(xa, (hipStream_t)r.stream); });
}

static int blstm_forward_impl(const float* x, int64_t xs_b, int64_t xs_t, int B, int T, int in_dim, int H, int L,
                              int ug, const float* const* wih_p_host, const float* const* whh_p_host,
                              const float* const* bias_p_host, float* y, void* ws, size_t ws_bytes, int flags,
                              void* stream, float* save_g, float* save_c, const int32_t* frames = nullptr) {
  BlstmRun r{x, xs_b, xs_t, B, T, in_dim, L, flags, wih_p_host, whh_p_host, bias_p_host, y, save_g, save_c, frames, stream};
  int rc = blstm_plan(r, H, ug, ws, ws_bytes);
  if (rc != ONSSEN_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (!r.xcd) {   // launch-per-step form: h_{-1} = 0 and the K padding of the hand-off images come from here
    hipError_t e = hipMemsetAsync(r.ws + r.o.hs, 0, r.o.hs_bytes, st);   // (the persistent kernels clear their own slots, K padding
    if (e != hipSuccess) return (int)e;                                   //  included, before their start-up barrier: one launch less per call)
  }
  if (r.images && (flags & ONSSEN_BLSTM_WS_DIRTY) && ((2 * r.g.Hp) & 31)) {
    const long rows = (long)T * B;
    const long n = rows * 2 * (32 - ((2 * r.g.Hp) & 31));
    const unsigned nb = (unsigned)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256);
    for (int i = 0; i < (L > 1 ? 2 : 1); ++i)
      hipLaunchKernelGGL(x3_pad_zero_kernel, dim3(nb), dim3(256), 0, st, r.img_ab[i], rows, ceil_div(2 * r.g.Hp, 32), 2 * r.g.Hp);
  }
  for (int l = 0; l < L; ++l) {
    if ((rc = blstm_project(r, l)) != ONSSEN_OK) return rc;
    if ((rc = blstm_recur(r, l)) != ONSSEN_OK) return rc;
  }
  return ONSSEN_OK;
}

int onssen_blstm_forward_f32(const float* x, int64_t xs_b, int64_t xs_t, int B, int T, int in_dim, int H, int L,
                             int ug, const float* const* wih_p_host, const float* const* whh_p_host,
                             const float* const* bias_p_host, float* y, void* ws, size_t ws_bytes, int flags,
                             void* stream) {
  return blstm_forward_impl(x, xs_b, xs_t, B, T, in_dim, H, L, ug, wih_p_host, whh_p_host, bias_p_host, y, ws, ws_bytes,
                            flags, stream, nullptr, nullptr);
}

int onssen_blstm_forward_ragged_f32(const float* x, int64_t xs_b, int64_t xs_t, int B, int T, const int32_t* frames,
                                    int in_dim, int H, int L, int ug, const float* const* wih_p_host,
                                    const float* const* whh_p_host, const float* const* bias_p_host, float* y, void* ws,
                                    size_t ws_bytes, int flags, void* stream) {
  if (!frames) return ONSSEN_E_ARG;
  return blstm_forward_impl(x, xs_b, xs_t, B, T, in_dim, H, L, ug, wih_p_host, whh_p_host, bias_p_host, y, ws, ws_bytes,
                            flags, stream, nullptr, nullptr, frames);
}

// training (SURVEY row N1): one layer forward with saved state
int onssen_lstm_train_forward_f32(const float* x, int64_t xs_b, int64_t xs_t, int B, int T, int in_dim, int H, int ug,
                                  const uint16_t* wih_img, const uint16_t* whh_x3, const float* bias_p, float* y,
                                  float* gates, float* cs, void* ws, size_t ws_bytes, void* stream) {
  return onssen_lstm_train_forward_form_f32(x, xs_b, xs_t, B, T, in_dim, H, ug, wih_img, whh_x3, bias_p, y, gates, cs, ws, ws_bytes,
                                            ONSSEN_BLSTM_BF16X3 | ONSSEN_BLSTM_XCD, stream);
}

int onssen_lstm_train_forward_form_f32(const float* x, int64_t xs_b, int64_t xs_t, int B, int T, int in_dim, int H, int ug,
                                       const void* wih, const void* whh, const float* bias_p, float* y, float* gates,
                                       float* cs, void* ws, size_t ws_bytes, int flags, void* stream) {
  if (!y || !gates || !cs || !aligned16(gates)) return ONSSEN_E_ARG;
  // the forms that can save state: the persistent split-bf16 launch, and the launch-per-step recurrence in either precision
  const int form = flags & (ONSSEN_BLSTM_XCD | ONSSEN_BLSTM_BF16X3);
  if ((flags & ~(ONSSEN_BLSTM_XCD | ONSSEN_BLSTM_BF16X3)) != 0 || form == ONSSEN_BLSTM_XCD) return ONSSEN_E_ARG;
  const float* wih_a[1] = {(const float*)wih};
  const float* whh_a[1] = {(const float*)whh};
  const float* bias[1] = {bias_p};
  return blstm_forward_impl(x, xs_b, xs_t, B, T, in_dim, H, 1, ug, wih_a, whh_a, bias, y, ws, ws_bytes, flags, stream, gates, cs);
}

// ---- two-layer stack, software-pipelined over consecutive calls (round 6) -------------------------------------------
// T_cap lays the workspace out (>= every T that passes through it); the uniform form has T_cap = T = T_prev and no frames
// the target map of THIS batch, built by spare workgroups of the pair launch (uniform form): the clustering workspace, or all null / zero
struct Pipe2Map { float db = 0.f; int D = 0; void* ws = nullptr; size_t ws_bytes = 0; };
static int blstm_pipe2_impl(const float* x, int64_t xs_b, int64_t xs_t, int B, int T_cap, int T, const int32_t* frames, int T_prev,
                            const int32_t* frames_prev, int in_dim, int H, int ug, const float* const* wih_p_host,
                            const float* const* whh_p_host, const float* const* bias_p_host, void* ws, size_t ws_bytes, int flags,
                            void* stream, const Pipe2Map& map = Pipe2Map()) {
  LstmGeo g;
  Pipe2Ws o;
  if (!lstm_geo(H, ug, &g)) return ONSSEN_E_ARG;
  if (!x || !ws || !wih_p_host || !whh_p_host || !bias_p_host || B <= 0 || B > 32 || T <= 0 || in_dim <= 0) return ONSSEN_E_ARG;
  if (T > T_cap || T_prev <= 0 || T_prev > T_cap) return ONSSEN_E_ARG;
  // ragged rows keep the bits of their own batch-1 run: stacked tiles only, i.e. <= 16 rows; both batches bring their frames
  if ((frames != nullptr) != (frames_prev != nullptr) || (frames && B > 16)) return ONSSEN_E_ARG;
  // the plain split-bf16 persistent recurrence only (no fused first layer, no bf16-only products)
  if ((flags & 0xff & ~ONSSEN_BLSTM_G_READY) != (ONSSEN_BLSTM_BF16X3 | ONSSEN_BLSTM_XCD)) return ONSSEN_E_ARG;
  const bool g_ready = (flags & ONSSEN_BLSTM_G_READY) != 0;     // measurement aid: the pair launch by itself, on the projections an earlier call left
  if (!pipe2_ws_layout(B, T_cap, in_dim, g, &o)) return ONSSEN_E_ARG;
  if (ws_bytes < o.total) return ONSSEN_E_WORKSPACE;
  if (!aligned256(ws)) return ONSSEN_E_ALIGN;
  if (ug > 20 || g.NU > 32 || g.KQ2 > 24) return ONSSEN_E_ARG;
  // the map's workspace: what onssen_dc_index_f32 asks of it; its features are x itself, so x is the dense [B][T][in_dim] array
  const DcWs ml(B, T, in_dim, map.D);
  if (map.ws) {
    if (frames || map.D <= 0 || map.D > km::DMAX || xs_t != in_dim || xs_b != (int64_t)T * in_dim) return ONSSEN_E_ARG;
    if (map.ws_bytes < ml.compact_bytes) return ONSSEN_E_WORKSPACE;
    if (!aligned256(map.ws)) return ONSSEN_E_ALIGN;
  }
  char* base = (char*)ws;
  float *G0 = (float*)(base + o.g0), *G1 = (float*)(base + o.g1);
  uint16_t *img_x = (uint16_t*)(base + o.img_x), *img0 = (uint16_t*)(base + o.img0), *img1 = (uint16_t*)(base + o.img1);
  const int NP = g.NP;
  // layer 0 of THIS batch: input image, input projection
  int rc = ONSSEN_OK;
  if (!g_ready) {
    rc = onssen_x3_image_f32(x, xs_t, xs_b, B, T * B, in_dim, img_x, stream);
    if (rc != ONSSEN_OK) return rc;
    rc = onssen_linear_x3p(img_x, T * B, in_dim, (const uint16_t*)wih_p_host[0], bias_p_host[0], 2 * NP, ONSSEN_EPI_BIAS, 0, 0.f, G0, B,
                           (int64_t)B * 2 * NP, 2 * NP, stream);
    if (rc != ONSSEN_OK) return rc;
  }
  // ONE launch: layer 1 of the batch before (its G1 was left by the call before) beside layer 0 of this one
  XcdArgs xa = xcd_args(g, ws, o.hs, B, flags);
  xa.G = G1; xa.whh = (const unsigned short*)whh_p_host[1]; xa.yimg = img1; xa.T = T_prev; xa.frames = frames_prev;
  xa.G_b = G0; xa.whh_b = (const unsigned short*)whh_p_host[0]; xa.yimg_b = img0; xa.T_b = T; xa.frames_b = frames;
  xa.ximg = img_x; xa.bias0 = bias_p_host[0]; xa.x0 = x; xa.xs_b = (long)xs_b; xa.xs_t = (long)xs_t;
  xa.terms = 3;
  if (map.ws) {
    xa.aux_n = B < 16 ? B : 16;      // two CUs per XCD are no member's
    xa.aux_D = map.D; xa.aux_db = map.db; xa.aux_feat = x; xa.aux_per_utt = (long)T * in_dim; xa.aux_stride = ml.stride;
    xa.aux_w = (float*)map.ws; xa.aux_iw = ml.at<int>(map.ws, ml.iw); xa.aux_dest = ml.at<int>(map.ws, ml.dest);
  }
  ONSSEN_CLEAR_ERROR();
  rc = dispatch_ug<20>(ug, [&](auto ugc) { return launch_xcd_pair<decltype(ugc)::value / 4>(xa, (hipStream_t)stream); });
  if (rc != ONSSEN_OK || g_ready) return rc;
  // layer 1's input projection of THIS batch, for the next call
  return onssen_linear_x3p(img0, T * B, 2 * g.Hp, (const uint16_t*)wih_p_host[1], bias_p_host[1], 2 * NP, ONSSEN_EPI_BIAS, 0, 0.f, G1, B,
                           (int64_t)B * 2 * NP, 2 * NP, stream);
}

int onssen_blstm_pipe2_forward_f32(const float* x, int64_t xs_b, int64_t xs_t, int B, int T, int in_dim, int H, int ug,
                                   const float* const* wih_p_host, const float* const* whh_p_host,
                                   const float* const* bias_p_host, void* ws, size_t ws_bytes, int flags, void* stream) {
  return blstm_pipe2_impl(x, xs_b, xs_t, B, T, T, nullptr, T, nullptr, in_dim, H, ug, wih_p_host, whh_p_host, bias_p_host, ws, ws_bytes,
                          flags, stream);
}

int onssen_blstm_pipe2_map_forward_f32(const float* x, int64_t xs_b, int64_t xs_t, int B, int T, int in_dim, int H, int ug,
                                       const float* const* wih_p_host, const float* const* whh_p_host,
                                       const float* const* bias_p_host, void* ws, size_t ws_bytes, int flags, float db_threshold, int D,
                                       void* map_ws, size_t map_ws_bytes, void* stream) {
  if (!map_ws) return ONSSEN_E_ARG;
  Pipe2Map map;
  map.db = db_threshold; map.D = D; map.ws = map_ws; map.ws_bytes = map_ws_bytes;
  return blstm_pipe2_impl(x, xs_b, xs_t, B, T, T, nullptr, T, nullptr, in_dim, H, ug, wih_p_host, whh_p_host, bias_p_host, ws, ws_bytes,
                          flags, stream, map);
}

int onssen_blstm_pipe2_forward_ragged_f32(const float* x, int64_t xs_b, int64_t xs_t, int B, int T_cap, int T, const int32_t* frames,
                                          int T_prev, const int32_t* frames_prev, int in_dim, int H, int ug,
                                          const float* const* wih_p_host, const float* const* whh_p_host,
                                          const float* const* bias_p_host, void* ws, size_t ws_bytes, int flags, void* stream) {
  if (!frames || !frames_prev) return ONSSEN_E_ARG;
  return blstm_pipe2_impl(x, xs_b, xs_t, B, T_cap, T, frames, T_prev, frames_prev, in_dim, H, ug, wih_p_host, whh_p_host, bias_p_host, ws,
                          ws_bytes, flags, stream);
}

// ---- training: the backward recurrence ------------------------------------------------------------------------------------
// launch-per-step form: hand-off images [2 slots][2 dirs][ceil(B/16)][KQB][2 KiB], then the carried dL/dc [2][B][Hp]
static size_t bwd_step_image_bytes(int B, const LstmGeo& g) { return align256((size_t)2 * 2 * ceil_div(B, 16) * g.KQB * 2048); }
// persistent form: header, then the exchange blocks [8 groups][2 slots][NU dst][NU src][ug][RG] (debug builds: timestamps behind them)
static size_t bwd_workspace_bytes(int B, const LstmGeo& g, int form) {
  if (form == ONSSEN_LSTM_BWD_XCD)
    return ONSSEN_BLSTM_WS_HEADER_BYTES + align256((size_t)8 * 2 * g.NU * g.NU * xcd_rows_per_group(B, false) * g.ug * sizeof(float));
  return bwd_step_image_bytes(B, g) + align256((size_t)2 * B * g.Hp * sizeof(float));
}
size_t onssen_lstm_train_backward_workspace_bytes(int B, int H, int ug, int form) {
  LstmGeo g;
  return B > 0 && lstm_geo(H, ug, &g) ? bwd_workspace_bytes(B, g, form) : 0;
}

static int lstm_train_backward_impl(int B, int T, int H, int ug, const uint16_t* whh_img, const float* dy, float* gates_dp,
                                    const float* cs, void* ws, size_t ws_bytes, int form, float* db_rows, uint16_t* dp_img, void* stream) {
  LstmGeo g;
  if (!whh_img || !dy || !gates_dp || !cs || !ws || B <= 0 || T <= 0 || !lstm_geo(H, ug, &g) ||
      (form != ONSSEN_LSTM_BWD_STEPS && form != ONSSEN_LSTM_BWD_XCD) || (db_rows && form != ONSSEN_LSTM_BWD_XCD) ||
      (db_rows && !aligned16(db_rows)))
    return ONSSEN_E_ARG;
  const size_t need = bwd_workspace_bytes(B, g, form);
  if (ws_bytes < need) return ONSSEN_E_WORKSPACE;
  if (!aligned256(ws) || !aligned16(gates_dp)) return ONSSEN_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  if (form == ONSSEN_LSTM_BWD_XCD) {
    if (g.NU > 32 || g.NUB > 40) return ONSSEN_E_ARG;
    static const int ablate_env = ONSSEN_KNOB_INT("ONSSEN_BWD_ABLATE", 0);
    static const int delay_env = ONSSEN_KNOB_INT("ONSSEN_BWD_DELAY", 0);
    static const bool bwd_unstacked = ONSSEN_KNOB_INT("ONSSEN_BWD_UNSTACKED", 0) != 0;      // debug builds: the three-term form of rounds 2-4, for A/B
    static const bool bwd_wide = ONSSEN_KNOB_INT("ONSSEN_BWD_WIDE", ONSSEN_BWD_WIDE) != 0;      // the wide poll of round 6 (lstm_bwd.inc: RGW)
    // ONSSEN_XCD_PROFILE builds only (ONSSEN_BWD_DBG=1, tools/bwd_timeline.py): 8 timestamps per step of workgroup 0 in the tail of ws
    static const bool dbg_env = ONSSEN_KNOB_INT("ONSSEN_BWD_DBG", 0) != 0;
    XcdBwdArgs xa;
    xa.gd = gates_dp; xa.cs = cs; xa.dy = dy; xa.wR = whh_img; xa.sync = (unsigned*)ws;
    xa.xch = (float*)((char*)ws + ONSSEN_BLSTM_WS_HEADER_BYTES);
    xa.B = B; xa.T = T; xa.Hp = g.Hp; xa.NP = g.NP; xa.NU = g.NU; xa.NTB = g.NUB; xa.RG = xcd_rows_per_group(B, false);
    xa.spin_limit = xcd_spin_limit(); xa.ablate = ablate_env; xa.delay = delay_env; xa.db_rows = db_rows; xa.dp_img = dp_img;
    xa.dbg = dbg_env && ws_bytes >= need + (size_t)T * 64 ? (long long*)((char*)ws + need) : nullptr;
    ONSSEN_CLEAR_ERROR();
    const dim3 grid((unsigned)(8 * xa.NU));
    const int E = xa.RG * ug, parts = 4 * E <= 320 ? 4 : 2 * E <= 320 ? 2 : 1;   // polling lanes per element (320 polling threads)
    dispatch_ug<20>(ug, [&](auto ugc) {
      constexpr int UG = decltype(ugc)::value;
#define ONSSEN_BWD_LAUNCH(...) hipLaunchKernelGGL((lstm_xcd_bwd_kernel<UG, __VA_ARGS__>), grid, dim3(512), 0, st, xa)
      for (int r0 = 0; r0 < B; r0 += 4 * xa.RG) {
        const int rows = B - r0 < 4 * xa.RG ? B - r0 : 4 * xa.RG;
        xa.row0 = r0;
        xa.nbg = ceil_div(rows, xa.RG);
        if (bwd_wide && !bwd_unstacked) {   // round 6: the wide poll (16-byte loads, 16 lanes per unit)
          if (xa.RG == 4) ONSSEN_BWD_LAUNCH(1, true, 4);
          else if (xa.RG == 8) ONSSEN_BWD_LAUNCH(1, true, 8);
          else ONSSEN_BWD_LAUNCH(1, false, 16);
        } else if (xa.RG <= 8 && !bwd_unstacked) {
          if (parts == 4) ONSSEN_BWD_LAUNCH(4, true);
          else if (parts == 2) ONSSEN_BWD_LAUNCH(2, true);
          else ONSSEN_BWD_LAUNCH(1, true);
        } else if (parts == 4) ONSSEN_BWD_LAUNCH(4, false);
        else if (parts == 2) ONSSEN_BWD_LAUNCH(2, false);
        else ONSSEN_BWD_LAUNCH(1, false);
      }
#undef ONSSEN_BWD_LAUNCH
      return ONSSEN_OK;
    });
    ONSSEN_LAUNCH_CHECK();
    return ONSSEN_OK;
  }
  const size_t img_bytes = bwd_step_image_bytes(B, g);
  hipError_t e = hipMemsetAsync(ws, 0, img_bytes, st);   // rows past B and the K tail of the images stay zero
  if (e != hipSuccess) return (int)e;
  BwdArgs p;
  p.gd = gates_dp; p.cs = cs; p.dy = dy; p.wT = whh_img; p.ds = (unsigned short*)ws; p.dc = (float*)((char*)ws + img_bytes);
  p.B = B; p.T = T; p.Hp = g.Hp; p.NP = g.NP; p.UG = ug; p.KQB = g.KQB; p.NUB = g.NUB;
  ONSSEN_CLEAR_ERROR();
  const dim3 grid((unsigned)g.NUB, 2, (unsigned)ceil_div(B, 16));
  for (int s = 0; s < T; ++s) {
    p.step = s;
    hipLaunchKernelGGL(lstm_bwd_step_kernel, grid, dim3(64 * recb::NW), 0, st, p);
  }
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

int onssen_lstm_train_backward_f32(int B, int T, int H, int ug, const uint16_t* whh_img, const float* dy, float* gates_dp,
                                   const float* cs, void* ws, size_t ws_bytes, int form, float* db_rows, void* stream) {
  return lstm_train_backward_impl(B, T, H, ug, whh_img, dy, gates_dp, cs, ws, ws_bytes, form, db_rows, nullptr, stream);
}

int onssen_lstm_train_backward_img_f32(int B, int T, int H, int ug, const uint16_t* whh_img, const float* dy, const float* gates,
                                       const float* cs, void* ws, size_t ws_bytes, float* db_rows, uint16_t* dp_img, void* stream) {
  LstmGeo g;
  if (!dp_img || !aligned16(dp_img) || !lstm_geo(H, ug, &g) || (2 * g.NP) % 32 != 0) return ONSSEN_E_ARG;
  return lstm_train_backward_impl(B, T, H, ug, whh_img, dy, const_cast<float*>(gates), cs, ws, ws_bytes, ONSSEN_LSTM_BWD_XCD, db_rows,
                                  dp_img, stream);
}
