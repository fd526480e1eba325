// Conv-TasNet streaming inference: n causal streams that advance in lockstep, F hops (F L/2 samples) in and out per step.
//
// With causal = 1 and norm in {cLN, BN} every stage of the forward is local to one encoder frame, except three that reach back:
// the encoder frame (one hop of samples), each block's dilated depthwise convolution ((P - 1) 2^x frames) and the decoder's
// overlap-add (one frame).  A step therefore is tas::run (tasnet_run.inc) over a STREAM Plan: the forward's own launch sequence
// and row kernels over the M = n F new frames (row = b F + t) -- tas_encoder_kernel on a staging row of carried hop ++ new
// samples, the GEMM helper, tas_prelu_stats_kernel, tas_residual_kernel, tas_mask_kernel, all indifferent to where a row sits --
// with the state pointers (cnt, carry_x, carry_d, the first block's history) in the plan and, at the boundary steps, the four
// kernels of this file, which also keeps the state and workspace layouts, reset and flush:
//   tas_stream_stage_kernel    staging rows [carried hop | new samples], the new carry, and the frame counters' advance
//   tas_stream_dwconv_kernel   the depthwise convolution whose taps before the chunk come from the block's history ring
//   tas_stream_history_kernel  the chunk's last min(F, history) rows (and their cLN statistics) into the ring
//   tas_stream_decoder_kernel  contraction over N as tas_decoder_tile, bias + frame j first half + frame j - 1 second half; the
//                              second half of the chunk's last frame is carried
// plus tas_stream_reset_kernel and tas_stream_flush_kernel.  The arithmetic of one output element is the offline kernels'
// expression in the offline order, so concat(steps)[hop:] ++ flush is bit for bit onssen_tasnet_forward_f32 of the whole signal.
//
// Frame counters: cnt[b] (int64, device) = index of the next frame of stream b, -1 after a reset (the first hop completes no
// frame: "frame -1" is computed like any row, from a zero carry, but nothing reads it -- every tap and every overlap-add term
// whose frame index is negative is SKIPPED, as the offline kernels skip them; it is not a zero row pushed through the norm).
// The stage kernel advances cnt by F at the start of the step; the later kernels of the step see first = cnt[b] - F.  No host
// value changes from step to step, so one captured graph of a step serves every later step of the same (n, F).
//
// Hazard rule: no launch writes a state row that another workgroup of the same launch reads.  The history is a ring keyed by the
// frame index (frame g lives in slot (g + 1) mod history), read by the depthwise launch and written only by the history launch
// after it, which reads nothing but the chunk; the ring's F oldest rows are the ones replaced, so F <, = and > history are
// one code path.  The input carry is read and rewritten by the same thread; the decoder carry of (speaker, stream) is read and
// rewritten by that pair's first workgroup alone, on the two sides of its barrier.
// No atomics, no spinning, no allocation: ordinary launches on one stream.

namespace tas {

struct StreamState {
  size_t cnt, carry_x, carry_d, blk0;     // byte offsets: int64 [n], float [n][hop], float [spk][n][hop], first block's history
  size_t total;                           // 0: the size does not fit
};

static inline int stream_history(const Cfg& g, int j) { return (g.P - 1) << (j % g.X); }

static bool stream_cfg(const int32_t* c, Cfg* g) {
  if (!read_cfg(c, g) || !g->causal || g->norm == ONSSEN_TASNET_GLN) return false;
  return ((long)(g->P - 1) << (g->X - 1)) <= ONSSEN_TASNET_STREAM_MAX_HISTORY;      // the deepest block's history, in frames
}

// Per block: the ring [n][history][H] followed by its statistics [n][history][2] (written for cLN only).
static size_t stream_block_bytes(const Cfg& g, int n, int j, size_t* stat_off) {
  const size_t hs = (size_t)stream_history(g, j);
  size_t ring, stat;
  if (__builtin_mul_overflow((size_t)n * hs, (size_t)g.H * 4, &ring) || ring > ((size_t)1 << 60)) return (size_t)-1;
  stat = (size_t)n * hs * 8;
  if (stat_off) *stat_off = al(ring);
  return al(ring) + al(stat);
}

static StreamState stream_state(const Cfg& g, int n) {
  StreamState o{};
  const size_t hop = g.L / 2;
  size_t p = 0;
  o.cnt = p; p += al((size_t)n * 8);
  o.carry_x = p; p += al((size_t)n * hop * 4);
  o.carry_d = p; p += al((size_t)g.spk * n * hop * 4);
  o.blk0 = p;
  for (int j = 0; j < g.R * g.X; ++j) {
    const size_t b = stream_block_bytes(g, n, j, nullptr);
    if (b == (size_t)-1 || __builtin_add_overflow(p, b, &p) || p > ((size_t)1 << 60)) return o;
  }
  o.total = p;
  return o;
}

// ---- reset: everything of the chosen slots to zero, their counters to -1 ------------------------------------------------------
// grid (blocks over a slot's floats, slots); slot = sl.v[blockIdx.y], or blockIdx.y when every slot is reset.  One launch per
// region: a slot's part of a region is per_slot_floats contiguous floats at `off` (is_cnt: the slot's counter instead).
struct StreamSlots { int v[ONSSEN_TASNET_STREAM_RESET_MAX]; };

__global__ __launch_bounds__(256) void tas_stream_reset_kernel(char* __restrict__ state, StreamSlots sl, int use_slots, size_t off,
                                                               long per_slot_floats, int is_cnt) {
  const int b = use_slots ? sl.v[blockIdx.y] : (int)blockIdx.y;
  if (is_cnt) {
    if (blockIdx.x == 0 && threadIdx.x == 0) reinterpret_cast<long long*>(state + off)[b] = -1;
    return;
  }
  float* p = reinterpret_cast<float*>(state + off) + (long)b * per_slot_floats;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < per_slot_floats; e += (long)gridDim.x * blockDim.x) p[e] = 0.0f;
}

// ---- stage: [carried hop | F hop new samples] per stream, the new carry, cnt += F ---------------------------------------------
__global__ __launch_bounds__(256) void tas_stream_stage_kernel(const float* __restrict__ x, long x_s, int n, int F, int hop,
                                                               float* __restrict__ carry, long long* __restrict__ cnt,
                                                               float* __restrict__ stage) {
  const long row = (long)(F + 1) * hop, total = (long)n * row;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const long b = e / row;
    const int i = (int)(e % row);
    float v;
    if (i < hop) {                                    // this thread alone reads and then rewrites carry[b][i]
      v = carry[b * hop + i];
      carry[b * hop + i] = x[b * x_s + (long)(F - 1) * hop + i];
      if (i == 0) cnt[b] += F;
    } else {
      v = x[b * x_s + (i - hop)];
    }
    stage[e] = v;
  }
}

// ---- norm_1 on load + dilated causal depthwise convolution over [history | chunk] ----------------------------------------------
// grid (tiles of 32 frames, streams); threads over channels.  Chunk frame t is frame first + t of the stream; tap p reads frame
// first + t - dil (P - 1 - p): skipped when negative, from the chunk when t - dil (P - 1 - p) >= 0, from the ring otherwise.
__global__ __launch_bounds__(256) void tas_stream_dwconv_kernel(const float* __restrict__ c, int F, int H, int P, int dil, int norm,
                                                                const float* __restrict__ rstat, const float* __restrict__ hist,
                                                                const float* __restrict__ hstat, const long long* __restrict__ cnt,
                                                                const float* __restrict__ na, const float* __restrict__ nb,
                                                                const float* __restrict__ dw, const float* __restrict__ dwb,
                                                                float* __restrict__ out) {
  const int b = blockIdx.y, hs = dil * (P - 1);
  const long long first = cnt[b] - F;
  int slot0 = hs > 0 ? (int)((first + 1) % hs) : 0;            // slot of chunk frame 0 (first + 1 >= 0); P = 1 has no history
  if (slot0 < 0) slot0 += hs;                                  // a state that was never reset: still inside the ring
  const long base = (long)b * F, hbase = (long)b * hs;
  const int t0 = blockIdx.x * DW_ROWS, t1 = t0 + DW_ROWS < F ? t0 + DW_ROWS : F;
  for (int k = threadIdx.x; k < H; k += blockDim.x) {
    const float ga = na[k], gb = nb[k], bias = dwb[k];
    for (int t = t0; t < t1; ++t) {
      float acc = bias;
      for (int p = 0; p < P; ++p) {
        const int li = t + dil * p - hs;
        if (first + li < 0) continue;
        float v, mean = 0.0f, rstd = 1.0f;
        if (li >= 0) {
          v = c[(base + li) * H + k];
          if (norm == ONSSEN_TASNET_CLN) { mean = rstat[(base + li) * 2]; rstd = rstat[(base + li) * 2 + 1]; }
        } else {
          int s = (slot0 + li) % hs;                  // slot0 + li in (-hs, hs)
          if (s < 0) s += hs;
          v = hist[(hbase + s) * H + k];
          if (norm == ONSSEN_TASNET_CLN) { mean = hstat[(hbase + s) * 2]; rstd = hstat[(hbase + s) * 2 + 1]; }
        }
        acc += dw[k * P + p] * norm_tap(v, mean, rstd, ga, gb, norm == ONSSEN_TASNET_CLN ? norm : ONSSEN_TASNET_BN);   // a stream has no gLN
      }
      out[(base + t) * H + k] = acc;
    }
  }
}

// ---- the chunk's last min(F, history) rows into the ring (reads the chunk only) ------------------------------------------------
// grid (rows, streams)
__global__ __launch_bounds__(256) void tas_stream_history_kernel(const float* __restrict__ c, int F, int H, int hs, int norm,
                                                                 const float* __restrict__ rstat, const long long* __restrict__ cnt,
                                                                 float* __restrict__ hist, float* __restrict__ hstat) {
  const int b = blockIdx.y, keep = F < hs ? F : hs, t = F - keep + (int)blockIdx.x;
  const long long first = cnt[b] - F;
  int s = (int)((first + 1 + t) % hs);
  if (s < 0) s += hs;                                          // a state that was never reset: still inside the ring
  const float* src = c + ((long)b * F + t) * H;
  float* dst = hist + ((long)b * hs + s) * H;
  for (int k = threadIdx.x; k < H; k += blockDim.x) dst[k] = src[k];
  if (norm == ONSSEN_TASNET_CLN && threadIdx.x < 2) hstat[((long)b * hs + s) * 2 + threadIdx.x] = rstat[((long)b * F + t) * 2 + threadIdx.x];
}

// ---- decoder: F hop-sized output blocks per (speaker, stream) -------------------------------------------------------------------
// grid (tiles of 16 blocks, streams, speakers).  Block t of the chunk is block first + t of the stream: zeros when negative, else
// bias + frame (first + t) taps [0, hop) + frame (first + t - 1) taps [hop, L) when first + t >= 1.  The frame before the chunk
// is the carry; tile 0 of each (speaker, stream) also contracts the second half of the chunk's last frame and, past the barrier
// behind which it has read the old carry, stores it as the new one.
__global__ __launch_bounds__(256) void tas_stream_decoder_kernel(const float* __restrict__ d, int F, int N, int L, int spk,
                                                                 const float* __restrict__ dw, const float* __restrict__ db,
                                                                 const long long* __restrict__ cnt, float* __restrict__ carry,
                                                                 float* __restrict__ out) {
  __shared__ float Ps[(DEC_FRAMES + 1) * MAX_L];
  __shared__ float tail[MAX_L / 2];
  const int b = blockIdx.y, s = blockIdx.z, n = gridDim.y, hop = L / 2, j0 = blockIdx.x * DEC_FRAMES;
  const long long first = cnt[b] - F;
  const long ldd = (long)spk * N, base = (long)b * F;
  float* cr = carry + ((long)s * n + b) * hop;
  for (int e = threadIdx.x; e < (DEC_FRAMES + 1) * L; e += blockDim.x) {
    const int jj = e / L, l = e % L, f = j0 - 1 + jj;
    float acc = 0.0f;
    if (f >= 0 && f < F) {
      acc = dec_tap(d + (base + f) * ldd + (long)s * N, dw, N, L, l);
    } else if (f < 0 && l >= hop) {
      acc = cr[l - hop];
    }
    Ps[jj * L + l] = acc;
  }
  if (j0 == 0)
    for (int e = threadIdx.x; e < hop; e += blockDim.x) tail[e] = dec_tap(d + (base + F - 1) * ldd + (long)s * N, dw, N, L, hop + e);
  __syncthreads();
  if (j0 == 0)
    for (int e = threadIdx.x; e < hop; e += blockDim.x) cr[e] = tail[e];
  const float bias = db[0];
  float* o = out + ((long)s * n + b) * ((long)F * hop);
  const int i0 = j0 * hop, i1 = (j0 + DEC_FRAMES) * hop < F * hop ? (j0 + DEC_FRAMES) * hop : F * hop;
  for (int i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
    const int j = i / hop, off = i - j * hop, jj = j - (j0 - 1);
    float v = 0.0f;
    if (first + j >= 0) {
      v = bias;
      v += Ps[jj * L + off];                                       // frame j, tap off
      if (first + j >= 1) v += Ps[(jj - 1) * L + off + hop];       // frame j - 1, tap off + hop
    }
    o[i] = v;
  }
}

// ---- flush: the block after the last frame, bias + the carried second half (zeros while the stream has no frame) ----------------
__global__ __launch_bounds__(256) void tas_stream_flush_kernel(const float* __restrict__ carry, const long long* __restrict__ cnt,
                                                               const float* __restrict__ db, int n, int hop, int spk,
                                                               float* __restrict__ out) {
  const long total = (long)spk * n * hop;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int b = (int)((e / hop) % n);
    float v = 0.0f;
    if (cnt[b] >= 1) {
      v = db[0];
      v += carry[e];
    }
    out[e] = v;
  }
}

struct StreamWs { size_t stage, fwd, total; Ws w; };

static StreamWs stream_ws(const Cfg& g, int n, int F) {
  StreamWs o;
  o.w = ws_layout_rows(g, (size_t)n * F, (size_t)n * ceil_div(F, ROWS_PER_CHUNK));
  o.stage = 0;
  o.fwd = al((size_t)n * ((size_t)F + 1) * (g.L / 2) * 4);
  o.total = o.fwd + o.w.total;
  return o;
}

// n is a grid dimension (y) of the per-stream kernels; M = n F rows obey the forward's bound
static bool stream_rows_ok(int n, int F) { return n >= 1 && n <= 65535 && F >= 1 && (long)n * F <= 0x7fffffffL / 4; }

}  // namespace tas

extern "C" {

size_t onssen_tasnet_stream_state_bytes(const int32_t* cfg_host, int n) {
  tas::Cfg g;
  if (!tas::stream_cfg(cfg_host, &g) || n < 1 || n > 65535) return 0;
  return tas::stream_state(g, n).total;
}

int onssen_tasnet_stream_reset(const int32_t* cfg_host, void* state, size_t state_bytes, int n, const int32_t* slots_host,
                               int n_slots, void* stream) {
  tas::Cfg g;
  if (!tas::stream_cfg(cfg_host, &g) || !state || n < 1 || n > 65535 || n_slots < 0 || (n_slots > 0 && !slots_host)) return ONSSEN_E_ARG;
  for (int i = 0; i < n_slots; ++i)
    if (slots_host[i] < 0 || slots_host[i] >= n) return ONSSEN_E_ARG;
  const tas::StreamState o = tas::stream_state(g, n);
  if (o.total == 0) return ONSSEN_E_ARG;
  if (state_bytes < o.total) return ONSSEN_E_WORKSPACE;
  if (!aligned256(state)) return ONSSEN_E_ALIGN;
  ONSSEN_CLEAR_ERROR();
  hipStream_t st = (hipStream_t)stream;
  char* sb = static_cast<char*>(state);
  const int hop = g.L / 2;
  // the slot list travels by value, ONSSEN_TASNET_STREAM_RESET_MAX slots per round of launches
  for (int at = 0; at < (n_slots ? n_slots : 1); at += ONSSEN_TASNET_STREAM_RESET_MAX) {
    tas::StreamSlots sl{};
    const int use = n_slots > 0;
    int m = n;
    if (use) {
      m = n_slots - at < ONSSEN_TASNET_STREAM_RESET_MAX ? n_slots - at : ONSSEN_TASNET_STREAM_RESET_MAX;
      for (int i = 0; i < m; ++i) sl.v[i] = slots_host[at + i];
    }
    auto zero = [&](size_t off, long per_slot) {
      const long nb = (per_slot + 255) / 256;
      hipLaunchKernelGGL(tas::tas_stream_reset_kernel, dim3((unsigned)(nb > 1024 ? 1024 : nb), (unsigned)m), dim3(256), 0, st, sb, sl,
                         use, off, per_slot, 0);
    };
    hipLaunchKernelGGL(tas::tas_stream_reset_kernel, dim3(1, (unsigned)m), dim3(256), 0, st, sb, sl, use, o.cnt, 0L, 1);
    zero(o.carry_x, hop);
    for (int s = 0; s < g.spk; ++s) zero(o.carry_d + (size_t)s * n * hop * 4, hop);
    size_t p = o.blk0;
    for (int j = 0; j < g.R * g.X; ++j) {
      const long hs = tas::stream_history(g, j);
      size_t stat_off;
      const size_t bytes = tas::stream_block_bytes(g, n, j, &stat_off);
      if (hs > 0) {
        zero(p, hs * g.H);
        zero(p + stat_off, hs * 2);
      }
      p += bytes;
    }
    if (!use) break;
  }
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

size_t onssen_tasnet_stream_workspace_bytes(const int32_t* cfg_host, int n, int frames) {
  tas::Cfg g;
  if (!tas::stream_cfg(cfg_host, &g) || !tas::stream_rows_ok(n, frames)) return 0;
  return tas::stream_ws(g, n, frames).total;
}

int onssen_tasnet_stream_step_f32(const int32_t* cfg_host, const void* image, const float* x_new, int n, int frames,
                                  int64_t x_stride, float* out, void* state, size_t state_bytes, void* ws, size_t ws_bytes,
                                  void* stream) {
  tas::Cfg g;
  if (!tas::stream_cfg(cfg_host, &g) || !image || !x_new || !out || !state || !ws || !tas::stream_rows_ok(n, frames)) return ONSSEN_E_ARG;
  const int hop = g.L / 2, F = frames;
  if (x_stride < (int64_t)F * hop) return ONSSEN_E_ARG;
  const tas::StreamState so = tas::stream_state(g, n);
  if (so.total == 0) return ONSSEN_E_ARG;
  const tas::StreamWs wo = tas::stream_ws(g, n, F);
  if (state_bytes < so.total || ws_bytes < wo.total) return ONSSEN_E_WORKSPACE;
  if (!aligned256(image) || !aligned256(ws) || !aligned256(state)) return ONSSEN_E_ALIGN;
  char *sb = static_cast<char*>(state), *wb = static_cast<char*>(ws);
  tas::Plan p = tas::in_place(tas::STREAM, n, F, (long)n * F, x_new, (long)x_stride, out, wb + wo.fwd, wo.w);
  p.cnt = reinterpret_cast<long long*>(sb + so.cnt);
  p.carry_x = reinterpret_cast<float*>(sb + so.carry_x); p.carry_d = reinterpret_cast<float*>(sb + so.carry_d);
  p.hist = sb + so.blk0; p.stage = reinterpret_cast<float*>(wb + wo.stage);
  return tas::run(g, image, p, stream);
}

int onssen_tasnet_stream_flush_f32(const int32_t* cfg_host, const void* image, const void* state, size_t state_bytes, int n,
                                   float* out_tail, void* stream) {
  tas::Cfg g;
  if (!tas::stream_cfg(cfg_host, &g) || !image || !state || !out_tail || n < 1 || n > 65535) return ONSSEN_E_ARG;
  const tas::StreamState so = tas::stream_state(g, n);
  if (so.total == 0) return ONSSEN_E_ARG;
  if (state_bytes < so.total) return ONSSEN_E_WORKSPACE;
  if (!aligned256(image) || !aligned256(state)) return ONSSEN_E_ALIGN;
  ONSSEN_CLEAR_ERROR();
  const tas::Layout o = tas::layout(g);
  const char* sb = static_cast<const char*>(state);
  const int hop = g.L / 2;
  hipLaunchKernelGGL(tas::tas_stream_flush_kernel, dim3(tas::ew_grid((long)g.spk * n * hop)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const float*>(sb + so.carry_d), reinterpret_cast<const long long*>(sb + so.cnt),
                     reinterpret_cast<const float*>(static_cast<const char*>(image) + o.dec_b), n, hop, g.spk, out_tail);
  ONSSEN_LAUNCH_CHECK();
  return ONSSEN_OK;
}

}  // extern "C"
