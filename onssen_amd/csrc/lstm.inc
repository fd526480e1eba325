// K4 BLSTM recurrence: launch-per-step kernel, XCD-local persistent kernel (part of onssen_hip.hip; their launchers: lstm_run.inc).
// =================================================================================================
// K4: one LSTM time step, both directions
// =================================================================================================
struct StepArgs {
  const float* G = nullptr;                // [T][B][2][NP]   input projection + biases, gate-permuted columns
  const float* whh = nullptr;              // [2][NU][KQ][NT][64][4]
  float* y = nullptr;                      // [T][B][2][Hp]   layer output (h_t)
  float* c = nullptr;                      // [2][B][Hp]      cell state
  const unsigned short* whh_x3 = nullptr;  // split-bf16 image [2][NU][KQ2][NT][2][64][8]          (X3 kernels)
  unsigned short* hs = nullptr;            // split h hand-off in A-fragment order:
                                           //   [2 slots][2 dirs][ceil(B/16)][KQ2][hi|lo][64 lanes][8] bf16   (X3 kernels)
  int KQ2 = 0, Hs = 0;                     // 32-wide k-chunks, padded row length Hs = 32*KQ2
  int B = 0, T = 0, Hp = 0, NP = 0, KQ = 0, NU = 0, step = 0;
  long long* dbg = nullptr;                // profiling only: per-step timestamps of workgroup (0,0,0), or null
  int ablate = 0;                          // profiling only (flags >> 8): 1 = no h loads, 2 = no W loads, 4 = no MFMA, 8 = no G / c loads
  const int* frames = nullptr;             // ragged batch: frames of every batch row (<= T), or null
  float* save_g = nullptr;                 // training forward: [T][B][2][NP] gate activations (i, f, g, o) in G's column layout, or null
  float* save_c = nullptr;                 // training forward: [T][B][2][Hp] cell states
};

namespace rec {
constexpr int RLD = 72;  // LDS row stride of the per-wave partial accumulators (64 lanes + pad)
constexpr int QB = 10;   // k-chunks (16 k each) a wave keeps in flight: 4 waves x 10 x 16 = 640 >= H
constexpr int QB3 = 5;   // same for the split-bf16 form (32 k per chunk)
}

// Gate non-linearities on the hardware transcendental units: sigmoid(x) = rcp(1 + exp2(-x log2 e)),
// tanh(x) = 2 sigmoid(2x) - 1.  v_exp_f32 / v_rcp_f32 are ~1 ulp, so the absolute error is ~1e-7 --
// far inside the 1e-5 parity budget -- while libm-grade expf/tanhf/IEEE divides made this epilogue
// (one wave per SIMD, nothing to hide latency behind) a measurable slice of every time step.
__device__ __forceinline__ float gate_sigmoid(float x) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x));
}
__device__ __forceinline__ float gate_tanh(float x) { return 2.0f * gate_sigmoid(2.0f * x) - 1.0f; }

// Arguments are 14 scalar dwords in order of first use so that, with -amdgpu-kernarg-preload-count, the
// command processor delivers them in SGPRs at dispatch.  Every launch starts with cold scalar/L2 caches, so
// each *dependent* s_load of a kernel argument is a ~1 us round trip to memory on the critical path of a
// time step; the struct-by-value form paid three of them.  Everything else is derived from these.
template <int MT, int NT, bool X3, bool DBG>
__global__ __launch_bounds__(256) void lstm_step_kernel(const void* w, char* ws, float* y, int step, int B, int NU,
                                                        int T, unsigned g_off256, unsigned c_off256,
                                                        unsigned hs_off256, int ablate_arg, long long* dbg_arg,
                                                        const int* frames_arg, float* save_g_arg, float* save_c_arg) {
  using namespace rec;
  constexpr int UG = 4 * NT;          // hidden units per workgroup
  StepArgs p;
  p.G = reinterpret_cast<const float*>(ws + (size_t)g_off256 * 256);
  p.c = reinterpret_cast<float*>(ws + (size_t)c_off256 * 256);
  p.hs = reinterpret_cast<unsigned short*>(ws + (size_t)hs_off256 * 256);
  p.whh = static_cast<const float*>(w);
  p.whh_x3 = static_cast<const unsigned short*>(w);
  p.y = y; p.step = step; p.B = B; p.NU = NU; p.T = T;
  p.Hp = NU * UG; p.NP = 4 * p.Hp; p.KQ = (p.Hp + 15) / 16; p.KQ2 = (p.Hp + 31) / 32; p.Hs = 32 * p.KQ2;
  p.ablate = DBG ? ablate_arg : 0;
  p.dbg = DBG ? dbg_arg : nullptr;
  // ragged batches (per-row frame counts, onssen_blstm_forward_ragged_f32) run on the DBG instantiations: the argument
  // lies past the preloaded dwords and the plain instantiations never read it
  const int* const frames = DBG ? frames_arg : nullptr;
  // training forward on the launch-per-step form (the re-run of an aborted training step, H > 640): the gate activations
  // (G's layout) and the cell states for the backward kernels -- also on the DBG instantiations only
  float* const save_g = DBG ? save_g_arg : nullptr;
  float* const save_c = DBG ? save_c_arg : nullptr;
  constexpr int NE = 16 * MT * UG;    // (batch row, unit) elements per workgroup
  constexpr int EPT = (NE + 255) / 256;
  __shared__ float red[4 * MT * NT * 4 * RLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ugi = blockIdx.x, dir = blockIdx.y, b0 = blockIdx.z * 16 * MT;
  const int t = dir == 0 ? p.step : p.T - 1 - p.step;
  const int tprev = dir == 0 ? t - 1 : t + 1;
  const bool first = p.step == 0;
  const bool stamp = p.dbg && tid == 0 && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0;
  if (stamp) { p.dbg[p.step * 8 + 0] = wall_clock64(); p.dbg[p.step * 8 + 1] = clock64(); }

  // ---- the epilogue's global reads (input projection, cell state) are independent of the recurrent
  // product: they are issued right after the operand fetches so that their latency hides behind the MFMAs
  float gpre[EPT][4], cold[EPT];
  auto load_epilogue_inputs = [&]() {
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
      const int e = tid + 256 * i;
      const int row = e / UG, ju = e % UG, b = b0 + row;
      const bool ok = (e < NE) && (b < p.B) && !(p.ablate & 8);
      const float4 g4 = ok ? *reinterpret_cast<const float4*>(p.G + ((long)(t * p.B + b) * 2 + dir) * p.NP + ugi * 4 * UG + ju * 4)
                           : make_float4(0.f, 0.f, 0.f, 0.f);
      gpre[i][0] = g4.x; gpre[i][1] = g4.y; gpre[i][2] = g4.z; gpre[i][3] = g4.w;
      cold[i] = (ok && !first) ? p.c[((long)dir * p.B + b) * p.Hp + ugi * UG + ju] : 0.0f;
    }
  };
  if (first) load_epilogue_inputs();

  if (!first) {
    f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int fi = lane & 15, fg = lane >> 4;
    // All operand fetches are raw buffer loads: one SGPR descriptor per operand, ONE per-lane byte offset,
    // compile-time deltas per fragment.  Out-of-range offsets return zeros, so rows past B and chunks past
    // the end of K need neither a branch nor address arithmetic per load -- with a single wave per SIMD the
    // issue cost of ~40 loads was a visible slice of every time step.  (The range check covers the per-lane
    // offset and the immediate, not the scalar offset, so everything goes into the former.)
    constexpr unsigned kOOB = 0x7ffffff0u;
    if constexpr (X3) {
      // split-bf16 form: A = (h_hi, h_lo) written by the previous step's epilogue, B = (W_hi, W_lo)
      const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(p.whh_x3 + (long)(dir * p.NU + ugi) * p.KQ2 * NT * 1024), 0, p.KQ2 * NT * 2048, 0x00020000);
      // the hand-off image is stored in A-fragment order, so each of these loads is one contiguous KiB per wave
      // (a row-major image costs 16 half-used cache lines per load and was the slowest fetch of the step)
      const int nmt = (p.B + 15) >> 4;
      const long hdir = (long)nmt * p.KQ2 * 1024;                     // uint16 elements per (slot, direction)
      const __amdgpu_buffer_rsrc_t rh = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(p.hs + ((long)((p.step - 1) & 1) * 2 + dir) * hdir), 0, (int)(hdir * 2), 0x00020000);
      const unsigned wv = (p.ablate & 2) ? kOOB : (unsigned)(wave * NT * 2048 + lane * 16);
      const unsigned hv = (p.ablate & 1) ? kOOB : (unsigned)((((b0 >> 4) * p.KQ2 + wave) * 2048) + lane * 16);
      const unsigned h_mt = p.KQ2 * 2048, h_hl = 1024;
      for (int qb = 0; qb < p.KQ2; qb += 4 * QB3) {
        u32x4 a[QB3][MT][2], w[QB3][NT][2];
#pragma unroll
        for (int i = 0; i < QB3; ++i) {
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int hl = 0; hl < 2; ++hl)
              a[i][mt][hl] = __builtin_amdgcn_raw_buffer_load_b128(rh, hv + mt * h_mt + hl * h_hl + (qb + 4 * i) * 2048, 0, 0);
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int hl = 0; hl < 2; ++hl)
              w[i][nt][hl] = __builtin_amdgcn_raw_buffer_load_b128(rw, wv + (nt * 2 + hl) * 1024 + (qb + 4 * i) * NT * 2048, 0, 0);
        }
        if (qb == 0) load_epilogue_inputs();
        if (stamp) p.dbg[p.step * 8 + 2] = clock64();
#pragma unroll
        for (int i = 0; i < QB3; ++i) {
          if (qb + wave + 4 * i < p.KQ2 && !(p.ablate & 4)) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
              for (int nt = 0; nt < NT; ++nt) {
                const s16x8 ah = __builtin_bit_cast(s16x8, a[i][mt][0]), al = __builtin_bit_cast(s16x8, a[i][mt][1]);
                const s16x8 wh = __builtin_bit_cast(s16x8, w[i][nt][0]), wl = __builtin_bit_cast(s16x8, w[i][nt][1]);
                acc[mt][nt] = mfma_bf16(al, wh, acc[mt][nt]);   // small terms first
                acc[mt][nt] = mfma_bf16(ah, wl, acc[mt][nt]);
                acc[mt][nt] = mfma_bf16(ah, wh, acc[mt][nt]);
              }
          }
        }
      }
    } else {
      const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(p.whh + (long)(dir * p.NU + ugi) * p.KQ * NT * 256), 0, p.KQ * NT * 1024, 0x00020000);
      // fp32 hand-off image in A-fragment order (same reason as the split-bf16 form): [slot][dir][m-tile][q][lane][4]
      const int nmt = (p.B + 15) >> 4;
      const long hdir = (long)nmt * p.KQ * 256;                       // floats per (slot, direction)
      const __amdgpu_buffer_rsrc_t rh = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(reinterpret_cast<float*>(p.hs) + ((long)((p.step - 1) & 1) * 2 + dir) * hdir), 0, (int)(hdir * 4),
          0x00020000);
      const unsigned wv = (p.ablate & 2) ? kOOB : (unsigned)(wave * NT * 1024 + lane * 16);
      const unsigned hv = (p.ablate & 1) ? kOOB : (unsigned)((((b0 >> 4) * p.KQ + wave) * 1024) + lane * 16);
      const unsigned h_mt = p.KQ * 1024;
      for (int qb = 0; qb < p.KQ; qb += 4 * QB) {
        u32x4 a[QB][MT], w[QB][NT];
#pragma unroll
        for (int i = 0; i < QB; ++i) {
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
            a[i][mt] = __builtin_amdgcn_raw_buffer_load_b128(rh, hv + mt * h_mt + (qb + 4 * i) * 1024, 0, 0);
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            w[i][nt] = __builtin_amdgcn_raw_buffer_load_b128(rw, wv + nt * 1024 + (qb + 4 * i) * NT * 1024, 0, 0);
        }
        if (qb == 0) load_epilogue_inputs();
#pragma unroll
        for (int i = 0; i < QB; ++i) {
          if (qb + wave + 4 * i < p.KQ && !(p.ablate & 4)) {  // wave-uniform: skip chunks past the end of K
            float4 af[MT], wf[NT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) af[mt] = __builtin_bit_cast(float4, a[i][mt]);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) wf[nt] = __builtin_bit_cast(float4, w[i][nt]);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
              for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                  acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4c(af[mt], r), f4c(wf[nt], r), acc[mt][nt], 0, 0, 0);
          }
        }
      }
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[((wave * MT * NT + mt * NT + nt) * 4 + r) * RLD + lane] = acc[mt][nt][r];
    if (stamp) p.dbg[p.step * 8 + 3] = clock64();
    __syncthreads();
    if (stamp) p.dbg[p.step * 8 + 4] = clock64();
  }

  // ---- fused cell update: one (batch row, hidden unit) per thread
#pragma unroll
  for (int i = 0; i < EPT; ++i) {
    const int e = tid + 256 * i;
    const int row = e / UG, ju = e % UG, b = b0 + row;
    if (e < NE && b < p.B) {
      float pre[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float s = 0.0f;
        if (!first) {
          const int pl = ju * 4 + g;
          const int tile = (row >> 4) * NT + (pl >> 4);
          const int src = (((row & 15) >> 2) << 4) + (pl & 15), r = row & 3;
#pragma unroll
          for (int w = 0; w < 4; ++w) s += red[((w * MT * NT + tile) * 4 + r) * RLD + src];
        }
        pre[g] = s + gpre[i][g];
      }
      float ig, fg2, gg, og, cn, h;
      if (p.ablate & 16) {   // profiling: libm-grade activations
        ig = 1.0f / (1.0f + expf(-pre[0]));
        fg2 = 1.0f / (1.0f + expf(-pre[1]));
        gg = tanhf(pre[2]);
        og = 1.0f / (1.0f + expf(-pre[3]));
        cn = fg2 * cold[i] + ig * gg;
        h = og * tanhf(cn);
      } else {
        ig = gate_sigmoid(pre[0]);
        fg2 = gate_sigmoid(pre[1]);
        gg = gate_tanh(pre[2]);
        og = gate_sigmoid(pre[3]);
        cn = fg2 * cold[i] + ig * gg;
        h = og * gate_tanh(cn);
      }
      if constexpr (DBG) {   // ragged batch: a row holds h = c = 0 outside its own frames (the reverse direction starts at the
        if (frames && t >= frames[b]) { h = 0.0f; cn = 0.0f; }   // row's last frame, the forward direction ends there)
      }
      if constexpr (X3) {   // hand h_t to the next step already split (3 VALU ops here vs hundreds in the consumer)
        unsigned short hi, lo;
        split_bf16(h, hi, lo);
        const int k = ugi * UG + ju, nmt = (p.B + 15) >> 4;
        unsigned short* dst = p.hs + ((((long)(p.step & 1) * 2 + dir) * nmt + (b >> 4)) * p.KQ2 + (k >> 5)) * 1024 +
                              ((b & 15) + 16 * ((k >> 3) & 3)) * 8 + (k & 7);
        dst[0] = hi;
        dst[512] = lo;
      } else {
        const int k = ugi * UG + ju, nmt = (p.B + 15) >> 4;
        reinterpret_cast<float*>(p.hs)[((((long)(p.step & 1) * 2 + dir) * nmt + (b >> 4)) * p.KQ + (k >> 4)) * 256 +
                                       ((b & 15) + 16 * ((k >> 2) & 3)) * 4 + (k & 3)] = h;
      }
      p.c[((long)dir * p.B + b) * p.Hp + ugi * UG + ju] = cn;
      p.y[((long)(t * p.B + b) * 2 + dir) * p.Hp + ugi * UG + ju] = h;
      if constexpr (DBG) {
        if (save_g) {
          *reinterpret_cast<float4*>(save_g + ((long)(t * p.B + b) * 2 + dir) * p.NP + ugi * 4 * UG + ju * 4) = make_float4(ig, fg2, gg, og);
          save_c[((long)(t * p.B + b) * 2 + dir) * p.Hp + ugi * UG + ju] = cn;
        }
      }
    }
  }
  if (stamp) { p.dbg[p.step * 8 + 5] = clock64(); p.dbg[p.step * 8 + 6] = wall_clock64(); }
}



// -------------------------------------------------------------------------------------------------
// K4, XCD-local persistent form (split-bf16 only): ONE launch runs all T steps of a layer.
//
// A (direction, batch-row group) recurrence is an exchange group of NU <= 32 workgroups, one hidden-unit
// group each, and the launch places every member of a group on the SAME XCD (workgroup b is observed to run
// on XCD b % 8, so group = b % 8, member = b / 8).  W_hh never leaves the register file, the cell state stays
// in registers, and h_t moves between the members through that XCD's own L2.
//
// The exchange is DATA-TAGGED (round 2; the round-1 form -- stores, s_waitcnt vmcnt(0), a flag per wave, one polling
// wave, a barrier, then the fragment loads -- spent ~1600 of a step's ~4700 clocks on the flag's two extra L2 trips):
//   * |h| < 1, so bit 14 (the exponent's top bit) of its bf16 halves is always 0.  A producer lane stores the four
//     units of its lane quad as one aligned 8-byte word (hi halves, or lo halves) and puts the step's tag into bit 14
//     of the first element of EACH dword: tag(step) = ((step >> 1) & 1) ^ 1, so the two writes that follow each other
//     in a slot (slot = step & 1) always differ, and a freshly zeroed slot differs from the first write.  No drain, no flag;
//   * a consumer wave polls the DATA: it loads its k-chunks of the fragment-ordered h image (sc1: served by L2), checks
//     the tag of every dword it received, clears it, multiplies the chunks that are complete and re-loads the
//     others.  A dword is the unit the memory system never tears (8-byte words WERE seen half old, half new on small
//     shapes, where consumers poll within nanoseconds of the store); every dword carries its own tag, so nothing depends
//     on the order in which stores -- or halves of a store -- become visible.
//   * every launch starts by zeroing its own words of both slots, BEFORE the start-up barrier below.
// One workgroup barrier is left in a step (partial sums -> cell update; the partial sums are double-buffered).
//
// Shape of a step inside a workgroup:
//   * K is split over the NW waves; the MFMA operands are SWAPPED (A = W fragments, B = h fragments), so a lane's
//     four accumulator registers are the four gates of ONE (hidden unit, batch row): partial sums go to the LDS as
//     one 16-byte store per tile and the cell update reads them back 16 bytes at a time;
//   * groups of <= 8 batch rows (B <= 32) would leave half of every 16-wide MFMA tile empty: the hand-off image is
//     STACKED instead -- columns 0..RG-1 of the tile are the bf16 hi halves of the rows, RG..2RG-1 their lo halves
//     -- so that TWO MFMAs (x W_hi, x W_lo) give all four hi/lo products (the three the split form needs plus lo*lo)
//     and the group's h is one KiB per 32-wide k-chunk instead of two half-empty ones;
//   * the four units of a lane quad are gathered with DPP: lanes 0 / 1 store the hand-off words (hi / lo), lanes 2 / 3 the
//     same halves into the next GEMM's operand image.
//
// Correctness never rests on the placement.  At start-up every member publishes its HW_REG_XCC_ID with
// agent-scope atomics; only if all ids of a group agree does the group use L2-local accesses (plain stores, sc1
// loads), otherwise the same loop runs with write-through stores and system-scope loads (sc0 sc1 on both sides),
// which is valid for any placement -- the tags make fences unnecessary there too.  Every spin is bounded; a timeout
// raises the abort word, all workgroups leave, and the status word tells the host.  A non-finite h (NaN input) cannot
// carry a tag: it is replaced by 0 and reported in status word 282 (the host raises; ONSSEN_XCD=0 propagates NaNs).
// -------------------------------------------------------------------------------------------------
// Profiling is a BUILD variant (tools/ab_variants.py build prof "-DONSSEN_XCD_PROFILE=1 -DONSSEN_XCD_ABLATE=<bits>"): a run-time
// switch inside the step costs scalar registers and branches on the critical path of every time step.
//   ONSSEN_XCD_PROFILE=1  timestamps of steps 64..127 of workgroup 0 (tools/xcd_timeline.py)
//   ONSSEN_XCD_ABLATE     1 = no h loads, 2 = no input-projection loads, 4 = no MFMA, 16 = no y / image stores,
//                         64 = no LDS reads in the cell update, 128 = no gate non-linearities   (results are garbage)
#ifndef ONSSEN_XCD_DELAY_CELL
#define ONSSEN_XCD_DELAY_CELL 0      // s_sleep argument (64 clocks each) before the next step's chunks are requested: waves with elements
#define ONSSEN_XCD_DELAY_IDLE 0      // ... waves without
#endif
#ifndef ONSSEN_XCD_EMAP
#define ONSSEN_XCD_EMAP 0
#endif
#ifndef ONSSEN_XCD_ST_AUX
#define ONSSEN_XCD_ST_AUX 0          // cache-policy bits of the hand-off stores when the group sits on one XCD (1 = sc0, 16 = sc1)
#endif
#ifndef ONSSEN_XCD_GEARLY
#define ONSSEN_XCD_GEARLY 0          // round 6: 1 = the loader waves request the NEXT step's input-projection slice as soon as their h chunks of THIS
                                     // step have arrived (before the MFMAs) instead of right after the barrier: an HBM-latency load that sits in
                                     // the CU's in-order vector-memory pipe in front of the next chunk requests holds them back
#endif
#ifndef ONSSEN_XCD_FETCH_FIRST
#define ONSSEN_XCD_FETCH_FIRST 0     // round 6: 1 = the loader waves request the next step's h chunks BEFORE they park the staged slice in the LDS
                                     // (the park waits for the slice's loads; the request does not depend on them)
#endif
#ifndef ONSSEN_XCD_REQ_EARLY
#define ONSSEN_XCD_REQ_EARLY 0       // round 6: 1 = the cell-update waves request the next step's h chunks right behind the hand-off store, before
                                     // the output stores (round 2 measured this slower; re-measured with the loader path shortened)
#endif
#ifndef ONSSEN_XCD_SKIP_OOR
#define ONSSEN_XCD_SKIP_OOR 0        // round 6: 1 = a wave does not issue the loads of chunk slots past its last k-chunk (H = 600: 19 chunks in 8 x 3
                                     // slots).  An out-of-range buffer load moves no data but still passes the CU's address unit (tools/micro/
                                     // l2_gather_probe: a 16-byte wave load costs ~16 clocks of it whether its lanes are in range or not)
#endif
#ifndef ONSSEN_XCD_TILE_GROUPS
#define ONSSEN_XCD_TILE_GROUPS 0     // round 6: the gate tiles of a wave are multiplied GROUP by group (decimal digits = group sizes, e.g. 221 for
                                     // NT = 5: tiles {0,1}, {2,3}, {4}) -- every chunk's products of a group, then that group's partial sums go to
                                     // the LDS under the next group's MFMAs instead of all NT ds_write_b128 (13 LDS cycles each, 8 waves at once)
                                     // behind the last MFMA.  Per accumulator the order of the terms is unchanged: same bits.  0 = one group
#endif
#ifndef ONSSEN_XCD_PROFILE_WG
#define ONSSEN_XCD_PROFILE_WG 0      // which workgroup is stamped (0 = member 0 of group 0)
#endif
#ifndef ONSSEN_XCD_PROFILE
#define ONSSEN_XCD_PROFILE 0
#endif
#ifndef ONSSEN_XCD_ABLATE
#define ONSSEN_XCD_ABLATE 0
#endif
#ifndef ONSSEN_XCD_IDLE_SLEEP
#define ONSSEN_XCD_IDLE_SLEEP 1      // s_sleep argument (x 64 clocks) of the waves that wait for this member's cell update
#endif
#ifndef ONSSEN_XCD_EARLYX_SLEEP
#define ONSSEN_XCD_EARLYX_SLEEP 0    // s_sleep argument (x 64 clocks) before the fused first layer's early x products (their W_ih fragment
#endif                               // reads share the LDS with the cell update's partial-sum reads)
#ifndef ONSSEN_XCD_LDS_BATCH1
#define ONSSEN_XCD_LDS_BATCH1 1      // the cell update's 16 partial-sum reads in ONE batch instead of two where the registers allow it (the plain
                                     // stacked form, 213 -> 242 VGPRs): 1.421-1.427 vs 1.439-1.443 us per step, same summation order, same bits
#endif
#ifndef ONSSEN_XCD_LDS_BATCH1U
#define ONSSEN_XCD_LDS_BATCH1U 0     // round 6: the same for the UNSTACKED 16-row tile (8 reads per element): 1.547-1.549 vs 1.550-1.553 ms per pipelined step,
                                     // inside the noise, and slower together with the priority above (1.543-1.545 vs 1.532-1.534): off
#endif
#ifndef ONSSEN_XCD_PAIRED
#define ONSSEN_XCD_PAIRED 0          // experiment (round 3): K split 4 ways over wave PAIRS that share their h chunks through the LDS
#endif
#ifndef ONSSEN_XCD_CELL_PRIO
#define ONSSEN_XCD_CELL_PRIO 0       // s_setprio of the waves that run the cell update (they share their SIMDs with waiting waves)
#endif
#ifndef ONSSEN_XCD_DELAY_CELL_U
#define ONSSEN_XCD_DELAY_CELL_U 12   // ONSSEN_XCD_DELAY_CELL of the UNSTACKED 16-row instantiations only: there the five cell-update waves asked for the
                                     // next chunks ~700 clocks before the hand-off stores were visible, and a failed polling pass costs ~1 100 clocks of the
                                     // CU's address unit (48 wave loads), in front of the loader waves' passes too.  Pipelined step, same box, x 64 clocks:
                                     // 0 / 2 / 4 / 8 / 10 / 12 / 16 / 20 / 24 = 1.542-1.547 / 1.583* / 1.575* / 1.505-1.510 / 1.503-1.504 / 1.501-1.504 /
                                     // 1.505-1.506 / 1.526-1.528 / 1.561-1.567 ms (* another box, base 1.597-1.604: profiles/r06_delay_ab.txt)
#endif
#ifndef ONSSEN_XCD_DELAY_CELL_S
#define ONSSEN_XCD_DELAY_CELL_S 2    // ... and of the STACKED inference instantiations (8- / 4-row groups, plain and fused first layer): one-batch headline step,
                                     // same box, two runs each, x 64 clocks: 0 / 2 / 4 / 8 / 12 = 1.852-1.854 / 1.841 / 1.844 / 1.872-1.874 / 1.889 ms; plain
                                     // recurrence 1.412 / 1.396 / 1.400-1.404 / 1.414-1.417 / 1.440 us per time step (profiles/r06_delay_ab.txt)
#endif
#ifndef ONSSEN_XCD_DELAY_CELL_T
#define ONSSEN_XCD_DELAY_CELL_T 0    // ... and of the training forward (SAVE: gates and cell states are stored before the request)
#endif
#ifndef ONSSEN_XCD_CELL_PRIO_U
#define ONSSEN_XCD_CELL_PRIO_U 2     // ... of the UNSTACKED 16-row instantiations only (five of eight waves run the cell update there, beside three that
                                     // stage the next input-projection slice): same-box A/B on the pair launch of the pipelined step, two rounds each --
                                     // priority 0 / 1 / 2 / 3: 1.558-1.562 / 1.541-1.543 / 1.536-1.539 / 1.543-1.544 ms per step; on the stacked 8-row groups
                                     // priority 2 moved the recurrence 1.411 -> 1.401 us per time step and the step not at all (profiles/r06_prio_ab.txt): 0 there
#endif
// ONSSEN_XCD_TILE_GROUPS helpers: decimal digits, most significant first = group sizes in tile order
constexpr int tile_group_count(int code) { int n = 0; for (; code > 0; code /= 10) ++n; return n; }
constexpr int tile_group_sum(int code) { int n = 0; for (; code > 0; code /= 10) n += code % 10; return n; }
constexpr int tile_group_size(int gi) {       // size of group gi (0 = first)
  int code = ONSSEN_XCD_TILE_GROUPS, n = tile_group_count(code);
  for (int k = n - 1; k > gi; --k) code /= 10;
  return code % 10;
}
struct XcdArgs {
  const float* G = nullptr;               // [T][B][2][NP]
  const unsigned short* whh = nullptr;    // split-bf16 image [2][NU][KQ2][NT][2][64][8]
  float* y = nullptr;                     // [T][B][2][Hp]
  unsigned short* hx = nullptr;           // per group: [2 slots][KQ2][2048 B]; a chunk is [hi|lo][64][8] bf16, or -- stacked -- one
                                          // [64][8] piece whose lane (r + 16 kg) holds row r (hi) for r < RG and row r - RG (lo) above
  unsigned* sync = nullptr;               // u32 words: [256 + g] arrivals, [280] abort, u64 pairs at [320 + 4g]: max(xcc+1), max(16-xcc),
                                          // [281] status (1 = some group ran the placement-independent accesses), [282] non-finite h seen,
                                          // [288 + g] launch generation.  The block is zeroed ONCE
                                          // by the workspace owner: everything in it is monotonic, so no launch depends on a
                                          // per-launch memset reaching this XCD's L2 (hipGraph replays showed that it may not)
  int B = 0, T = 0, Hp = 0, NP = 0, KQ2 = 0, NU = 0, row0 = 0, nbg = 0;
  const unsigned short* wih0 = nullptr;   // FUSE_IN0: fragment image of the layer's W_ih [2][NU][KC0][NT][hi|lo][64][8], else null
  const unsigned short* ximg = nullptr;   // FUSE_IN0: x3 image of the layer's input rows [T*B][KC0][2][32]
  const float* bias0 = nullptr;           // FUSE_IN0: [2*NP] packed bias (G column order)
  int KC0 = 0;                            // FUSE_IN0: ceil(in_dim / 32) <= 5 with KCM <= 4, else 0
  int KCM = 0;                            // FUSE_IN0: chunks multiplied on the MFMA pipe: KC0, or KC0 - 1 when in_dim = 32*KCM + 1 (129, 257:
                                          // the lone last column is a rank-1 update on the VALU in the cell update instead)
  const float* x0 = nullptr;              // FUSE_IN0 tail: fp32 input, element (b, t, k) at x0 + b*xs_b + t*xs_t + k
  long xs_b = 0, xs_t = 0;
  const float* wtail = nullptr;           // FUSE_IN0 tail: column in_dim-1 of the packed W_ih, [2*NP] (G column order)
  float* save_g = nullptr;                // SAVE: [T][B][2][NP] gate activations (i, f, g, o) in G's column layout, else null
  float* save_c = nullptr;                // SAVE: [T][B][2][Hp] cell states
  int terms = 0;                          // 3 = split-bf16 products, 1 = plain bf16 products (ONSSEN_BLSTM_BF16)
  int RG = 0;                             // batch rows per exchange group: 16, or 8 / 4 when the batch is small enough to give
                                          // every XCD a group anyway (the MFMA tile stays 16 wide: see STACK)
  unsigned spin_limit = 0;
  long long* dbg = nullptr;               // ONSSEN_XCD_PROFILE builds: where the timestamps go, or null
  int ablate = 0;                         // test only: 8 = rotate groups over XCDs (the placement-independent accesses run with real cross-XCD traffic)
  unsigned short* yimg = nullptr;         // x3 image [T*B][KBI][2][32] of the layer output (the next GEMM's A operand), or null
  int KBI = 0;                            // ceil(2*Hp / 32)
  const int* frames = nullptr;            // RAGGED: [B] frames of every batch row (<= T): a row holds h = c = 0 at t >= frames[b], or null
  // PAIR launch (round 6, onssen_blstm_pipe2_forward_f32): the batch groups bg >= nbg_a of a launch are a SECOND recurrence -- another
  // layer's weights and input projection over the same rows [row0, row0 + nbg_a RG) -- that shares nothing with the first but the launch:
  // layer 1 of batch n-1 on one half of the XCDs, layer 0 of batch n on the other (16-row groups: the B = 64 cost per time step for
  // two B = 32 recurrences that would otherwise run one after the other on 8-row groups).  nbg_a = 0: an ordinary launch
  int nbg_a = 0;
  const float* G_b = nullptr;             // second recurrence: input projection ...
  const unsigned short* whh_b = nullptr;  // ... recurrent weight image ...
  unsigned short* yimg_b = nullptr;       // ... and output image (no fp32 rows)
  // RAGGED pair launch (round 6c, onssen_blstm_pipe2_forward_ragged_f32): the two recurrences belong to two DIFFERENT ragged batches of
  // whole utterances, each padded to its own longest one -- the second recurrence runs T_b time steps over rows of frames_b[b] frames
  int T_b = 0;                            // RAGGED: time steps of the second recurrence (a uniform pair runs T in both)
  const int* frames_b = nullptr;          // RAGGED: [B] frames of the second recurrence's rows
  // AUX workgroups (onssen_blstm_pipe2_map_forward_f32): the aux_n workgroups behind the 8 NU members build the target map of the
  // second recurrence's batch (kmeans2_map_workgroup, labels_cluster.inc) on the CUs the members leave free; they share nothing with
  // the recurrences but the launch.  aux_n = 0: an ordinary launch
  int aux_n = 0, aux_D = 0;
  float aux_db = 0.f;
  const float* aux_feat = nullptr;        // [B][aux_per_utt] log-magnitude
  long aux_per_utt = 0, aux_stride = 0;   // bins per utterance; floats per utterance of the clustering workspace's header
  float* aux_w = nullptr;                 // clustering workspace: header ...
  int* aux_iw = nullptr;                  // ... int words ...
  int* aux_dest = nullptr;                // ... target map
};

// broadcast lane J of every lane quad (DPP quad_perm, one VALU op; all four lanes of a quad must be active)
template <int J>
__device__ __forceinline__ unsigned quad_bcast(unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, J * 0x55, 0xf, 0xf, false);
}

// FUSE: the first layer's input projection is computed in here (ONSSEN_BLSTM_FUSE_IN0); a compile-time switch so that
// the plain instantiation carries none of its registers
// SAVE (training forward, lstm_bwd.inc): also leaves the gate activations (in G's layout) and the cell states
// TERMS: 3 = split-bf16 products, 1 = plain bf16 (hi halves only), 0 = EXACT fp32 (round 3: v_mfma_f32_16x16x4_f32 on fp32
// fragment images -- the weights of onssen_lstm_pack_f32, the hand-off as tagged fp32 words; ONSSEN_PRECISION=f32 no longer
// needs one launch per time step).  STACK: hi and lo halves of <= 8 rows share a tile.
// RAGGED (round 4): the batch rows are whole utterances of different lengths padded to T (the shape the reference's evaluation
// runs one by one, onssen/utils/test.py:29-41): row b is live at t < frames[b] and holds h = c = 0 elsewhere -- the reverse
// direction then starts from zero state at the row's own last frame, the forward direction stops there -- so every row's
// outputs at its own frames are what a batch-1 run of that utterance gives, bit for bit (a tile column never sees its
// neighbours).  A template flag: one compare and two selects per element and step that the other instantiations do not carry.
// AUX (the uniform pair launch of onssen_blstm_pipe2_map_forward_f32 only): the workgroups behind the 8 NU members build a target map
// and return -- a template flag, so that no other instantiation carries the branch.
template <int NT, int NW, bool FUSE, int TERMS, bool STACK, bool SAVE = false, bool RAGGED = false, bool AUX = false>
__global__ __launch_bounds__(64 * NW) void lstm_xcd_kernel(XcdArgs p) {
  static_assert(!STACK || TERMS == 3, "stacking is a property of the split form");
  static_assert(!AUX || (TERMS == 3 && !FUSE && !SAVE && !RAGGED), "aux workgroups ride in the uniform pair launch");
  constexpr bool F32 = TERMS == 0;
  static_assert(!F32 || (!FUSE && !SAVE), "the exact-fp32 form is the plain inference recurrence");
  static_assert(NW == 8, "waves 5..7 never own elements: they stage the input projection");
  static_assert(!RAGGED || (TERMS == 3 && STACK && !FUSE && !SAVE), "ragged batches: the plain stacked split-bf16 inference recurrence");
  constexpr int UG = 4 * NT;
  constexpr int NE = 16 * UG;
  constexpr int NTHR = 64 * NW;                // NW = 4 or 8 waves: two waves per SIMD issue MFMAs ~1.4x denser than one
  constexpr int EPT = (NE + NTHR - 1) / NTHR;
  // k-chunks per wave: 32 k each (bf16 forms: NW x CPW x 32 >= 640 >= H) or 16 k each (fp32: four 16x16x4 MFMA steps per
  // 16-byte fragment; NW x CPW x 16 >= 640)
  // PAIRED (round-3 experiment): waves (p, p + 4) share a K quarter (chunks p, p + 4, ...): wave p + 4 polls the L2, multiplies
  // the first NTA gate tiles and hands the checked fragments to wave p through the LDS, which multiplies the other tiles --
  // half the partial sums (4 K parts instead of 8), half the polling waves, no chunk requested twice
  constexpr bool PAIRED = ONSSEN_XCD_PAIRED && STACK && !FUSE && NT >= 2;     // (the stacked forms: B <= 32)
  constexpr int NTA = PAIRED ? (NT + 1) / 2 : NT;          // gate tiles of the polling wave / register tiles of any wave
  constexpr int NKP = PAIRED ? 4 : NW;                     // K parts = partial-sum sets per step
  constexpr int CPW = F32 ? 40 / NW + (40 % NW != 0) : PAIRED ? 5 : 20 / NW + (20 % NW != 0);
  constexpr int CHB = F32 ? 1024 : 2048;          // bytes of a k-chunk in the hand-off image
  constexpr int NHL = TERMS == 3 ? 2 : 1;          // weight fragment halves kept
  constexpr int NLD = (TERMS == 3 && !STACK) ? 2 : 1;   // 16-byte h-fragment loads per chunk
  // LDS bytes per 16-lane block of a partial-sum tile / per tile: with 320 / 1296 the cell update's 16-byte reads (lane ->
  // element (row, unit) = (e / UG, e % UG)) fall on 16 different bank slots in each of ds_read_b128's four 16-lane groups, for
  // 8- and 16-row groups alike (272 / 1088 left 108 two-way conflicts per pass: SQ_LDS_BANK_CONFLICT 18.4 M per launch)
  constexpr int PBS = 320, PTS = 4 * PBS + 16;
  // bit 14 of the first bf16 of every dword of the hand-off image; fp32 form: bit 30 of every word (|h| < 1 < 2: always 0)
  constexpr unsigned TAG = F32 ? 0x40000000u : 0x4000u;
  // tile groups (ONSSEN_XCD_TILE_GROUPS): only where the digits add up to this instantiation's NT (bf16 forms, not the PAIRED experiment)
  constexpr int NGRP = tile_group_count(ONSSEN_XCD_TILE_GROUPS);
  constexpr bool GROUPED = !F32 && !PAIRED && NGRP > 1 && tile_group_sum(ONSSEN_XCD_TILE_GROUPS) == NT;
  __shared__ __attribute__((aligned(16))) char part_s[2 * NKP * NT * PTS];   // partial sums, [step parity][K part][tile][4 blocks]
  __shared__ __attribute__((aligned(16))) u32x4 share_s[PAIRED ? 4 * CPW * NLD * 64 : 1];   // PAIRED: checked h fragments, [pair][chunk][hi|lo][lane]
  __shared__ unsigned share_flag[4];           // PAIRED: step + 1 once the pair's fragments of `step` are in share_s
  constexpr int KCMAX = 4;                       // fused layer-0 input projection: <= 4 k-chunks on the MFMA pipe (in_dim <= 128, or 129 with the tail form)
  __shared__ unsigned s_ctl[3];                // [0] abort, [1] fast, [2] launch generation
  __shared__ unsigned s_done[8];               // [0] counts the (wave, step) pairs whose h has been stored (waves with elements)
  // profiling only: timestamps of steps 64..127 of workgroup 0 are collected in the LDS (a stamp stored to memory would sit
  // in vmcnt and be waited for with everything else) and written out when the launch ends
#ifndef ONSSEN_XCD_PROFILE_STN
#define ONSSEN_XCD_PROFILE_STN 64     // stamped steps (12 KB of LDS; the fused instantiations only have room for 32)
#endif
  constexpr int ST0 = 64, STN = ONSSEN_XCD_PROFILE_STN;
  constexpr bool PROF = ONSSEN_XCD_PROFILE != 0;
  constexpr int ABL = ONSSEN_XCD_ABLATE;
  constexpr int DELAY_CELL = ONSSEN_XCD_DELAY_CELL ? ONSSEN_XCD_DELAY_CELL : (!STACK && TERMS == 3 && !FUSE) ? ONSSEN_XCD_DELAY_CELL_U
                             : (STACK && !SAVE) ? ONSSEN_XCD_DELAY_CELL_S : SAVE ? ONSSEN_XCD_DELAY_CELL_T : 0;
  constexpr int CELL_PRIO = ONSSEN_XCD_CELL_PRIO ? ONSSEN_XCD_CELL_PRIO : (!STACK && TERMS == 3 && !FUSE) ? ONSSEN_XCD_CELL_PRIO_U : 0;
  __shared__ long long stamp_s[PROF ? STN * 24 : 1];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform by construction: tell the compiler (scalar branches)
  if constexpr (AUX) {
    // not a member of any group: no barrier of theirs, no arrival, no word of p.sync or p.hx -- only the map, in the LDS of the
    // partial sums (free here), and out
    static_assert(sizeof(part_s) >= NTHR * 8 + 512, "the map's scratch fits the partial sums' LDS");
    if ((int)blockIdx.x >= 8 * p.NU) {
      kmeans2_map_workgroup<NTHR>(p.aux_feat, p.aux_per_utt, p.aux_db, p.aux_w, p.aux_stride, p.aux_iw, p.aux_dest, p.aux_D, p.B,
                                  (int)blockIdx.x - 8 * p.NU, p.aux_n, part_s);
      return;
    }
  }
  // group = workgroup id mod 8 (the XCD the dispatcher is observed to use); test bit 8 rotates the groups across
  // the XCDs instead, so that the placement-independent accesses run with real cross-XCD traffic
  const int ugi = blockIdx.x >> 3, g = (p.ablate & 8) ? ((blockIdx.x + ugi) & 7) : (blockIdx.x & 7);
  if (PROF && p.dbg && tid == 0)               // where did the dispatcher put this workgroup?
    p.dbg[4096 + blockIdx.x] = (long long)(__builtin_amdgcn_s_getreg(6164) & 15u) |
                               ((long long)__builtin_amdgcn_s_getreg(63492) << 8);   // hwreg(HW_REG_HW_ID)
  if (g >= 2 * p.nbg) return;                  // whole workgroup, before any barrier
  const int dir = g / p.nbg;
  int bg = g % p.nbg;
  if (p.nbg_a > 0 && bg >= p.nbg_a) {          // PAIR launch: this group belongs to the second recurrence (wave-uniform: scalar selects, once)
    bg -= p.nbg_a;
    p.G = p.G_b; p.whh = p.whh_b; p.yimg = p.yimg_b; p.y = nullptr;
    // (the ragged instantiation only: a uniform pair has T_b == T, and the selects in every instantiation measured 1.551-1.552 against
    //  1.546-1.549 ms per pipelined step on one box -- code placement, not work; round 6c)
    if constexpr (RAGGED) { p.T = p.T_b; p.frames = p.frames_b; }
  }
  const int RG = p.RG;
  const int b0 = p.row0 + bg * RG;
  unsigned* abort_w = p.sync + 280;
  const long hx_group = (long)g * 2 * p.KQ2 * 1024;             // uint16 elements per group (two slots of KQ2 x 2048 bytes)
  const int KQX = F32 ? (p.Hp + 15) / 16 : p.KQ2;               // k-chunks of this form (the fp32 image fits: KQ <= 2 KQ2)

  // ---- per-thread constants of the cell update: element e = (row, ju) of this member's RG x UG tile; the four lanes
  //      of a quad hold four consecutive units of one row
  const int qj = tid & 3;                   // role of this lane in the quad's store: 0 / 1 hand-off hi / lo, 2 / 3 image hi / lo
  const unsigned lo_delta = STACK ? (unsigned)RG * 16u : 1024u;   // hand-off: byte distance from a hi piece to its lo piece
  const long g_step = (long)p.B * 2 * p.NP, y_step = (long)p.B * 2 * p.Hp, i_step = (long)p.B * p.KBI * 64;
  bool e_ok[EPT], e_inb[EPT];
  unsigned g_off[EPT], y_off[EPT];          // byte offsets inside a time step's slab of G / y
  unsigned g_off_st[EPT];                   // ... of the saved gates (SAVE), out of range for lanes without a row
  unsigned i_off[EPT];                      // byte offset of this lane's 4-unit image segment inside a time step's slab (lanes 2, 3)
  unsigned hx_off[EPT];                     // byte offset of this lane's 4-unit hand-off word inside a slot (lanes 0, 1)
  int red_off[EPT];                         // LDS byte offset of the wave-0 partial (all four gates) of this element
  int tlen[RAGGED ? EPT : 1];               // RAGGED: frames of this element's row (0 for rows past B)
  // element e -> (row, unit): consecutive quads are the SAME four units of consecutive rows, so that the hand-off store of
  // a wave (8 bytes per quad lane 0 / 1) fills whole 16-byte slots of neighbouring rows -- contiguous 128-byte runs --
  // instead of pieces of many lines (ONSSEN_XCD_EMAP=0: units fastest, the round-2a order)
  auto emap = [&](int e, int& row, int& ju) {
    if (ONSSEN_XCD_EMAP) { const int q = e >> 2; row = (q % RG) & 15; ju = ((q / RG) * 4 + (e & 3)) % UG; }
    else { row = (e / UG) & 15; ju = e % UG; }
  };
#pragma unroll
  for (int i = 0; i < EPT; ++i) {
    const int e = tid + NTHR * i;
    int row, ju;
    emap(e, row, ju);
    const int b = b0 + row, k = ugi * UG + ju, kq = k & ~3, ik = dir * p.Hp + kq;
    e_ok[i] = e < RG * UG;
    e_inb[i] = e_ok[i] && b < p.B;
    if constexpr (RAGGED) tlen[i] = e_inb[i] ? p.frames[b] : 0;
    g_off[i] = (unsigned)(((b * 2 + dir) * p.NP + ugi * 4 * UG + ju * 4) * 4);
    y_off[i] = (unsigned)(((b * 2 + dir) * p.Hp + k) * 4);
    i_off[i] = (unsigned)(((b * p.KBI + (ik >> 5)) * 64 + (ik & 31) + (qj & 1) * 32) * 2);
    if (F32)   // fp32 fragment image [chunk of 16 k][lane = row + 16 ((k >> 2) & 3)][k & 3], the k order of the weight image
      hx_off[i] = (unsigned)((k >> 4) * 1024 + (row + 16 * ((k >> 2) & 3)) * 16 + (k & 3) * 4);   // (every lane stores its own word)
    else
      hx_off[i] = (unsigned)((kq >> 5) * 2048 + (row + 16 * ((kq >> 3) & 3)) * 16 + (kq & 7) * 2) + (qj & 1) * lo_delta;
    red_off[i] = (ju >> 2) * PTS + (ju & 3) * PBS + row * 16;
    // lanes that do not take part store out of range: decided once, no select (or branch) in the step
    const bool live = e_inb[i] && !(ONSSEN_XCD_ABLATE & 16);
    if (!(e_ok[i] && (F32 || qj < (TERMS == 3 ? 2 : 1)))) hx_off[i] = 0x7ffffff0u;
    if (!(live && qj >= 2)) i_off[i] = 0x7ffffff0u;
    if (!live) y_off[i] = 0x7ffffff0u;
    if (!live) g_off_st[i] = 0x7ffffff0u; else g_off_st[i] = g_off[i];
  }
  // ---- this member's words of both hand-off slots start the launch untagged (zero); write-through, because the
  //      placement is not known yet
  {
    const __amdgpu_buffer_rsrc_t r2 = __builtin_amdgcn_make_buffer_rsrc((void*)(p.hx + hx_group), 0, p.KQ2 * 4096, 0x00020000);
#pragma unroll
    for (int i = 0; i < EPT; ++i)
      if (F32) {
        if (e_ok[i]) {
          __builtin_amdgcn_raw_buffer_store_b32(0u, r2, hx_off[i], 0, 17);
          __builtin_amdgcn_raw_buffer_store_b32(0u, r2, hx_off[i] + (unsigned)p.KQ2 * 2048u, 0, 17);
        }
      } else if (e_ok[i] && qj < (TERMS == 3 ? 2 : 1)) {
        __builtin_amdgcn_raw_buffer_store_b64(u32x2{0u, 0u}, r2, hx_off[i], 0, 17);
        __builtin_amdgcn_raw_buffer_store_b64(u32x2{0u, 0u}, r2, hx_off[i] + (unsigned)p.KQ2 * 2048u, 0, 17);
      }
    // the K padding of both slots (k in [Hp, 32 KQ2), fp32: [Hp, 16 KQX)) is nobody's element: it is never stored in a step and
    // never tag-checked, but it IS multiplied (by zero weights), so it must be finite -- the group's last member clears it
    // here, which is what lets the host drop its memset of the hand-off area (one launch per call)
    if (ugi == p.NU - 1) {
      constexpr int WPC = F32 ? 16 : 8;                        // 4-byte (fp32) / 4-unit 8-byte words per row of a chunk
      const int w0 = F32 ? p.Hp : p.Hp / 4, w1 = KQX * WPC, nrow = STACK ? 2 * RG : 16;
      for (int w = w0 * nrow + tid; w < w1 * nrow; w += NTHR) {
        const int wi = w / nrow, row = w - wi * nrow;
        if (F32) {
          const unsigned off = (unsigned)((wi >> 4) * 1024 + (row + 16 * ((wi >> 2) & 3)) * 16 + (wi & 3) * 4);
          __builtin_amdgcn_raw_buffer_store_b32(0u, r2, off, 0, 17);
          __builtin_amdgcn_raw_buffer_store_b32(0u, r2, off + (unsigned)p.KQ2 * 2048u, 0, 17);
        } else {
          // word wi = units 4 wi .. 4 wi + 3: chunk wi >> 3, k group (wi >> 1) & 3, half (wi & 1); stacked: row < RG hi, row >= RG lo;
          // otherwise the lo piece of a chunk follows its hi piece
#pragma unroll
          for (int hl = 0; hl < (STACK || TERMS != 3 ? 1 : 2); ++hl) {
            const unsigned off = (unsigned)((wi >> 3) * 2048 + (row + 16 * ((wi >> 1) & 3)) * 16 + (wi & 1) * 8) + (unsigned)hl * 1024u;
            __builtin_amdgcn_raw_buffer_store_b64(u32x2{0u, 0u}, r2, off, 0, 17);
            __builtin_amdgcn_raw_buffer_store_b64(u32x2{0u, 0u}, r2, off + (unsigned)p.KQ2 * 2048u, 0, 17);
          }
        }
      }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);   // s_waitcnt vmcnt(0): acknowledged by memory
    __syncthreads();
  }

  // ---- placement check: do all members of this group sit on one XCD?  (also the start-up barrier of the group)
  if (tid == 0) {
    const unsigned xcc = __builtin_amdgcn_s_getreg(6164) & 15u;      // hwreg(HW_REG_XCC_ID, 0, 4)
    // launch generation: bumped by member 0 once everybody has arrived, read here by everyone
    const unsigned gen0 = __hip_atomic_fetch_add(p.sync + 288 + g, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_ctl[2] = gen0;
    // max(xcc+1) and max(16-xcc) of THIS launch: tagged with the generation, so older launches (the dispatcher
    // may start a launch on another XCD) never win the max
    unsigned long long* xw = reinterpret_cast<unsigned long long*>(p.sync + 320) + 2 * g;
    __hip_atomic_fetch_max(xw, ((unsigned long long)gen0 << 8) | (xcc + 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(xw + 1, ((unsigned long long)gen0 << 8) | (16u - xcc), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __hip_atomic_fetch_add(p.sync + 256 + g, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned spins = 0, ab = p.spin_limit == 0u ? 1u : 0u;      // a spin limit of 0 aborts at once, whatever the timing (tests)
    // the arrival counter is never reset: NU arrivals per launch, so launch `gen0` ends at (gen0+1)*NU
    while (__hip_atomic_fetch_add(p.sync + 256 + g, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - gen0 * (unsigned)p.NU <
           (unsigned)p.NU) {
      __builtin_amdgcn_s_sleep(8);
      if (++spins > p.spin_limit || __hip_atomic_load(abort_w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { ab = 1; break; }
    }
    const unsigned hi = (unsigned)__hip_atomic_fetch_add(xw, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 255u;
    const unsigned lo = (unsigned)__hip_atomic_fetch_add(xw + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 255u;
    s_ctl[0] = ab;
    s_ctl[1] = (hi + lo == 17u) ? 1u : 0u;     // max(xcc)+1 + 16-min(xcc) == 17  <=>  max == min
    if (ab) __hip_atomic_store(abort_w, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!ab && s_ctl[1] == 0u) __hip_atomic_store(p.sync + 281, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // everybody has read the generation (they arrive after reading it): the next launch gets a new one
    if (!ab && ugi == 0) __hip_atomic_fetch_add(p.sync + 288 + g, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  }
  __syncthreads();
  if (s_ctl[0]) return;
  const bool fast = s_ctl[1] != 0;

  // ---- resident recurrent weights (hi and lo fragments), chunks q = wq, wq + NW, ... with wq = NW-1-wave: the waves that
  //      run the cell update (the low ones) start polling last, so they get the chunk counts that round down
  const int wq = NW - 1 - wave;
  const int pp = wave & 3;                                  // PAIRED: the pair (K quarter) of this wave ...
  const bool poller = !PAIRED || wave >= 4;                 // ... and whether it is the one that polls the L2
  const int tb = PAIRED && !poller ? NTA : 0;               // first gate tile / number of gate tiles of this wave
  const int ntw = PAIRED ? (poller ? NTA : NT - NTA) : NT;
  auto chunk_of = [&](int i) { return PAIRED ? pp + 4 * i : wq + NW * i; };   // k-chunk in slot i of this wave
  s16x8 w[CPW][NTA][NHL];
  {
    // (fp32 form: the image of onssen_lstm_pack_f32, [dir][unit group][chunk of 16 k][tile][64 lanes][4 floats]: a lane's four
    //  floats are its A operands of four consecutive 16x16x4 MFMA steps)
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(p.whh + (long)(dir * p.NU + ugi) * KQX * NT * (CHB / 2)), 0, KQX * NT * CHB, 0x00020000);
#pragma unroll
    for (int i = 0; i < CPW; ++i)
#pragma unroll
      for (int nt = 0; nt < NTA; ++nt)
#pragma unroll
        for (int hl = 0; hl < NHL; ++hl)
          w[i][nt][hl] = __builtin_bit_cast(s16x8, __builtin_amdgcn_raw_buffer_load_b128(
              rw, nt < ntw ? (unsigned)((chunk_of(i) * NT + tb + nt) * CHB + hl * 1024 + lane * 16) : 0x7ffffff0u, 0, 0));
  }
  // ---- fused input projection of the first layer (in_dim <= 160): x_t W_ih^T is accumulated into the same MFMA accumulators
  //      as h_{t-1} W_hh^T -- BEFORE the wait for h, which it does not depend on -- and G never exists in memory.  Its k-chunks
  //      go to the LAST waves (round 3: chunk c to wave NW-1 - c), which own no elements (all four at <= 8 rows, three of
  //      four at 16 rows): those have requested their h chunks ~800 clocks before they arrive and would only wait, while the
  //      waves that run the cell update (which got the chunks in rounds 1-2) are the critical path of the step.  The W_ih fragments stay in the LDS (40 more resident registers
  //      per wave spilled: 14-52 VGPRs to scratch in the step), a wave reads the fragments of its chunk two tiles at a time
  constexpr bool fuse = FUSE;
  constexpr int XS = FUSE ? KCMAX / NW + (KCMAX % NW != 0) : 1;
  __shared__ __attribute__((aligned(16))) unsigned short wx_s[FUSE ? KCMAX * NT * NHL * 512 : 8];   // [chunk][tile][hi|lo][64][8]
  if constexpr (FUSE) {
    const __amdgpu_buffer_rsrc_t rwx = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(p.wih0 + (long)(dir * p.NU + ugi) * p.KC0 * NT * 1024), 0, p.KC0 * NT * 2048, 0x00020000);
    for (int f = wave; f < KCMAX * NT * NHL; f += NW) {          // fragment f = (c * NT + nt) * NHL + hl
      const int hl = f % NHL, cn = f / NHL;
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(
          rwx, cn / NT < p.KCM ? (unsigned)(cn * 2048 + hl * 1024 + lane * 16) : 0x7ffffff0u, 0, 0);
      *reinterpret_cast<u32x4*>(wx_s + (long)f * 512 + lane * 8) = v;
    }
  }
  float cst[EPT];
#pragma unroll
  for (int i = 0; i < EPT; ++i) cst[i] = 0.0f;
  bool seen_nonfinite = false;
  // an output the caller does not want: a zero-sized buffer somewhere valid (no select on the pointer in the step)
  unsigned short* const yimg_base = p.yimg ? p.yimg : p.hx;
  float* const y_base = p.y ? p.y : reinterpret_cast<float*>(p.hx);
  const int yimg_bytes = p.yimg ? (int)(i_step * 2) : 0, y_bytes = p.y ? (int)(y_step * 4) : 0;
  const unsigned qsel = (qj & 1) ? 0x07060302u : 0x05040100u;   // v_perm_b32 selector of the quad gather (bytes 0-3 = second operand)
  const bool stamp = PROF && p.dbg && lane == 0 && blockIdx.x == ONSSEN_XCD_PROFILE_WG;      // wave 0: slots 0..8, last wave: 9..12
  auto mark = [&](int step, int slot) {       // ONSSEN_XCD_PROFILE is a bit mask of the slots that are stamped (a stamp costs ~100 clocks)
    if constexpr (PROF)
      if (((ONSSEN_XCD_PROFILE >> slot) & 1) && stamp && (unsigned)(step - ST0) < (unsigned)STN) stamp_s[(step - ST0) * 24 + slot] = clock64();
  };

  // ---- input projection of a step (G row slice, or -- fused first layer -- the lone tail column of x): vmcnt retires in
  //      order and the compiler cannot count across the polling loop, so a prefetch issued by the wave that consumes it
  //      is waited for (vmcnt(0)) long before it is needed -- an HBM latency on the critical path of every step.  The
  //      waves WITHOUT elements fetch it instead, during the cell update they would otherwise sleep through, and park it
  //      in the LDS (two step parities); the cell update reads it from there.  (Requesting it two steps ahead, behind the
  //      request for the next h chunks, measured slower: 2.43 vs 2.11 ms -- the wait for the chunks took the loads along.)
  constexpr int NLW = NW - 1;                                // at most this many loader waves (wave >= ncw)
  __shared__ __attribute__((aligned(16))) float gbuf_s[2 * NE * 4];
  const int ncw = (RG * UG + 63) / 64;                       // waves that own elements: wave < ncw  (NW = 8: ncw <= 5)
  const int nld = 64 * (NW - ncw);                           // loader lanes
  constexpr int LPT = (NE + 64 * (NW - 5) - 1) / (64 * (NW - 5));   // elements per loader lane, worst case (ncw = 5)
  auto stage_issue = [&](f32x4 (&gq)[LPT], int step) {       // request step `step`'s slice (lanes of the loader waves)
    const int t = dir == 0 ? step : p.T - 1 - step;
    const bool live = step < p.T && !(ABL & 2);
#pragma unroll
    for (int k = 0; k < LPT; ++k) {
      const int e = (tid - 64 * ncw) + nld * k;
      int row, ju;
      emap(e < 0 ? 0 : e, row, ju);
      const int b = b0 + row;
      const bool ok = live && wave >= ncw && e < RG * UG && b < p.B;
      if constexpr (FUSE) {
        const bool tl = p.KCM < p.KC0;                       // in_dim = 32*KCM + 1: the lone last column
        const __amdgpu_buffer_rsrc_t rxt = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(p.x0 + (tl && live ? (long)t * p.xs_t + 32 * p.KCM : 0)), 0, tl && live ? 0x7fffffe0 : 0, 0x00020000);
        gq[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        gq[k][0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rxt, ok ? (unsigned)((long)b * p.xs_b * 4) : 0x7ffffff0u, 0, 0));
      } else {
        const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc((void*)(p.G + (long)(live ? t : 0) * g_step), 0, (int)(g_step * 4), 0x00020000);
        gq[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
            rg, ok ? (unsigned)((((long)b * 2 + dir) * p.NP + ugi * 4 * UG + ju * 4) * 4) : 0x7ffffff0u, 0, 0));
      }
    }
  };
  auto stage_park = [&](const f32x4 (&gq)[LPT], int step) {  // ... and park it for the cell update of that step
#pragma unroll
    for (int k = 0; k < LPT; ++k) {
      const int e = (tid - 64 * ncw) + nld * k;
      if (e < RG * UG) *reinterpret_cast<f32x4*>(gbuf_s + ((step & 1) * NE + e) * 4) = gq[k];
    }
  };
  float bgate[EPT][4];
#pragma unroll
  for (int i = 0; i < EPT; ++i)
#pragma unroll
    for (int gt = 0; gt < 4; ++gt)
      bgate[i][gt] = (fuse && e_ok[i]) ? p.bias0[dir * p.NP + g_off[i] / 4 % p.NP + gt] : 0.0f;
  // input fragments of a step (B operand: 32-wide k chunk x batch columns, stacked like h when STACK); like G they
  // are fetched one step ahead into a second register set
  const int r16 = lane & 15;
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.ximg, 0, fuse ? (int)((long)p.T * p.B * p.KC0 * 128) : 0, 0x00020000);
  auto xchunk = [&](int ci) { return (NW - 1 - wave) + NW * ci; };      // input chunk of this wave in slot ci
  auto load_x = [&](u32x4 (&xf)[XS][NLD], int step) {
    const int t = dir == 0 ? step : p.T - 1 - step;
#pragma unroll
    for (int ci = 0; ci < XS; ++ci) {
      const int c = xchunk(ci);
#pragma unroll
      for (int ld = 0; ld < NLD; ++ld) {
        const int hl = STACK ? (r16 >= RG ? 1 : 0) : ld;
        const int row = STACK ? r16 - hl * RG : r16;
        const int b = b0 + row;
        const bool ok = fuse && c < p.KCM && row < RG && r16 < 2 * RG && b < p.B && step < p.T;
        xf[ci][ld] = __builtin_amdgcn_raw_buffer_load_b128(
            rx, ok ? (unsigned)((((long)(t * p.B + b) * p.KC0 + c) * 2 + hl) * 64 + (lane >> 4) * 16) : 0x7ffffff0u, 0, 0);
      }
    }
  };
  u32x4 xbuf[XS][NLD];                              // ONE set: a step's fragments are consumed before its barrier and re-loaded after it
  if constexpr (FUSE) load_x(xbuf, 0);
  // EARLYX (stacked forms, B <= 32: the input chunks sit on waves that never own elements): the x products of step t + 1 are
  // formed right after the barrier of step t -- in the window the waves without elements would sleep through -- instead of
  // at the start of step t + 1, where they pushed those waves' second polling pass (and with it the barrier) ~550 clocks back
  constexpr bool EARLYX = FUSE && STACK;
  f32x4 accx[NTA];
#pragma unroll
  for (int nt = 0; nt < NTA; ++nt) accx[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  // lone last input column (in_dim = 32*KCM + 1): w_tail per (element, gate) in registers, x_tail comes through the staged slice
  const bool tail = fuse && p.KCM < p.KC0;
  float wt[EPT][4];
#pragma unroll
  for (int i = 0; i < EPT; ++i)
#pragma unroll
    for (int gt = 0; gt < 4; ++gt)
      wt[i][gt] = (tail && e_ok[i]) ? p.wtail[dir * p.NP + g_off[i] / 4 % p.NP + gt] : 0.0f;
  // ---- which dwords of a fragment this lane checks: all four of the 16 bytes it loads for a chunk carry a tag, unless the
  //      lane's column is empty or the 4-unit word lies in the K padding (k >= Hp: never written, stays zero)
  const bool col_ok = r16 < (STACK ? 2 * RG : RG);    // empty columns of the tile: no traffic, zeros
  constexpr int NCM = F32 ? 4 : 2;             // fp32: word r of a fragment is k = 16 chunk + 4 (lane >> 4) + r
  unsigned cm[CPW][NCM];
#pragma unroll
  for (int i = 0; i < CPW; ++i)
#pragma unroll
    for (int hf = 0; hf < NCM; ++hf)
      cm[i][hf] = (col_ok && (F32 ? 16 * chunk_of(i) + 4 * (lane >> 4) + hf : 32 * chunk_of(i) + 8 * (lane >> 4) + 4 * hf) < p.Hp) ? TAG : 0u;
  int nch = 0;                                 // this wave's k-chunks below KQX
#pragma unroll
  for (int i = 0; i < CPW; ++i) nch += (chunk_of(i) < KQX) ? 1 : 0;
  if (tid < 8) s_done[tid] = 0u;
  if (tid < 4) share_flag[tid] = 0u;
  {   // step 0's slice
    f32x4 gq0[LPT];
    stage_issue(gq0, 0);
    if (wave >= ncw) stage_park(gq0, 0);
  }
  __syncthreads();
  bool gave_up = false;                          // after a timeout nobody waits any more: the launch drains
                                                 // with garbage and the abort word tells the host
  // the loop body exists twice: L2-local accesses (FAST) and placement-independent accesses
  auto run = [&](auto fast_c) {
    constexpr bool FAST = decltype(fast_c)::value;
    constexpr int LD_AUX = FAST ? 16 : 17;       // sc1: bypass L1, served by this XCD's L2 | sc0 sc1: coherent anywhere
    constexpr int ST_AUX = FAST ? ONSSEN_XCD_ST_AUX : 17;   // hand-off stores: L2-local | sc0 sc1 write-through
    u32x4 a[CPW][NLD];                           // this wave's chunks of h_{t-1}: requested at the END of the step before
    if (ONSSEN_XCD_SKIP_OOR) {                   // slots that are never loaded hold zeros (their tag masks are empty, their products skipped)
#pragma unroll
      for (int i = 0; i < CPW; ++i)
#pragma unroll
        for (int ld = 0; ld < NLD; ++ld) a[i][ld] = u32x4{0u, 0u, 0u, 0u};
    }
    auto fetch = [&](int i, int step) {          // chunk i of what step `step` multiplies (written by step-1 into slot (step-1)&1)
      const __amdgpu_buffer_rsrc_t rh = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(p.hx + hx_group + (long)((step - 1) & 1) * p.KQ2 * 1024), 0, KQX * CHB, 0x00020000);
#pragma unroll
      for (int ld = 0; ld < NLD; ++ld)       // chunks past KQX are out of range (never branch around a load: the compiler counts them)
        a[i][ld] = __builtin_amdgcn_raw_buffer_load_b128(
            rh, (col_ok && !(ABL & 1)) ? (unsigned)(chunk_of(i) * CHB + ld * 1024 + lane * 16) : 0x7ffffff0u, 0, LD_AUX);
    };
    auto fetch_all = [&](int step) {
      if (step < p.T && !(ABL & 4) && poller) {
#pragma unroll
        for (int i = 0; i < CPW; ++i)
          if (!ONSSEN_XCD_SKIP_OOR || PAIRED || i < nch) fetch(i, step);
      }
    };
    // x_t W_ih^T of the fused first layer for this wave's input chunk(s), accumulated into dst (xbuf holds the fragments)
    auto x_mfma = [&](f32x4 (&dst)[NTA]) __attribute__((always_inline)) {
    if constexpr (FUSE) {
#pragma unroll
      for (int ci = 0; ci < XS; ++ci)
        if (xchunk(ci) < p.KCM) {
          // the W_ih fragments of a chunk pass through registers two tiles at a time (all NT x NHL at once are 40
          // VGPRs on top of the resident W_hh: the 16-row instantiation spilled 9 of them to scratch in every step);
          // per accumulator the order of the terms is the one chunk_mfma uses (small terms first): same bits
          const s16x8 ah = __builtin_bit_cast(s16x8, xbuf[ci][0]), al = __builtin_bit_cast(s16x8, xbuf[ci][NLD - 1]);
          constexpr int NTX = NT > 2 ? 2 : NT;   // tiles per batch of W_ih fragments
#pragma unroll
          for (int n0 = 0; n0 < NT; n0 += NTX) {
            s16x8 wxf[NTX][NHL];
#pragma unroll
            for (int k = 0; k < NTX; ++k)
#pragma unroll
              for (int hl = 0; hl < NHL; ++hl)
                if (n0 + k < NT)
                  wxf[k][hl] = *reinterpret_cast<const s16x8*>(wx_s + ((xchunk(ci) * NT + n0 + k) * NHL + hl) * 512 + lane * 8);
            if constexpr (TERMS == 3 && STACK) {
#pragma unroll
              for (int k = 0; k < NTX; ++k) if (n0 + k < NT) dst[n0 + k] = mfma_bf16(wxf[k][NHL - 1], ah, dst[n0 + k]);
#pragma unroll
              for (int k = 0; k < NTX; ++k) if (n0 + k < NT) dst[n0 + k] = mfma_bf16(wxf[k][0], ah, dst[n0 + k]);
            } else if constexpr (TERMS == 3) {
#pragma unroll
              for (int k = 0; k < NTX; ++k) if (n0 + k < NT) dst[n0 + k] = mfma_bf16(wxf[k][0], al, dst[n0 + k]);
#pragma unroll
              for (int k = 0; k < NTX; ++k) if (n0 + k < NT) dst[n0 + k] = mfma_bf16(wxf[k][NHL - 1], ah, dst[n0 + k]);
#pragma unroll
              for (int k = 0; k < NTX; ++k) if (n0 + k < NT) dst[n0 + k] = mfma_bf16(wxf[k][0], ah, dst[n0 + k]);
            } else {
#pragma unroll
              for (int k = 0; k < NTX; ++k) if (n0 + k < NT) dst[n0 + k] = mfma_bf16(wxf[k][0], ah, dst[n0 + k]);
            }
          }
        }
    }
    };
    // one time step; `xbuf` holds this step's input fragments (fused first layer) until the barrier, the next step's after it
    auto body = [&](int step) {
      const int t = dir == 0 ? step : p.T - 1 - step;
      char* partb = part_s + (step & 1) * (NKP * NT * PTS);
      if constexpr (PROF) if (wave == 0) mark(step, 0);
      f32x4 acc[NTA];
      f32x4 gq[LPT];                            // the loader waves' staged slice of the next step's input projection
#pragma unroll
      for (int nt = 0; nt < NTA; ++nt) acc[nt] = EARLYX ? accx[nt] : f32x4{0.f, 0.f, 0.f, 0.f};
      // the products of one k-chunk: A = weight fragments (rows = 4 units x 4 gates), B = activation fragments (columns =
      // batch rows, or hi | lo halves of <= 8 rows when stacked); term-major, small terms first
      auto chunk_mfma = [&](auto ntc, const s16x8 (&wf)[NTA][NHL], const u32x4 (&af)[NLD]) {
        constexpr int NTC = decltype(ntc)::value;   // gate tiles multiplied by this wave (PAIRED: NTA or NT - NTA)
        const s16x8 ah = __builtin_bit_cast(s16x8, af[0]), al = __builtin_bit_cast(s16x8, af[NLD - 1]);
        if constexpr (F32) {                     // four exact-fp32 MFMA steps (k = 4 each) per fragment, tiles interleaved
          const f32x4 hf = __builtin_bit_cast(f32x4, af[0]);
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int nt = 0; nt < NTC; ++nt)
              acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_bit_cast(f32x4, wf[nt][0])[r], hf[r], acc[nt], 0, 0, 0);
        } else if constexpr (TERMS == 3 && STACK) {
#pragma unroll
          for (int nt = 0; nt < NTC; ++nt) acc[nt] = mfma_bf16(wf[nt][NHL - 1], ah, acc[nt]);   // (hi | lo) x W_lo
#pragma unroll
          for (int nt = 0; nt < NTC; ++nt) acc[nt] = mfma_bf16(wf[nt][0], ah, acc[nt]);         // (hi | lo) x W_hi
        } else if constexpr (TERMS == 3) {
#pragma unroll
          for (int nt = 0; nt < NTC; ++nt) acc[nt] = mfma_bf16(wf[nt][0], al, acc[nt]);
#pragma unroll
          for (int nt = 0; nt < NTC; ++nt) acc[nt] = mfma_bf16(wf[nt][NHL - 1], ah, acc[nt]);
#pragma unroll
          for (int nt = 0; nt < NTC; ++nt) acc[nt] = mfma_bf16(wf[nt][0], ah, acc[nt]);
        } else {
#pragma unroll
          for (int nt = 0; nt < NTC; ++nt) acc[nt] = mfma_bf16(wf[nt][0], ah, acc[nt]);
        }
      };
      // the same products tile GROUP by group (ONSSEN_XCD_TILE_GROUPS): for the tiles [t0, t1) every chunk's terms in chunk_mfma's order
      // (per accumulator: chunk 0's small term, its large term, chunk 1's ...), the group's partial sums stored behind the FIRST chunk
      // of the next group -- an in-order wave that reaches a ds_write waits for the accumulator it stores, so the store must not sit
      // right behind its own MFMAs
      auto group_terms = [&](int i, int t0, int t1) __attribute__((always_inline)) {
        const s16x8 ah = __builtin_bit_cast(s16x8, a[i][0]), al = __builtin_bit_cast(s16x8, a[i][NLD - 1]);
        if constexpr (TERMS == 3 && STACK) {
#pragma unroll
          for (int nt = 0; nt < NTA; ++nt) if (nt >= t0 && nt < t1) acc[nt] = mfma_bf16(w[i][nt][NHL - 1], ah, acc[nt]);
#pragma unroll
          for (int nt = 0; nt < NTA; ++nt) if (nt >= t0 && nt < t1) acc[nt] = mfma_bf16(w[i][nt][0], ah, acc[nt]);
        } else if constexpr (TERMS == 3) {
#pragma unroll
          for (int nt = 0; nt < NTA; ++nt) if (nt >= t0 && nt < t1) acc[nt] = mfma_bf16(w[i][nt][0], al, acc[nt]);
#pragma unroll
          for (int nt = 0; nt < NTA; ++nt) if (nt >= t0 && nt < t1) acc[nt] = mfma_bf16(w[i][nt][NHL - 1], ah, acc[nt]);
#pragma unroll
          for (int nt = 0; nt < NTA; ++nt) if (nt >= t0 && nt < t1) acc[nt] = mfma_bf16(w[i][nt][0], ah, acc[nt]);
        } else {
#pragma unroll
          for (int nt = 0; nt < NTA; ++nt) if (nt >= t0 && nt < t1) acc[nt] = mfma_bf16(w[i][nt][0], ah, acc[nt]);
        }
      };
      auto store_tiles = [&](int t0, int t1) __attribute__((always_inline)) {
#pragma unroll
        for (int nt = 0; nt < NTA; ++nt)
          if (nt >= t0 && nt < t1)
            *reinterpret_cast<f32x4*>(partb + (wave * NT + nt) * PTS + (lane >> 4) * PBS + r16 * 16) = acc[nt];
      };
      auto tile_groups = [&](auto full_c, int nchunks) __attribute__((always_inline)) {
        constexpr bool FULL = decltype(full_c)::value;       // every chunk slot of this wave is live: no branch per chunk
        if constexpr (GROUPED) {
          int pt0 = 0, pt1 = 0;                          // the group whose partial sums are still to be stored
#pragma unroll
          for (int gi = 0, t0 = 0; gi < NGRP; ++gi) {
            const int t1 = t0 + tile_group_size(gi);
            if (FULL || 0 < nchunks) group_terms(0, t0, t1);
            __builtin_amdgcn_sched_barrier(0);
            store_tiles(pt0, pt1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 1; i < CPW; ++i)
              if (FULL || i < nchunks) group_terms(i, t0, t1);
            pt0 = t0; pt1 = t1; t0 = t1;
          }
          __builtin_amdgcn_sched_barrier(0);
          store_tiles(pt0, pt1);
        }
      };
      if constexpr (FUSE && !EARLYX) x_mfma(acc);   // independent of the exchange -- issued BEFORE the wait for h, the MFMAs run under it
      if (!(ABL & 4)) {
        // (step 0 polls like every other step: it waits for tag 0 in slot 1 -- the zeros every member wrote before the
        //  start-up barrier -- and multiplies h_{-1} = 0)
        // ---- poll the data: a pass checks every dword of this wave's chunks; if one is still old, ALL chunks are loaded
        //      again (one L2 round trip per pass) -- then the chunks are multiplied in their fixed order (the accumulation
        //      order decides the last bits of the sum).  The first pass was requested at the end of the step before.
        const unsigned tg = ((((unsigned)(step - 1) >> 1) & 1u) ^ 1u) ? 0xffffffffu : 0u;   // all ones when the expected tag is 1
        unsigned spins = 0;
        if constexpr (PAIRED) {
          if (!poller) {     // the partner polls: wait for its checked fragments in the LDS (bounded like every wait)
            for (unsigned sp = 0; sp < 4000000u; ++sp) {
              if (__hip_atomic_load(&share_flag[pp], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= (unsigned)(step + 1)) break;
              __builtin_amdgcn_s_sleep(1);
            }
#pragma unroll
            for (int i = 0; i < CPW; ++i)
#pragma unroll
              for (int ld = 0; ld < NLD; ++ld) a[i][ld] = share_s[((pp * CPW + i) * NLD + ld) * 64 + lane];
          }
        }
        for (; poller;) {
          unsigned bad = 0u;
#pragma unroll
          for (int i = 0; i < CPW; ++i) {            // (a chunk past KQ2 read zeros and has an empty mask: no branch around it)
#pragma unroll
            for (int ld = 0; ld < NLD; ++ld) {
              if constexpr (F32) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                  a[i][ld][r] ^= cm[i][r] & tg;
                  bad |= a[i][ld][r] & cm[i][r];
                }
              } else {
                a[i][ld][0] ^= cm[i][0] & tg;            // a dword of this step has its tag cleared by this ...
                a[i][ld][1] ^= cm[i][0] & tg;
                a[i][ld][2] ^= cm[i][1] & tg;
                a[i][ld][3] ^= cm[i][1] & tg;
                bad |= ((a[i][ld][0] | a[i][ld][1]) & cm[i][0]) | ((a[i][ld][2] | a[i][ld][3]) & cm[i][1]);   // ... an older one ends up with bit 14 set
              }
            }
          }
          if (__all(bad == 0u) || gave_up || (ABL & 1)) break;
          if (!FAST) __builtin_amdgcn_s_sleep(1);
          if ((++spins & 63u) == 0 &&
              (spins > p.spin_limit || __hip_atomic_load(abort_w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
            if (lane == 0) __hip_atomic_store(abort_w, 2u + (unsigned)step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            gave_up = true;
          }
#pragma unroll
          for (int i = 0; i < CPW; ++i)
            if (!ONSSEN_XCD_SKIP_OOR || PAIRED || i < nch) fetch(i, step);
        }
        if constexpr (PROF) if (wave == 0) mark(step, 8);
        if constexpr (PROF) if (wave == NW - 1) mark(step, 10);
        if (ONSSEN_XCD_GEARLY && wave >= ncw) stage_issue(gq, step + 1);   // (see ONSSEN_XCD_GEARLY: a whole MFMA phase + cell update to arrive in)
        if constexpr (PAIRED) {
          if (poller) {      // hand the checked (tags cleared) fragments to the partner, then multiply the first NTA tiles
#pragma unroll
            for (int i = 0; i < CPW; ++i)
#pragma unroll
              for (int ld = 0; ld < NLD; ++ld) share_s[((pp * CPW + i) * NLD + ld) * 64 + lane] = a[i][ld];
            __builtin_amdgcn_wave_barrier();     // (a wave's LDS operations are performed in order: the flag follows the data)
            if (lane == 0) __hip_atomic_store(&share_flag[pp], (unsigned)(step + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
            for (int i = 0; i < CPW; ++i)
              if (i < nch) chunk_mfma(std::integral_constant<int, NTA>{}, w[i], a[i]);
          } else {
#pragma unroll
            for (int i = 0; i < CPW; ++i)
              if (i < nch) chunk_mfma(std::integral_constant<int, NT - NTA>{}, w[i], a[i]);
          }
        } else if (GROUPED) {                  // tile groups: see ONSSEN_XCD_TILE_GROUPS (the partial sums of a group are written below,
          if (nch == CPW) tile_groups(std::true_type{}, CPW); else tile_groups(std::false_type{}, nch);   // interleaved with the next group's products)
        } else if (nch == CPW) {               // the usual case: one branch instead of one per chunk
#pragma unroll
          for (int i = 0; i < CPW; ++i) chunk_mfma(std::integral_constant<int, NT>{}, w[i], a[i]);
        } else {
#pragma unroll
          for (int i = 0; i < CPW; ++i)
            if (i < nch) chunk_mfma(std::integral_constant<int, NT>{}, w[i], a[i]);
        }
        if constexpr (PROF)
          if (stamp && (unsigned)(step - ST0) < (unsigned)STN && (wave == 0 || wave == NW - 1)) stamp_s[(step - ST0) * 24 + (wave == 0 ? 15 : 14)] = (long long)spins + 1;
        if constexpr (PROF) if (wave == NW - 1) mark(step, 11);
        if constexpr (PROF)
          if (stamp && (unsigned)(step - ST0) < (unsigned)STN && (wave == 0 || wave == NW - 1)) stamp_s[(step - ST0) * 24 + (wave == 0 ? 15 : 14)] = (long long)spins + 1;
      }
      if constexpr (PROF) if (wave == 0) mark(step, 7);
      if constexpr (!GROUPED) {
#pragma unroll
      for (int nt = 0; nt < NTA; ++nt)
        if (!PAIRED || nt < ntw)
          *reinterpret_cast<f32x4*>(partb + ((PAIRED ? pp : wave) * NT + tb + nt) * PTS + (lane >> 4) * PBS + r16 * 16) = acc[nt];
      }
      if constexpr (PROF) if (wave == 0) mark(step, 2);
      __syncthreads();
      if constexpr (PROF) if (wave == 0) mark(step, 3);
      if constexpr (FUSE && !EARLYX) load_x(xbuf, step + 1);
      if (!ONSSEN_XCD_GEARLY && wave >= ncw) stage_issue(gq, step + 1);     // next step's input projection: under the cell update of the other waves

      // ---- fused cell update; publish h_t (tagged split-bf16 fragment image for the group, x3 image for the next GEMM)
      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(p.hx + hx_group + (long)(step & 1) * p.KQ2 * 1024), 0, KQX * CHB, 0x00020000);
      const unsigned mytag = ((((unsigned)step >> 1) & 1u) ^ 1u) ? TAG : 0u;
      float keep_h[EPT];
      u32x2 keep_img[EPT];
      float keep_g[SAVE ? EPT : 1][4];
      if (wave < ncw) {
        if (CELL_PRIO) __builtin_amdgcn_s_setprio(CELL_PRIO);
#pragma unroll
        for (int i = 0; i < EPT; ++i) {
          float h = 0.0f;
          {   // every lane of a wave with elements computes (lanes past the tile read in-range LDS and store out of range)
            // wave partials of all four gates (x 2 when the hi and lo halves of the row sit in different columns): 16-byte LDS
            // reads, two batches of NW/2 waves (all at once would need 64 registers on top of the resident weights)
#ifdef ONSSEN_XCD_NOSTAGE
            const f32x4 gin = *reinterpret_cast<const f32x4*>(p.G + (long)t * g_step + g_off[i] / 4);
#else
            const f32x4 gin = *reinterpret_cast<const f32x4*>(gbuf_s + ((step & 1) * NE + tid + NTHR * i) * 4);
#endif
            f32x4 sum;
#if ONSSEN_XCD_LDS_BATCH1
            if constexpr (STACK && NKP == 8 && !FUSE && !SAVE && NT <= 5) {   // all 16 reads in flight at once (64 registers; NT = 6 has none to spare)
              f32x4 pa[8], pb[8];
#pragma unroll
              for (int wv = 0; wv < 8; ++wv) {
                const char* src = partb + wv * NT * PTS + red_off[i];
                pa[wv] = (ABL & 64) ? f32x4{0.f, 0.f, 0.f, 0.f} : *reinterpret_cast<const f32x4*>(src);
                pb[wv] = (ABL & 64) ? f32x4{0.f, 0.f, 0.f, 0.f} : *reinterpret_cast<const f32x4*>(src + RG * 16);
              }
              asm volatile("" : "+v"(pa[0]), "+v"(pa[1]), "+v"(pa[2]), "+v"(pa[3]), "+v"(pa[4]), "+v"(pa[5]), "+v"(pa[6]), "+v"(pa[7]));
              asm volatile("" : "+v"(pb[0]), "+v"(pb[1]), "+v"(pb[2]), "+v"(pb[3]), "+v"(pb[4]), "+v"(pb[5]), "+v"(pb[6]), "+v"(pb[7]));
#pragma unroll
              for (int wv = 0; wv < 8; ++wv) pa[wv] += pb[wv];
              sum = ((pa[0] + pa[1]) + (pa[2] + pa[3])) + ((pa[4] + pa[5]) + (pa[6] + pa[7]));
            } else if constexpr (ONSSEN_XCD_LDS_BATCH1U && !STACK && TERMS == 3 && NKP == 8 && !FUSE && !SAVE && NT <= 5) {
              // the unstacked 16-row tile (the pair launch of the pipelined step): its 8 reads in one batch too, same summation order
              f32x4 pa[8];
#pragma unroll
              for (int wv = 0; wv < 8; ++wv)
                pa[wv] = (ABL & 64) ? f32x4{0.f, 0.f, 0.f, 0.f} : *reinterpret_cast<const f32x4*>(partb + wv * NT * PTS + red_off[i]);
              asm volatile("" : "+v"(pa[0]), "+v"(pa[1]), "+v"(pa[2]), "+v"(pa[3]), "+v"(pa[4]), "+v"(pa[5]), "+v"(pa[6]), "+v"(pa[7]));
              sum = ((pa[0] + pa[1]) + (pa[2] + pa[3])) + ((pa[4] + pa[5]) + (pa[6] + pa[7]));
            } else
#endif
#pragma unroll
            for (int hb = 0; hb < 2; ++hb) {
              f32x4 part[NKP / 2], part2[STACK ? NKP / 2 : 1];
#pragma unroll
              for (int wv = 0; wv < NKP / 2; ++wv) {
                const char* src = partb + (hb * (NKP / 2) + wv) * NT * PTS + red_off[i];
                part[wv] = (ABL & 64) ? f32x4{0.f, 0.f, 0.f, 0.f} : *reinterpret_cast<const f32x4*>(src);
                if constexpr (STACK) part2[wv] = (ABL & 64) ? f32x4{0.f, 0.f, 0.f, 0.f} : *reinterpret_cast<const f32x4*>(src + RG * 16);
              }
              if constexpr (STACK) {
#pragma unroll
                for (int wv = 0; wv < NKP / 2; ++wv) part[wv] += part2[wv];
              }
              const f32x4 hs = NKP == 8 ? (part[0] + part[1]) + (part[NKP / 2 - 2] + part[NKP / 2 - 1]) : part[0] + part[1];
              sum = hb == 0 ? hs : sum + hs;
            }
            if constexpr (PROF) if (wave == 0) { asm volatile("" :: "v"(sum[0]), "v"(sum[3]), "v"(gin[0])); mark(step, 16); }
            float pre[4];
#pragma unroll
            for (int gt = 0; gt < 4; ++gt) {
              const float sg = sum[gt];
              if constexpr (FUSE) pre[gt] = sg + bgate[i][gt] + gin[0] * wt[i][gt];
              else pre[gt] = sg + gin[gt];
            }
            float ig, fg2, gg, og, cn;
            if (ABL & 128) { ig = pre[0]; fg2 = pre[1]; gg = pre[2]; og = pre[3]; cn = fg2 * cst[i] + ig * gg; h = e_inb[i] ? 0.001f * og * cn : 0.0f; }
            else {
            ig = gate_sigmoid(pre[0]), fg2 = gate_sigmoid(pre[1]), gg = gate_tanh(pre[2]), og = gate_sigmoid(pre[3]);
            cn = fg2 * cst[i] + ig * gg;
            if constexpr (RAGGED) {                     // outside its own frames a row holds h = c = 0 (selects: a NaN of the padding dies here)
              const bool on = t < tlen[i];
              h = on ? og * gate_tanh(cn) : 0.0f;
              cn = on ? cn : 0.0f;
            } else
            h = e_inb[i] ? og * gate_tanh(cn) : 0.0f;   // rows past B carry zeros through the exchange
            }
            cst[i] = cn;
            if constexpr (PROF) if (wave == 0) { asm volatile("" :: "v"(h)); mark(step, 17); }
            const bool nonfin = !(__builtin_fabsf(h) < 2.0f);   // NaN: cannot carry a tag (bit 14 is part of its exponent)
            h = nonfin ? 0.0f : h;
            seen_nonfinite |= nonfin && e_ok[i];                            // reported once, when the launch ends (no branch, no store in the step)
            if constexpr (SAVE) { keep_g[i][0] = ig; keep_g[i][1] = fg2; keep_g[i][2] = gg; keep_g[i][3] = og; }
          }
          keep_h[i] = h;
          // quad gather (all lanes take part: whole quads share e_ok): lanes 0 / 2 assemble the four hi halves, 1 / 3 the lo halves
          unsigned short hi, lo;
          split_bf16(h, hi, lo);
          const unsigned hl = (unsigned)hi | ((unsigned)lo << 16);
          const unsigned q0 = quad_bcast<0>(hl), q1 = quad_bcast<1>(hl), q2 = quad_bcast<2>(hl), q3 = quad_bcast<3>(hl);
          u32x2 v;                                   // one byte permute each: lanes 0 / 2 take the low halves of the pair, 1 / 3 the high halves
          v[0] = __builtin_amdgcn_perm(q1, q0, qsel);
          v[1] = __builtin_amdgcn_perm(q3, q2, qsel);
          keep_img[i] = v;
          v[0] |= mytag;                      // one tag per DWORD: the unit the memory system never tears
          v[1] |= mytag;
          if constexpr (PROF) if (wave == 0) { asm volatile("" :: "v"(v[0]), "v"(v[1])); mark(step, 18); }
          if constexpr (F32) {                 // the exact-fp32 hand-off: this lane's own word, tagged in bit 30
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, h) | mytag, rs, hx_off[i], 0, ST_AUX);
          } else {
#ifdef ONSSEN_XCD_EXP_ATOMIC
          // experiment (round 3): the hand-off as a returnless 64-bit atomic exchange executed AT the L2 instead of a store that
          // passes through the L1's write path -- does the data become visible to the pollers sooner?  (profiles/r03_*: no)
          if (FAST) {
            if (hx_off[i] != 0x7ffffff0u) {
              unsigned long long* dst = reinterpret_cast<unsigned long long*>(
                  reinterpret_cast<char*>(p.hx + hx_group + (long)(step & 1) * p.KQ2 * 1024) + hx_off[i]);
              (void)__hip_atomic_exchange(dst, ((unsigned long long)v[1] << 32) | (unsigned long long)v[0], __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_WORKGROUP);
            }
          } else
#endif
          __builtin_amdgcn_raw_buffer_store_b64(v, rs, hx_off[i], 0, ST_AUX);
          }
          if constexpr (PROF) if (wave == 0) mark(step, 19);
#ifdef ONSSEN_XCD_EXP_STOREACK
          __builtin_amdgcn_s_waitcnt(0x0F70);          // experiment: how long until the hand-off store is acknowledged?
          if constexpr (PROF) if (wave == 0) mark(step, 20);
#endif
        }
        // tell the waves without elements that this member's h is on its way (the other members run in step with it)
        if (lane == 0) __hip_atomic_fetch_add(&s_done[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (ONSSEN_XCD_REQ_EARLY) fetch_all(step + 1);
        if (CELL_PRIO) __builtin_amdgcn_s_setprio(0);
        if constexpr (PROF) if (wave == 1) mark(step, 13);
        if constexpr (PROF) if (wave == 2) mark(step, 1);
        // the layer's OUTPUT (fp32 rows for the caller, x3 image for the next GEMM) is nobody's business inside this launch
        // one buffer resource per output and step (scalar arithmetic), 32-bit lane offsets
        const __amdgpu_buffer_rsrc_t ri = __builtin_amdgcn_make_buffer_rsrc((void*)(yimg_base + t * i_step), 0, yimg_bytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void*)(y_base + t * y_step), 0, y_bytes, 0x00020000);
#pragma unroll
        for (int i = 0; i < EPT; ++i) {
          __builtin_amdgcn_raw_buffer_store_b64(keep_img[i], ri, i_off[i], 0, 0);
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, keep_h[i]), ry, y_off[i], 0, 0);
          if constexpr (SAVE) {
            const __amdgpu_buffer_rsrc_t rsg = __builtin_amdgcn_make_buffer_rsrc((void*)(p.save_g + t * g_step), 0, (int)(g_step * 4), 0x00020000);
            const __amdgpu_buffer_rsrc_t rsc = __builtin_amdgcn_make_buffer_rsrc((void*)(p.save_c + t * y_step), 0, (int)(y_step * 4), 0x00020000);
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, f32x4{keep_g[i][0], keep_g[i][1], keep_g[i][2], keep_g[i][3]}), rsg, g_off_st[i], 0, 0);
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, cst[i]), rsc, y_off[i], 0, 0);
          }
        }
        if constexpr (PROF) if (wave == 0) mark(step, 4);
        // ---- request the chunks of the next step: a request that arrives before the data costs a whole extra round trip (what
        //      this member has just stored, the others have too: they run in step).  Requesting them BEFORE the output stores
        //      measured slower (1.73 vs 1.69 us per step: the chunks did not arrive earlier, profiles/r02b_xcd_timeline.txt)
        if (DELAY_CELL) __builtin_amdgcn_s_sleep(DELAY_CELL);
        if (!ONSSEN_XCD_REQ_EARLY) fetch_all(step + 1);
        if constexpr (PROF) if (wave == 0) mark(step, 5);
      } else {
        if constexpr (EARLYX) {   // x_{t+1} W_ih^T NOW, while the cell-update waves work and the MFMA pipe is idle: the fragments were
          // requested a step ago, the products wait in accx for the next step's accumulation; then request x_{t+2}
          if (ONSSEN_XCD_EARLYX_SLEEP) __builtin_amdgcn_s_sleep(ONSSEN_XCD_EARLYX_SLEEP);   // (let the cell update's LDS reads go first)
#pragma unroll
          for (int nt = 0; nt < NTA; ++nt) accx[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
          x_mfma(accx);
          load_x(xbuf, step + 2);
        }
        if (step + 1 < p.T) {
          // a wave without elements would otherwise poll the L2 for a whole cell update: it sleeps on the LDS instead
          if constexpr (PROF) if (wave == NW - 1) mark(step, 12);
          for (unsigned spins = 0; spins < 100000u; ++spins) {
            if (__hip_atomic_load(&s_done[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= (unsigned)(ncw * (step + 1))) break;
            __builtin_amdgcn_s_sleep(ONSSEN_XCD_IDLE_SLEEP);
          }
        }
        if (ONSSEN_XCD_FETCH_FIRST) fetch_all(step + 1);
        if (step + 1 < p.T) stage_park(gq, step + 1);
        if (ONSSEN_XCD_DELAY_IDLE) __builtin_amdgcn_s_sleep(ONSSEN_XCD_DELAY_IDLE);
        if (!ONSSEN_XCD_FETCH_FIRST) fetch_all(step + 1);
        if constexpr (PROF) if (wave == NW - 1) mark(step, 9);
      }
    };
    if constexpr (EARLYX) {      // step 0's x products (its fragments were requested above), then request step 1's
      x_mfma(accx);
      load_x(xbuf, 1);
    }
    fetch_all(0);
    for (int step = 0; step < p.T; step += 2) {
      body(step);
      if (step + 1 < p.T) body(step + 1);
    }
  };
  if (fast) run(std::true_type{}); else run(std::false_type{});
  if (seen_nonfinite) __hip_atomic_store(p.sync + 282, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (PROF && p.dbg && blockIdx.x == ONSSEN_XCD_PROFILE_WG) {
    __syncthreads();
    for (int i = tid; i < STN * 24; i += NTHR) p.dbg[i] = stamp_s[i];
  }
}

// calibration probe: a chain of n dependent near-empty launches (measures the launch-boundary floor)
__global__ void probe_kernel(float* p) {
  if (threadIdx.x == 0 && blockIdx.x == 0) p[0] += 1.0f;
}
