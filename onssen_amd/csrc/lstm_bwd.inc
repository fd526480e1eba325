// BLSTM recurrence, backward in time (training; SURVEY row N1): part of onssen_hip.hip.
//
// What autograd does for nn.LSTM inside `loss.backward()` (onssen/utils/train.py:80-84), restated per layer:
//   saved by the forward launch (lstm_xcd_kernel<SAVE>): the gate activations (i, f, g, o)_t in the slots of the
//   input projection G they were computed from, and the cell states c_t.
//   step (dir 0 walks t = T-1 .. 0, dir 1 walks t = 0 .. T-1 -- each direction against its own forward order):
//     dh    = dy_t + dP_next W_hh                  (dP_next = this kernel's output of the step before)
//     dc    = dc_carry + dh o (1 - tanh^2 c_t)
//     dP_t  = [dc g i(1-i), dc c_prev f(1-f), dc i (1-g^2), dh tanh(c_t) o(1-o)]      (pre-activation gradient)
//     dc_carry = dc f
//   dP overwrites the saved gates in place (fp32, the operand of the weight-gradient GEMMs) and is handed to the next
//   step as a split-bf16 A-fragment image, like h in the forward kernels.  The product dP_next W_hh has K = 4H: the
//   workgroup of 16 hidden units keeps no weights resident here (launch per step) and streams its [4Hp x 16] slice
//   of W_hh (B-fragment image, split bf16) from L2 every step.

// B-fragment image of W_hh for the backward product: [dir-less][ub][q][hi|lo][lane][8],
//   n = lane & 15 -> hidden unit j = 16 ub + n;  k = 32 q + 8 (lane >> 4) + i -> packed gate column of the forward
//   layout (k = ugi*4*UG + ju*4 + gate  <->  nn.LSTM row gate*H + ugi*UG + ju)
__global__ void pack_whhT_bf16x3_kernel(const float* __restrict__ w_hh, int H, int Hp, int UG, int KQB, int NUB,
                                        unsigned short* __restrict__ out) {
  const long total = (long)NUB * KQB * 512;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int i = (int)(e & 7), lane = (int)((e >> 3) & 63);
    const long rest = e >> 9;
    const int q = (int)(rest % KQB), ub = (int)(rest / KQB);
    const int j = ub * 16 + (lane & 15);
    const int k = 32 * q + 8 * (lane >> 4) + i;
    const int ugi = k / (4 * UG), rem = k % (4 * UG), ju = rem >> 2, gate = rem & 3;
    const int u = ugi * UG + ju;
    const float v = (k < 4 * Hp && u < H && j < H) ? w_hh[(long)(gate * H + u) * H + j] : 0.0f;
    unsigned short hi, lo;
    split_bf16(v, hi, lo);
    const long base = ((long)(ub * KQB + q) * 2) * 512 + lane * 8 + i;
    out[base] = hi;
    out[base + 512] = lo;
  }
}

struct BwdArgs {
  float* gd = nullptr;                 // [T][B][2][NP]  in: saved gate activations; out: dL/d(pre-activation), same slots
  const float* cs = nullptr;           // [T][B][2][Hp]  cell states
  const float* dy = nullptr;           // [T][B][2][Hp]  gradient w.r.t. the layer output
  const unsigned short* wT = nullptr;  // [2][NUB][KQB][hi|lo][64][8]
  unsigned short* ds = nullptr;        // hand-off images [2 slots][2 dirs][nmt][KQB][hi|lo][64][8]
  float* dc = nullptr;                 // [2][B][Hp] carried dL/dc
  int B = 0, T = 0, Hp = 0, NP = 0, UG = 0, KQB = 0, NUB = 0, step = 0;
};

namespace recb {
constexpr int QB = 5;      // k-chunks (32 k) a wave keeps in flight
constexpr int NW = 16;     // waves per workgroup: K = 4Hp <= 2560 is split 16 ways, so that ALL of a step's operand
                           // fetches (QB chunks per wave) are in flight at once -- four dependent batches of L2 latency
                           // per step (4 waves) measured 8.0 us per launch
}

__global__ __launch_bounds__(64 * recb::NW) void lstm_bwd_step_kernel(BwdArgs p) {
  using namespace rec;
  constexpr int NW = recb::NW;
  __shared__ float red[NW * 4 * RLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ub = blockIdx.x, dir = blockIdx.y, b0 = blockIdx.z * 16;
  const int t = dir == 0 ? p.T - 1 - p.step : p.step;
  const int tprev = dir == 0 ? t - 1 : t + 1;          // the step BEFORE t in this direction's forward order
  const bool first = p.step == 0;
  const int nmt = (p.B + 15) >> 4;
  const long sdir = (long)nmt * p.KQB * 1024;           // uint16 elements per (slot, direction)
  constexpr unsigned kOOB = 0x7ffffff0u;

  // ---- one (batch row, hidden unit) per thread of the first four waves; its saved state does not depend on the
  //      recurrent product, so these loads are issued first and complete under the operand fetches
  const int row = (tid >> 4) & 15, n = tid & 15, b = b0 + row, j = ub * 16 + n;
  const bool mine = tid < 256 && b < p.B && j < p.Hp;
  const int col = (j / p.UG) * 4 * p.UG + (j % p.UG) * 4;
  float4* gp = reinterpret_cast<float4*>(p.gd + ((long)(t * p.B + b) * 2 + dir) * p.NP + col);
  float* dcp = p.dc + ((long)dir * p.B + b) * p.Hp + j;
  float4 gt = make_float4(0.f, 0.f, 0.f, 0.f);
  float ct = 0.f, cprev = 0.f, dh = 0.f, dcin = 0.f;
  if (mine) {
    gt = *gp;                                               // i, f, g, o
    ct = p.cs[((long)(t * p.B + b) * 2 + dir) * p.Hp + j];
    if (tprev >= 0 && tprev < p.T) cprev = p.cs[((long)(tprev * p.B + b) * 2 + dir) * p.Hp + j];
    dh = p.dy[((long)(t * p.B + b) * 2 + dir) * p.Hp + j];
    if (!first) dcin = *dcp;
  }

  if (!first) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(p.wT + (long)(dir * p.NUB + ub) * p.KQB * 1024), 0, p.KQB * 2048, 0x00020000);
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(p.ds + ((long)((p.step - 1) & 1) * 2 + dir) * sdir + (long)(b0 >> 4) * p.KQB * 1024), 0, p.KQB * 2048,
        0x00020000);
    for (int qb = 0; qb < p.KQB; qb += NW * recb::QB) {
      u32x4 a[recb::QB][2], w[recb::QB][2];
#pragma unroll
      for (int i = 0; i < recb::QB; ++i) {
        const int q = qb + wave + NW * i;
        const unsigned off = q < p.KQB ? (unsigned)(q * 2048 + lane * 16) : kOOB;
#pragma unroll
        for (int hl = 0; hl < 2; ++hl) {
          a[i][hl] = __builtin_amdgcn_raw_buffer_load_b128(ra, off + hl * 1024, 0, 0);
          w[i][hl] = __builtin_amdgcn_raw_buffer_load_b128(rw, off + hl * 1024, 0, 0);
        }
      }
#pragma unroll
      for (int i = 0; i < recb::QB; ++i) {
        if (qb + wave + NW * i < p.KQB) {
          const s16x8 ah = __builtin_bit_cast(s16x8, a[i][0]), al = __builtin_bit_cast(s16x8, a[i][1]);
          const s16x8 wh = __builtin_bit_cast(s16x8, w[i][0]), wl = __builtin_bit_cast(s16x8, w[i][1]);
          acc = mfma_bf16(al, wh, acc);
          acc = mfma_bf16(ah, wl, acc);
          acc = mfma_bf16(ah, wh, acc);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) red[(wave * 4 + r) * RLD + lane] = acc[r];
    __syncthreads();
  }

  if (mine) {
    if (!first) {
      const int src = ((row >> 2) << 4) + n, r = row & 3;
#pragma unroll
      for (int w = 0; w < NW; ++w) dh += red[(w * 4 + r) * RLD + src];
    }
    const float tc = gate_tanh(ct);
    const float dcv = dcin + dh * gt.w * (1.0f - tc * tc);
    float4 d;
    d.x = dcv * gt.z * gt.x * (1.0f - gt.x);
    d.y = dcv * cprev * gt.y * (1.0f - gt.y);
    d.z = dcv * gt.x * (1.0f - gt.z * gt.z);
    d.w = dh * tc * gt.w * (1.0f - gt.w);
    *dcp = dcv * gt.y;
    *gp = d;
    // hand dP_t to the next step: k = col .. col+3 are consecutive elements of one lane's 8-element fragment row
    unsigned short hi[4], lo[4];
    split_bf16(d.x, hi[0], lo[0]);
    split_bf16(d.y, hi[1], lo[1]);
    split_bf16(d.z, hi[2], lo[2]);
    split_bf16(d.w, hi[3], lo[3]);
    unsigned short* dst = p.ds + (((long)(p.step & 1) * 2 + dir) * nmt + (b >> 4)) * p.KQB * 1024 + (long)(col >> 5) * 1024 +
                          ((b & 15) + 16 * ((col >> 3) & 3)) * 8 + (col & 7);
    *reinterpret_cast<uint2*>(dst) = make_uint2((unsigned)hi[0] | ((unsigned)hi[1] << 16), (unsigned)hi[2] | ((unsigned)hi[3] << 16));
    *reinterpret_cast<uint2*>(dst + 512) = make_uint2((unsigned)lo[0] | ((unsigned)lo[1] << 16), (unsigned)lo[2] | ((unsigned)lo[3] << 16));
  }
}

// -------------------------------------------------------------------------------------------------
// XCD-local persistent form of the backward recurrence: ONE launch runs all T steps of a layer.
//
// Same grouping, placement check and bounded waits as lstm_xcd_kernel (lstm.inc); what moves between the members is
// different.  The product dh = dP W_hh has K = 4H, and a member that owned an output slice would need a [4H x UG]
// weight slice resident AND all of dP every step (4x the forward's exchange).  Instead every member keeps the ROWS of
// W_hh that belong to its own 4*UG gate columns ([4*UG x Hp], split bf16, in registers: 3 k-chunks x 5 unit tiles x
// hi/lo per wave at H = 600) and multiplies them with the dP it has just produced itself -- the A operand never leaves
// the workgroup (LDS).  The result is its CONTRIBUTION to everybody's dh; the exchange is a reduce-scatter of fp32
// partial sums through the XCD's L2: member m stores [dst][m][UG][RG] blocks, and at the next step every member adds up
// the NU blocks addressed to it (fixed order: bitwise reproducible).
//
// Round 2: the exchange carries its own "ready" (as the forward kernel's does).  Bit 0 of every partial sum -- the last
// mantissa bit, 2^-24 relative -- is a TAG that alternates every second step (two slots): a consumer polls the DATA
// until every dword it needs carries the tag of the step it waits for.  No drain of the stores, no flag store, no flag
// poll: one L2 round trip per step where the flag protocol had three.  The producers' own blocks start a launch
// zeroed (tag 0; the first two steps write tag 1) before the group's start-up barrier.
//   * threads 0 .. 319 (waves 0-4) poll: P = 1 / 2 / 4 lanes per element (row, unit) of the member's RG x UG tile, each
//     adding up NU / P source blocks; the lanes of an element sit in one quad and finish the sum with DPP quad
//     permutes -- no LDS pass, no barrier between the poll and the cell arithmetic;
//   * waves 5-7 fetch the saved state of step s+2 (gates, c_t, c_prev, dy_t) after the barrier of step s and park it in
//     the LDS before the barrier of step s+1: vmcnt retires in order, so a prefetch issued by a polling wave would be
//     waited for by its next poll -- an HBM latency on the critical path;
//   * ONE barrier per step (dP fragments in the LDS -> MFMAs of all eight waves).
// -------------------------------------------------------------------------------------------------

// Row-slice image of W_hh for member m: [m][c][nt][hi|lo][lane][8] with
//   n = lane & 15 -> hidden unit j = 16 nt + n;  k_local = 32 c + 8 (lane >> 4) + i = ju*4 + gate of member m's units
__device__ __forceinline__ void pack_whhR_bf16x3_body(const float* __restrict__ w_hh, int H, int Hp, int UG, int KC, int NTB,
                                                      unsigned short* __restrict__ out, long first, long stride) {
  const int NU = Hp / UG;
  const long total = (long)NU * KC * NTB * 64;     // one thread per fragment lane: its 8 gate columns of hidden unit j (8 rows of W_hh)
  for (long e = first; e < total; e += stride) {
    const int lane = (int)(e & 63);
    long rest = e >> 6;
    const int nt = (int)(rest % NTB);
    rest /= NTB;
    const int c = (int)(rest % KC), m = (int)(rest / KC);
    const int j = nt * 16 + (lane & 15);
    const int kl0 = 32 * c + 8 * (lane >> 4);
    unsigned short hi[8], lo[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int kl = kl0 + i, ju = kl >> 2, gate = kl & 3, u = m * UG + ju;
      split_bf16((kl < 4 * UG && u < H && j < H) ? w_hh[(long)(gate * H + u) * H + j] : 0.0f, hi[i], lo[i]);
    }
    u32x4 h4, l4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      h4[i] = (unsigned)hi[2 * i] | ((unsigned)hi[2 * i + 1] << 16);
      l4[i] = (unsigned)lo[2 * i] | ((unsigned)lo[2 * i + 1] << 16);
    }
    const long base = (((long)(m * KC + c) * NTB + nt) * 2) * 512 + lane * 8;
    *reinterpret_cast<u32x4*>(out + base) = h4;
    *reinterpret_cast<u32x4*>(out + base + 512) = l4;
  }
}

__global__ void pack_whhR_bf16x3_kernel(const float* __restrict__ w_hh, int H, int Hp, int UG, int KC, int NTB,
                                        unsigned short* __restrict__ out) {
  pack_whhR_bf16x3_body(w_hh, H, Hp, UG, KC, NTB, out, (long)blockIdx.x * blockDim.x + threadIdx.x, (long)gridDim.x * blockDim.x);
}

// ---- round 5: the training forward re-packs every step (the optimizer moves the weights between two forwards): ALL images of the
// stack -- per (layer, direction): packed W_ih + bias + its x3 image, the W_hh fragment image of the forward recurrence, the W_hh
// row-slice image of the backward recurrence -- in ONE launch instead of 18 (L = 3).  A job is one of the three bodies above on a
// slice of the grid; the results are those of the single-job kernels bit for bit (same device functions).
namespace packt { constexpr int MAXJ = 24; }
struct PackJob {
  const float* w;             // W_ih (type 0) or W_hh (types 1, 2)
  const float* b_ih;
  const float* b_hh;
  float* wih_p;
  float* bias_p;
  unsigned short* out;        // x3 image (0) / whh_x3 (1) / whhR (2)
  int type, in_dim, bidir, Kp, K, KB;
  int first_block, nblocks;
};
struct PackTrainArgs {
  PackJob job[packt::MAXJ];
  int njobs, H, Hp, UG, KQ2, KC, NTB;
};

__global__ __launch_bounds__(256) void lstm_pack_train_kernel(PackTrainArgs a) {
  int j = 0;
#pragma unroll 1
  while (j + 1 < a.njobs && (int)blockIdx.x >= a.job[j + 1].first_block) ++j;
  const PackJob& jb = a.job[j];
  const long first = (long)((int)blockIdx.x - jb.first_block) * 256 + threadIdx.x, stride = (long)jb.nblocks * 256;
  if (jb.type == 0)
    pack_wih_image_body(jb.w, jb.b_ih, jb.b_hh, jb.in_dim, jb.bidir, a.H, a.Hp, a.UG, jb.Kp, jb.K, jb.KB, jb.wih_p, jb.bias_p, jb.out, first, stride);
  else if (jb.type == 1)
    pack_whh_bf16x3_body(jb.w, a.H, a.Hp, a.UG, a.KQ2, a.H, jb.out, first, stride);
  else
    pack_whhR_bf16x3_body(jb.w, a.H, a.Hp, a.UG, a.KC, a.NTB, jb.out, first, stride);
}

#ifndef ONSSEN_BWD_WIDE
#define ONSSEN_BWD_WIDE 1            // 1 = lstm_xcd_bwd_kernel's wide poll (RGW below) is what onssen_lstm_train_backward_* launches
#endif
struct XcdBwdArgs {
  float* gd = nullptr;                 // [T][B][2][NP]  in: saved gate activations; out: dL/d(pre-activation)
  const float* cs = nullptr;           // [T][B][2][Hp]
  const float* dy = nullptr;           // [T][B][2][Hp]
  const unsigned short* wR = nullptr;  // [2][NU][KC][NTB][hi|lo][64][8]
  float* xch = nullptr;                // [8 groups][2 slots][NU dst][NU src][UG][RG] partial sums, bit 0 = tag
  unsigned* sync = nullptr;            // header words as in XcdArgs (own workspace, zeroed once by its owner)
  int B = 0, T = 0, Hp = 0, NP = 0, NU = 0, NTB = 0, RG = 0, row0 = 0, nbg = 0;
  unsigned spin_limit = 0;
  int ablate = 0;                      // test only: 8 = rotate groups over XCDs
  int delay = 0;                       // s_sleep(1) repetitions between a step's stores and the first request for the next step's sums
  long long* dbg = nullptr;            // ONSSEN_XCD_PROFILE builds: 8 timestamps per step of workgroup 0 (tools/bwd_timeline.py), or null
  float* db_rows = nullptr;            // [B][2][NP] sum over t of dL/d(pre-activation) per batch row (the bias gradient is its sum over rows), or null
  unsigned short* dp_img = nullptr;    // (round 5) x3 image [T*B][2*NP/32][2][32] of dP, written INSTEAD of the fp32 dP (the gradient GEMMs' operand), or null
};

// STACK (round 5; groups of <= 8 rows -- the as-shipped B_local = 16 runs 4-row groups): the hi and the lo half of a batch row
// share ONE A tile.  Tile row 4 (row >> 1) + 2 (row & 1) + s holds the hi (s = 0) / lo (s = 1) bf16 half of dP of batch row
// `row`, so that after A x W_hi and A x W_lo into the SAME accumulators a lane holds, for its unit, hi.W + lo.W of rows 2i
// (registers 0 + 1) and 2i + 1 (registers 2 + 3), i = lane >> 4: two MFMAs and one fragment read per (k-chunk, unit tile)
// instead of three and two (with 4-row groups three quarters of the unstacked tiles' rows were zeros), the sum of the two
// halves is an in-lane add, and the product is the full (hi + lo)(W_hi + W_lo) -- the lo.lo term the three-term form drops
// comes for free.  The timeline (profiles/r02b_bwd_timeline.txt) had the MFMAs at 24 % of a step.
// RGW (round 6; 0 = the round-2 poll above, 4 / 8 / 16 = rows per group of this instantiation): the WIDE poll.  The CU's address unit
// takes a wave-level load at ~16 clocks whatever its width (tools/micro/l2_gather_probe.hip), so the round-2 poll -- P lanes per element,
// each with SPS 4-byte loads: 5 waves x 8 / 16 / 32 = 40 / 80 / 160 wave loads per pass -- was instruction-bound (the "poll 24 %" of
// the timeline).  Inside an exchange block the batch row runs fastest, so ONE 16-byte load fetches a unit's four rows from one source:
// 16 lanes per unit, lane (row quad `sub`, part `rp`) loads sources rp, rp + S, ... (S = 64 / RG lanes per row quad) -- 5 waves x 2 / 4 /
// 8 = 10 / 20 / 40 wave loads --, adds them up in that order, the S lanes of a row quad finish the sum with log2(S) DPP row rotations
// (a fixed order per lane), and lane rp < 4 of a quad is the element (row 4 sub + rp).  Same bytes, same tags, a quarter of the requests.
template <int UG, int P, bool STACK, int RGW = 0>
__global__ __launch_bounds__(512) void lstm_xcd_bwd_kernel(XcdBwdArgs p) {
  constexpr int NW = 8, NTHR = 512;
  constexpr int NPOLL = 320;                   // polling threads (waves 0-4); waves 5-7 stage the saved state
  constexpr int NLOAD = NTHR - NPOLL;
  constexpr int EMAX = 16 * UG;                // elements of a member's tile, RG = 16
  constexpr int LPT = (EMAX + NLOAD - 1) / NLOAD;
  constexpr bool WIDE = RGW != 0;
  static_assert(!WIDE || ((RGW == 4 || RGW == 8 || RGW == 16) && UG <= 20), "wide poll: 16 lanes per unit of the 320 polling lanes");
  constexpr int WSUBS = WIDE ? RGW / 4 : 1;    // row quads per unit
  constexpr int WS = 16 / WSUBS;               // lanes (= source residues) per row quad
  constexpr int WNL = (32 + WS - 1) / WS;      // 16-byte loads per polling lane (NU <= 32)
  constexpr int SPS = WIDE ? 4 * WNL : (32 + P - 1) / P;        // dwords per polling lane: source blocks (NU <= 32), x 4 rows when WIDE
  constexpr int KC = (4 * UG + 31) / 32;       // k-chunks of a member's own gate columns
  constexpr int TPW = 5;                       // unit tiles per wave: 8 x 5 x 16 = 640 >= Hp
  constexpr unsigned kOOB = 0x7ffffff0u;
  constexpr bool PROF = ONSSEN_XCD_PROFILE != 0;
  constexpr int ST0 = 64, STN = 64;
  // [step parity][chunk][hi|lo][64][8]: a wave may write the fragments of step s+1 while another still reads those of step s
  // (its poll only proves that the waves holding ITS sources have stored)
  constexpr int AFT = STACK ? 1 : 2;           // A tiles per k-chunk: one stacked tile, or a hi tile and a lo tile
  __shared__ __attribute__((aligned(16))) unsigned short afrag[2 * KC * AFT * 512];
  __shared__ __attribute__((aligned(16))) float stbuf[2 * EMAX * 8];            // [step parity][element][i f g o | c_t c_prev dy -]
  __shared__ unsigned s_ctl[3];
  __shared__ long long stamp_s[PROF ? STN * 8 : 1];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ugi = blockIdx.x >> 3, g = (p.ablate & 8) ? ((blockIdx.x + ugi) & 7) : (blockIdx.x & 7);
  if (g >= 2 * p.nbg) return;
  const int dir = g / p.nbg, bg = g % p.nbg;
  const int RG = p.RG, E = RG * UG;
  const int b0 = p.row0 + bg * RG;
  unsigned* abort_w = p.sync + 280;
  const long slot_elems = (long)p.NU * p.NU * E;
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)(p.xch + (long)g * 2 * slot_elems), 0,
                                                                       (int)(2 * slot_elems * 4), 0x00020000);

  // ---- this member's blocks of both slots start the launch untagged (zero); write-through, because the placement is
  //      not known yet
  for (int i = tid; i < 2 * p.NU * E / 4; i += NTHR) {
    const int q = i * 4, sl = q / (p.NU * E), rem = q % (p.NU * E), md = rem / E, el = rem % E;
    __builtin_amdgcn_raw_buffer_store_b128(u32x4{0u, 0u, 0u, 0u}, rx,
        (unsigned)((sl * slot_elems + ((long)md * p.NU + ugi) * E + el) * 4), 0, 17);
  }
  __builtin_amdgcn_s_waitcnt(0x0F70);   // s_waitcnt vmcnt(0): acknowledged by memory
  __syncthreads();

  // ---- placement check (as lstm_xcd_kernel; also the start-up barrier of the group)
  if (tid == 0) {
    const unsigned xcc = __builtin_amdgcn_s_getreg(6164) & 15u;
    const unsigned gen0 = __hip_atomic_fetch_add(p.sync + 288 + g, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_ctl[2] = gen0;
    unsigned long long* xw = reinterpret_cast<unsigned long long*>(p.sync + 320) + 2 * g;
    __hip_atomic_fetch_max(xw, ((unsigned long long)gen0 << 8) | (xcc + 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(xw + 1, ((unsigned long long)gen0 << 8) | (16u - xcc), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __hip_atomic_fetch_add(p.sync + 256 + g, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned spins = 0, ab = p.spin_limit == 0u ? 1u : 0u;      // a spin limit of 0 aborts at once, whatever the timing (tests)
    while (__hip_atomic_fetch_add(p.sync + 256 + g, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - gen0 * (unsigned)p.NU <
           (unsigned)p.NU) {
      __builtin_amdgcn_s_sleep(8);
      if (++spins > p.spin_limit || __hip_atomic_load(abort_w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { ab = 1; break; }
    }
    const unsigned hi = (unsigned)__hip_atomic_fetch_add(xw, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 255u;
    const unsigned lo = (unsigned)__hip_atomic_fetch_add(xw + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 255u;
    s_ctl[0] = ab;
    s_ctl[1] = (hi + lo == 17u) ? 1u : 0u;
    if (ab) __hip_atomic_store(abort_w, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!ab && s_ctl[1] == 0u) __hip_atomic_store(p.sync + 281, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // everybody has read the generation (they arrive after reading it): the next launch gets a new one
    if (!ab && ugi == 0) __hip_atomic_fetch_add(p.sync + 288 + g, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  }
  for (int i = tid; i < 2 * KC * AFT * 512 / 2; i += NTHR) reinterpret_cast<unsigned*>(afrag)[i] = 0u;   // rows nobody owns, k >= 4 UG stay zero
  __syncthreads();
  if (s_ctl[0]) return;
  const bool fast = s_ctl[1] != 0;

  // ---- resident weights: this member's rows of W_hh, unit tiles wave, wave + 8, ...
  s16x8 w[KC][TPW][2];
  {
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(p.wR + (long)(dir * p.NU + ugi) * KC * p.NTB * 1024), 0, KC * p.NTB * 2048, 0x00020000);
#pragma unroll
    for (int c = 0; c < KC; ++c)
#pragma unroll
      for (int i = 0; i < TPW; ++i)
#pragma unroll
        for (int hl = 0; hl < 2; ++hl) {
          const int nt = wave + NW * i;
          w[c][i][hl] = __builtin_bit_cast(s16x8, __builtin_amdgcn_raw_buffer_load_b128(
              rw, nt < p.NTB ? (unsigned)(((c * p.NTB + nt) * 2 + hl) * 1024 + lane * 16) : kOOB, 0, 0));
        }
  }

  // ---- polling lane (element ex, part r): P lanes of a quad share an element; inside an exchange block the batch row runs
  //      fastest ([ju][RG]): the producer's four rows of one unit are ONE 16-byte store
  const int wsub = (tid & 15) % WSUBS, wrp = (tid & 15) / WSUBS;           // WIDE: row quad and part of this lane within its unit's 16 lanes
  const int ex = WIDE ? (tid >> 4) * RG + 4 * wsub + (wrp & 3) : tid / P, r = WIDE ? wrp : tid % P;
  const bool poller = tid < NPOLL && (WIDE ? (tid >> 4) < UG : ex < E);
  const bool is_el = poller && (WIDE ? wrp < 4 : r == 0);
  const int ju = ex / RG, row = ex % RG, b = b0 + row;
  const bool inb = is_el && b < p.B;
  const long g_off = ((long)b * 2 + dir) * p.NP + ugi * 4 * UG + ju * 4;
  const long g_step = (long)p.B * 2 * p.NP, y_step = (long)p.B * 2 * p.Hp;
  // this element's four gate columns inside a row of the dP image: k = dir * NP + ugi * 4 UG + 4 ju (a multiple of 4: one 8-byte
  // piece of the hi half and one of the lo half of k-block k / 32)
  const int ik = dir * p.NP + ugi * 4 * UG + ju * 4;
  const long i_row = (long)(2 * p.NP / 32) * 64;               // uint16 elements per image row
  const long i_off = (long)b * i_row + (long)(ik >> 5) * 64 + (ik & 31);
  const long i_step = (long)p.B * i_row;
  // source r, r + P, ...: E * P elements apart (WIDE: the four rows 4 wsub .. 4 wsub + 3 of unit ju from source r, r + WS, ...)
  const unsigned lane_base = !poller ? kOOB : WIDE ? (unsigned)((r * E + ju * RG + 4 * wsub) * 4) : (unsigned)((r * E + ex) * 4);
  unsigned vmask = 0u;                          // bit k: source r + P k (WIDE: r + WS k) exists
#pragma unroll
  for (int k = 0; k < (WIDE ? WNL : SPS); ++k) vmask |= (poller && r + (WIDE ? WS : P) * k < p.NU) ? (1u << k) : 0u;
  const int kl = ju * 4;
  const int trow = STACK ? 4 * (row >> 1) + 2 * (row & 1) : row;     // tile row of this element's hi half (STACK: lo in the next row)
  unsigned short* af_dst = afrag + (kl >> 5) * (AFT * 512) + (trow + 16 * ((kl >> 3) & 3)) * 8 + (kl & 7);
  // ---- loader lane: elements lx = tid - NPOLL + NLOAD * k
  constexpr int NREG = SPS > 8 * LPT ? SPS : 8 * LPT;   // a polling lane's partial sums / a loader lane's staged state: same registers
  auto stage_issue = [&](unsigned (&sv)[NREG], int step) {
    const int t = dir == 0 ? p.T - 1 - step : step;
    const int tprev = dir == 0 ? t - 1 : t + 1;
#pragma unroll
    for (int k = 0; k < LPT; ++k) {
      const int lx = tid - NPOLL + NLOAD * k;
      const int lju = lx / RG, lrow = lx % RG, lb = b0 + lrow;
      const bool ok = tid >= NPOLL && lx < E && lb < p.B && step < p.T;
      const long go = ((long)lb * 2 + dir) * p.NP + ugi * 4 * UG + lju * 4, yo = ((long)lb * 2 + dir) * p.Hp + ugi * UG + lju;
#pragma unroll
      for (int q = 0; q < 8; ++q) sv[8 * k + q] = 0u;
      if (ok) {
        const u32x4 gq = *reinterpret_cast<const u32x4*>(p.gd + go + t * g_step);
        sv[8 * k + 0] = gq[0]; sv[8 * k + 1] = gq[1]; sv[8 * k + 2] = gq[2]; sv[8 * k + 3] = gq[3];
        sv[8 * k + 4] = __builtin_bit_cast(unsigned, p.cs[yo + t * y_step]);
        if (tprev >= 0 && tprev < p.T) sv[8 * k + 5] = __builtin_bit_cast(unsigned, p.cs[yo + tprev * y_step]);
        sv[8 * k + 6] = __builtin_bit_cast(unsigned, p.dy[yo + t * y_step]);
      }
    }
  };
  auto stage_park = [&](const unsigned (&sv)[NREG], int step) {
#pragma unroll
    for (int k = 0; k < LPT; ++k) {
      const int lx = tid - NPOLL + NLOAD * k;
      if (tid >= NPOLL && lx < E) {
        unsigned* d = reinterpret_cast<unsigned*>(stbuf) + ((step & 1) * EMAX + lx) * 8;
        *reinterpret_cast<u32x4*>(d) = u32x4{sv[8 * k + 0], sv[8 * k + 1], sv[8 * k + 2], sv[8 * k + 3]};
        *reinterpret_cast<u32x4*>(d + 4) = u32x4{sv[8 * k + 4], sv[8 * k + 5], sv[8 * k + 6], sv[8 * k + 7]};
      }
    }
  };
  {
    unsigned sv[NREG];
    stage_issue(sv, 0); stage_park(sv, 0);
    stage_issue(sv, 1); stage_park(sv, 1);
  }
  __syncthreads();
  const bool stamp = PROF && p.dbg && tid == 0 && blockIdx.x == 0;
  auto mark = [&](int step, int slot) {
    if constexpr (PROF)
      if (stamp && (unsigned)(step - ST0) < (unsigned)STN) stamp_s[(step - ST0) * 8 + slot] = clock64();
  };
  float dcarry = 0.0f;
  float4 dsum = make_float4(0.f, 0.f, 0.f, 0.f);   // sum over the steps of this element's dP: the bias gradient needs no pass over dP
  bool gave_up = false;

  auto run = [&](auto fast_c) {
    constexpr bool FAST = decltype(fast_c)::value;
    constexpr int LD_AUX = FAST ? 16 : 17;       // sc1: served by this XCD's L2 | sc0 sc1: coherent anywhere
    constexpr int ST_AUX = FAST ? 0 : 17;
    unsigned v[NREG];
    auto fetch = [&](int step) {                 // the partial sums step `step` adds up (written by step-1 into slot (step-1)&1)
      // the NU blocks addressed to this member are one buffer: a source past NU is out of range and reads as zero
      const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(p.xch + (long)g * 2 * slot_elems + ((long)((step - 1) & 1) * p.NU + ugi) * p.NU * E), 0, p.NU * E * 4, 0x00020000);
      unsigned off = lane_base;
      asm volatile("" : "+v"(off));              // one add per load instead of SPS loop-invariant offsets held in registers
      if constexpr (WIDE) {
#pragma unroll
        for (int k = 0; k < WNL; ++k) {
          const u32x4 q = __builtin_amdgcn_raw_buffer_load_b128(rb, off + (unsigned)(k * WS * E * 4), 0, LD_AUX);
          v[4 * k] = q[0]; v[4 * k + 1] = q[1]; v[4 * k + 2] = q[2]; v[4 * k + 3] = q[3];
        }
      } else {
#pragma unroll
      for (int k = 0; k < SPS; ++k)
        v[k] = __builtin_amdgcn_raw_buffer_load_b32(rb, off + (unsigned)(k * P * E * 4), 0, LD_AUX);
      }
    };
    for (int step = 0; step < p.T; ++step) {
      const int t = dir == 0 ? p.T - 1 - step : step;
      mark(step, 0);
      float dh = 0.0f;
      if (step > 0 && tid < NPOLL) {
        // ---- poll the data: every dword of this lane must carry the tag of step-1; if one is still old, ALL are loaded again
        const unsigned tg = ((((unsigned)(step - 1) >> 1) & 1u) ^ 1u);
        unsigned spins = 0;
        for (;;) {
          unsigned bad = 0u;
#pragma unroll
          for (int k = 0; k < SPS; ++k) bad |= (v[k] ^ tg) & (vmask >> (WIDE ? k / 4 : k));
          if (__all((bad & 1u) == 0u) || gave_up) break;
          if (!FAST) __builtin_amdgcn_s_sleep(1);
          if ((++spins & 63u) == 0 &&
              (spins > p.spin_limit || __hip_atomic_load(abort_w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
            if (lane == 0) __hip_atomic_store(abort_w, 2u + (unsigned)step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            gave_up = true;
          }
          fetch(step);
        }
        mark(step, 1);
        if constexpr (WIDE) {
          float s4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
          for (int k = 0; k < WNL; ++k)
#pragma unroll
            for (int c = 0; c < 4; ++c) s4[c] += __builtin_bit_cast(float, v[4 * k + c] & ~1u);   // out-of-range loads return 0
          // the WS lanes of a row quad (lanes wsub, wsub + WSUBS, ... of the unit's 16): rotations within the row of 16, every lane takes part
          auto ror_add = [&](auto off_c) __attribute__((always_inline)) {          // s4 += row_ror:OFF (s4): the DPP control is an immediate
            constexpr int OFF = decltype(off_c)::value;
            if constexpr (OFF >= WSUBS) {
#pragma unroll
              for (int c = 0; c < 4; ++c)
                s4[c] += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s4[c]), 0x120 + OFF, 0xf, 0xf, false));
            }
          };
          ror_add(std::integral_constant<int, 1>{});
          ror_add(std::integral_constant<int, 2>{});
          ror_add(std::integral_constant<int, 4>{});
          ror_add(std::integral_constant<int, 8>{});
          const int rc = wrp & 3;
          dh = rc == 0 ? s4[0] : rc == 1 ? s4[1] : rc == 2 ? s4[2] : s4[3];
        } else {
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < SPS; ++k) s += __builtin_bit_cast(float, v[k] & ~1u);   // out-of-range loads return 0
        // the parts of an element: lanes of one quad (every lane of the wave takes part)
        if (P >= 2) s += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s), 0xB1, 0xf, 0xf, false));   // quad_perm [1,0,3,2]
        if (P >= 4) s += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s), 0x4E, 0xf, 0xf, false));   // quad_perm [2,3,0,1]
        dh = s;
        }
      }
      float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
      uint2 dhi = make_uint2(0u, 0u), dlo = make_uint2(0u, 0u);      // the split halves of d: LDS fragment now, dP image behind the exchange
      if (is_el) {
        const float* st = stbuf + ((step & 1) * EMAX + ex) * 8;
        const f32x4 gt = *reinterpret_cast<const f32x4*>(st), cc = *reinterpret_cast<const f32x4*>(st + 4);
        const float ct = cc[0], cprev = cc[1];
        dh += cc[2];
        const float tc = gate_tanh(ct);
        const float dcv = dcarry + dh * gt[3] * (1.0f - tc * tc);
        d.x = dcv * gt[2] * gt[0] * (1.0f - gt[0]);
        d.y = dcv * cprev * gt[1] * (1.0f - gt[1]);
        d.z = dcv * gt[0] * (1.0f - gt[2] * gt[2]);
        d.w = dh * tc * gt[3] * (1.0f - gt[3]);
        dcarry = dcv * gt[1];
        dsum.x += d.x; dsum.y += d.y; dsum.z += d.z; dsum.w += d.w;
        unsigned short hi[4], lo[4];
        split_bf16(d.x, hi[0], lo[0]);
        split_bf16(d.y, hi[1], lo[1]);
        split_bf16(d.z, hi[2], lo[2]);
        split_bf16(d.w, hi[3], lo[3]);
        unsigned short* afd = af_dst + (step & 1) * (KC * AFT * 512);
        dhi = make_uint2((unsigned)hi[0] | ((unsigned)hi[1] << 16), (unsigned)hi[2] | ((unsigned)hi[3] << 16));
        dlo = make_uint2((unsigned)lo[0] | ((unsigned)lo[1] << 16), (unsigned)lo[2] | ((unsigned)lo[3] << 16));
        *reinterpret_cast<uint2*>(afd) = dhi;
        *reinterpret_cast<uint2*>(afd + (STACK ? 8 : 512)) = dlo;
      }
      mark(step, 2);
      if (tid >= NPOLL && step > 0) {            // the state requested after the barrier of the step before: step + 1's
        __builtin_amdgcn_s_waitcnt(0x0F70);
        stage_park(v, step + 1);
      }
      __syncthreads();
      mark(step, 3);
      if (tid >= NPOLL) stage_issue(v, step + 2);
      // ---- this member's contribution to everybody's dh: [16 x 4UG] x [4UG x Hp]
      f32x4 acc[TPW];
#pragma unroll
      for (int i = 0; i < TPW; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < KC; ++c) {
        const unsigned short* afs = afrag + (step & 1) * (KC * AFT * 512);
        if constexpr (STACK) {
          const s16x8 a = *reinterpret_cast<const s16x8*>(afs + c * 512 + lane * 8);
#pragma unroll
          for (int i = 0; i < TPW; ++i) acc[i] = mfma_bf16(a, w[c][i][1], acc[i]);
#pragma unroll
          for (int i = 0; i < TPW; ++i) acc[i] = mfma_bf16(a, w[c][i][0], acc[i]);
        } else {
          const s16x8 ah = *reinterpret_cast<const s16x8*>(afs + (c * 2 + 0) * 512 + lane * 8);
          const s16x8 al = *reinterpret_cast<const s16x8*>(afs + (c * 2 + 1) * 512 + lane * 8);
#pragma unroll
          for (int i = 0; i < TPW; ++i) acc[i] = mfma_bf16(al, w[c][i][0], acc[i]);
#pragma unroll
          for (int i = 0; i < TPW; ++i) acc[i] = mfma_bf16(ah, w[c][i][1], acc[i]);
#pragma unroll
          for (int i = 0; i < TPW; ++i) acc[i] = mfma_bf16(ah, w[c][i][0], acc[i]);
        }
      }
      mark(step, 4);
      if (step + 1 < p.T) {
        const long sbase = (long)(step & 1) * slot_elems;
        const unsigned mytag = ((((unsigned)step >> 1) & 1u) ^ 1u);
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
          const int jj = (wave + NW * i) * 16 + (lane & 15);
          const int md = jj / UG, jl = jj % UG;
          if constexpr (STACK) {
            const int ro = 2 * (lane >> 4);           // this lane's two rows of unit jj: hi.W + lo.W of each
            const bool ok = jj < p.Hp && ro < RG;
            u32x2 o = {__builtin_bit_cast(unsigned, acc[i][0] + acc[i][1]), __builtin_bit_cast(unsigned, acc[i][2] + acc[i][3])};
            o[0] = (o[0] & ~1u) | mytag;
            o[1] = (o[1] & ~1u) | mytag;
            __builtin_amdgcn_raw_buffer_store_b64(o, rx,
                ok ? (unsigned)((sbase + ((long)md * p.NU + ugi) * E + jl * RG + ro) * 4) : kOOB, 0, ST_AUX);
          } else {
            const int ro = 4 * (lane >> 4);           // this lane's four rows of unit jj
            const bool ok = jj < p.Hp && ro < RG;
            u32x4 o = __builtin_bit_cast(u32x4, acc[i]);
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = (o[q] & ~1u) | mytag;
            __builtin_amdgcn_raw_buffer_store_b128(o, rx,
                ok ? (unsigned)((sbase + ((long)md * p.NU + ugi) * E + jl * RG + ro) * 4) : kOOB, 0, ST_AUX);
          }
        }
      }
      mark(step, 5);
      // the pre-activation gradient itself (operand of the weight-gradient GEMMs) leaves behind the exchange -- as fp32, or
      // (round 5) straight as the split-bf16 image those GEMMs read: the same 16 bytes per element, and the separate
      // fp32 -> image pass over all of dP (123 MB read + 123 MB written per layer, 38 us) is gone
      if (inb) {
        if (p.dp_img) {
          unsigned short* ip = p.dp_img + i_off + t * i_step;
          *reinterpret_cast<uint2*>(ip) = dhi;
          *reinterpret_cast<uint2*>(ip + 32) = dlo;
        } else {
          *reinterpret_cast<float4*>(p.gd + g_off + t * g_step) = d;
        }
      }
      mark(step, 7);
      if (step + 1 < p.T && tid < NPOLL) {
        for (int dl = 0; dl < p.delay; ++dl) __builtin_amdgcn_s_sleep(1);
        fetch(step + 1);
      }
      mark(step, 6);
    }
  };
  if (fast) run(std::true_type{}); else run(std::false_type{});
  if (p.db_rows && inb) *reinterpret_cast<float4*>(p.db_rows + g_off) = dsum;
  if constexpr (PROF) {
    __syncthreads();
    if (stamp)
      for (int i = 0; i < STN * 8; ++i) p.dbg[(ST0 + i / 8) * 8 + i % 8] = stamp_s[i];
  }
}
