// The pieces the ping-pong conv kernels share (dcx_conv_x6.hip, dcx_conv_x6w8.hip, dcx_conv_h3.hip,
// dcx_conv.hip, dcx_conv_vq.hip): step positions and ring slots, accumulator zeroing, the x6 MFMA
// cluster, the register staging of the 56-ushort-row image, the two-group three-slot LDS-DMA loop,
// the grouped launches' member pick, tile geometry and buffer descriptors, and the diagnostic
// builds' clock and tile stamps.  Phases and hooks, as dcx_resblock_common.h: a kernel keeps its own
// images, DMA and fragment maps and hands them in as callables.
#pragma once
#include "dcx_conv_common.h"

namespace dcx {

// ---------------------------------------------------------------------------------------------
// step positions and ring slots
// ---------------------------------------------------------------------------------------------
// A step is one tap of one input-channel chunk, taps fastest: the position after (c, m).
__device__ __forceinline__ void step_adv(int& c, int& m, int taps) {
  if (++m == taps) { m = 0; ++c; }
}
template <int NS = 3>  // slots of the ring
__device__ __forceinline__ void ring_inc(int& slot) { slot = slot == NS - 1 ? 0 : slot + 1; }
// Group 1's issue slot after its memory segment s, for a ring of NS slots: it issues nothing in
// MEM1(0) (the prologue staged the first NS steps), so its first issue, step NS, takes slot 0.
template <int NS = 3>
__device__ __forceinline__ void ring_inc_issue1(int& ws, int s) {
  if (s >= 1) ring_inc<NS>(ws);
  else ws = 0;  // step NS's slot
}

// Accumulator zeroing.  The f32x16[TM][TN] form is a macro: as a function taking the array by reference
// (any of three bodies tried) hipcc scheduled conv_gemm_x6dm<512,128,halo> differently and its epilogue
// spilled 8 bytes more per lane than with the loops in place (profiles/conv_fold_resources.md).
#define DCX_ZERO_ACC16(acc, TM, TN) \
  _Pragma("unroll") for (int i_ = 0; i_ < (TM); ++i_) \
    _Pragma("unroll") for (int j_ = 0; j_ < (TN); ++j_) \
      _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) (acc)[i_][j_][r_] = 0.f
template <int TM, int TN>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[TM][TN]) {
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// ---------------------------------------------------------------------------------------------
// the x6 products of one K16 step: per 32 x 32 block the six plane products, smallest terms first
// (PROD == 1, the bf16 mode: hi * hi' alone).  The order fixes the bits.
// ---------------------------------------------------------------------------------------------
template <int PROD = 6, int TM, int TN>
__device__ __forceinline__ void x6_products(f32x16 (&acc)[TM][TN], const s16x8 (&af)[TM][3], const s16x8 (&bfr)[TN][3]) {
#define DCX_MF(i, j, x, y) \
  acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[i][x]), \
                                                      __builtin_bit_cast(bf16x8, bfr[j][y]), acc[i][j], 0, 0, 0)
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      if constexpr (PROD == 6) {
        DCX_MF(i, j, 2, 0);
        DCX_MF(i, j, 1, 1);
        DCX_MF(i, j, 0, 2);
        DCX_MF(i, j, 1, 0);
        DCX_MF(i, j, 0, 1);
      }
      DCX_MF(i, j, 0, 0);
    }
#undef DCX_MF
}
// The MFMA segment of a ping-pong x6 kernel.  s_setprio around the cluster keeps hipcc from moving
// MFMAs across the segment barriers (cdna_hip_programming.md T5), which would collapse the ping-pong
template <int TM, int TN>
__device__ __forceinline__ void x6_mfma_segment(f32x16 (&acc)[TM][TN], const s16x8 (&af)[TM][3], const s16x8 (&bfr)[TN][3]) {
  __builtin_amdgcn_s_setprio(1);
  x6_products(acc, af, bfr);
  __builtin_amdgcn_s_setprio(0);
}

// ---------------------------------------------------------------------------------------------
// tile geometry and buffer descriptors
// ---------------------------------------------------------------------------------------------
// Thread roles and the tile's place in the conv: group = the ping-pong group of the wave (waves 0-3 /
// 4-7), gw its wave within the group; (q0, co0) the tile's first output row / channel; row0 the
// input row of image row 0 (lo_rel: the lowest tap's offset, for convs that step backwards).
struct TileGeo {
  int tid, lane, wave, group, gw, wm, wn;
  int q0, co0, nchunks, taps, nsteps, lo_rel, row0;
};
// wg = row tile * column tiles + column tile: the tile's first output row and channel.  On its own for
// the ragged x3dq kernels, which test for a dead tile before anything else of the geometry is computed.
template <int BM, int BN>
__device__ __forceinline__ void tile_origin(const ConvParams& p, int wg, int& q0, int& co0) {
  const int ntiles = p.Cout / BN;
  const int mt = wg / ntiles, nt = wg - mt * ntiles;
  q0 = mt * BM;
  co0 = nt * BN;
}
// nchunks = the K chunks this tile sums
template <int BM, int BN, int WN>
__device__ __forceinline__ TileGeo tile_geo(const ConvParams& p, int wg, int ph, int nchunks) {
  TileGeo g;
  g.tid = threadIdx.x;
  g.lane = g.tid & 63;
  g.wave = g.tid >> 6;
  g.group = __builtin_amdgcn_readfirstlane(g.tid >> 8);
  g.gw = __builtin_amdgcn_readfirstlane((g.tid >> 6) & 3);
  g.wm = g.wave / WN;
  g.wn = g.wave % WN;
  const int ntiles = p.Cout / BN;
  const int mt = wg / ntiles, nt = wg - mt * ntiles;
  g.q0 = mt * BM;
  g.co0 = nt * BN;
  g.nchunks = nchunks;
  g.taps = p.taps;
  g.nsteps = nchunks * g.taps;
  g.lo_rel = p.in_step < 0 ? (g.taps - 1) * p.in_step : 0;
  g.row0 = g.q0 + p.in_base[ph] + g.lo_rel;
  return g;
}
// Input descriptors of the LDS-DMA kernels; EB = bytes per element of a row (planes 6, h2 4).
// Halo: over the clip (negative rows wrap past its range: zeros).
template <int EB>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t x_desc_clip(const ConvParams& p, int b) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)(p.x6 + (long long)b * p.x_bstride * (EB / 2)), 0, p.Lin * (p.ldx * EB),
                                           0x00020000);
}
// One tap: over the tile's rows only, so clips of any length keep 32-bit offsets (row0 >= 0 without a halo).
template <int EB>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t x_desc_tile(const ConvParams& p, int b, int row0, int rows) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)(p.x6 + ((long long)b * p.x_bstride + (long long)row0 * p.ldx) * (EB / 2)), 0,
                                           max(0, min(rows, p.Lin - row0)) * (p.ldx * EB), 0x00020000);
}
template <int EB, int HALO>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t x_desc(const ConvParams& p, int b, int row0, int rows) {
  if constexpr (HALO > 0) return x_desc_clip<EB>(p, b);
  else return x_desc_tile<EB>(p, b, row0, rows);
}

// ---------------------------------------------------------------------------------------------
// Register staging and fragment reads of the register-staged ping-pong kernels (conv_gemm_x6pp,
// x6lm): the 56-ushort-row image (padded 112-byte rows, [half 2][plane 3][8] bf16 per row), two
// input-chunk buffers (chunk parity) and two weight slots.  Each group stages half of every tile,
// both halves with the same maps; the kernel passes the staging register set (x6pp has one, x6lm two).
// AF32: fp32 input, split into planes while staging (4 channels per 16-byte load).
// ---------------------------------------------------------------------------------------------
template <int BM, int BN, int HALO, int WN, bool AF32>
struct X6Stage {
  static constexpr int XROW = 56;  // padded 112-byte rows
  static constexpr int AROWS = BM + HALO;
  static constexpr int APC = AF32 ? 4 : 6;  // staged 16-byte pieces per input row per chunk
  static constexpr int A_P = AROWS * APC, B_P = BN * 6;  // 16-byte pieces per tile
  static constexpr int A_H = A_P / 2, B_H = B_P / 2;     // per group
  static constexpr int A_PT = (A_H + 255) / 256, B_PT = (B_H + 255) / 256;
  static constexpr int ABUF = AROWS * XROW, BBUF = BN * XROW, LDS_US = 2 * ABUF + 2 * BBUF;
  static constexpr int WR = 64, WC = BN / WN, TM = 2, TN = WC / 32;  // wave tiles 64 x (BN / WN)
  static_assert(A_P % 2 == 0 && B_P % 2 == 0, "halves");

  const ConvParams& p;
  // the kernel's image, typed as LDS: behind a generic pointer hipcc's loop heuristics no longer saw
  // LDS accesses and stopped peeling step 0 of group 1's loop in conv_gemm_x6pf (1-2 % slower);
  // C-style casts below, since the host pass rejects a reinterpret_cast out of an address space
  __attribute__((address_space(3))) unsigned short* const lds;
  const unsigned short* __restrict__ xb6;
  const float* __restrict__ xbf;
  const unsigned short* __restrict__ wbase;
  long long ldx6, wslab;
  int wchunks, row0, lin, lo_rel, wm, wn, lrow, hoff;
  // this thread's staging slots in its group's half of each tile (surplus slots repeat the last)
  int a_row[A_PT], a_k[A_PT], b_off[B_PT], b_lds[B_PT];

  // clip, c0: the split-K slice's clip and first chunk (ksplit_slice)
  __device__ __forceinline__ X6Stage(const ConvParams& p_, unsigned short* lds_, const TileGeo& g, int clip, int c0, int ph)
      : p(p_), lds((__attribute__((address_space(3))) unsigned short*)lds_) {
    xb6 = AF32 ? nullptr : p.x6 + (long long)clip * p.x_bstride * 3 + c0 * 48;
    xbf = AF32 ? p.x + (long long)clip * p.x_bstride : nullptr;
    ldx6 = (long long)p.ldx * 3;
    wchunks = p.Cin / BK;  // weight layout
    wbase = p.w6 + ((long long)ph * g.taps * wchunks + c0) * p.Cout * 48 + (long long)g.co0 * 48;
    wslab = (long long)p.Cout * 48;
    row0 = g.row0;
    lin = p.Lin;
    lo_rel = g.lo_rel;
    wm = g.wm;
    wn = g.wn;
    lrow = g.lane & 31;
    hoff = (g.lane >> 5) * 24;
    const int gt = g.tid & 255;
#pragma unroll
    for (int i = 0; i < A_PT; ++i) {
      const int idx = g.group * A_H + min(gt + 256 * i, A_H - 1);
      a_row[i] = idx / APC;
      a_k[i] = idx - a_row[i] * APC;  // AF32: 4-channel group
    }
#pragma unroll
    for (int i = 0; i < B_PT; ++i) {
      const int idx = g.group * B_H + min(gt + 256 * i, B_H - 1);
      const int col = idx / 6, piece = idx - col * 6;
      b_off[i] = idx * 8;
      b_lds[i] = col * XROW + piece * 8;
    }
  }
  __device__ __forceinline__ void loadA(int c, f32x4 (&r)[A_PT]) const {
#pragma unroll
    for (int i = 0; i < A_PT; ++i) {
      const int ir = row0 + a_row[i];
      const bool ok = ir >= 0 && ir < lin;
      if constexpr (AF32) {
        const float* src = ok ? xbf + (long long)ir * p.ldx + c * 16 + a_k[i] * 4 : g_zero_row;
        r[i] = *reinterpret_cast<const f32x4*>(src);
      } else {
        const unsigned short* src =
            ok ? xb6 + (long long)ir * ldx6 + c * 48 + a_k[i] * 8 : reinterpret_cast<const unsigned short*>(g_zero_row);
        r[i] = *reinterpret_cast<const f32x4*>(src);
      }
    }
  }
  __device__ __forceinline__ void storeA(int buf, const f32x4 (&r)[A_PT]) const {
#pragma unroll
    for (int i = 0; i < A_PT; ++i) {
      if constexpr (AF32) {  // silu (optional) and the 3-plane split of 4 channels: three 8-byte stores
        s16x4 hv, mv, lv;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          unsigned short hb, mb, lb;
          split3(p.silu_in ? silu_f(r[i][e]) : r[i][e], hb, mb, lb);  // silu(0) = 0: padding stays 0
          hv[e] = (short)hb;
          mv[e] = (short)mb;
          lv[e] = (short)lb;
        }
        auto* d = lds + buf * ABUF + a_row[i] * XROW + (a_k[i] >> 1) * 24 + (a_k[i] & 1) * 4;
        *(s16x4*)d = hv;
        *(s16x4*)(d + 8) = mv;
        *(s16x4*)(d + 16) = lv;
      } else {
        *(f32x4*)(lds + buf * ABUF + a_row[i] * XROW + a_k[i] * 8) = r[i];
      }
    }
  }
  __device__ __forceinline__ void loadB(int c, int m, f32x4 (&r)[B_PT]) const {
    const unsigned short* src = wbase + ((long long)m * wchunks + c) * wslab;
#pragma unroll
    for (int i = 0; i < B_PT; ++i) r[i] = *reinterpret_cast<const f32x4*>(src + b_off[i]);
  }
  __device__ __forceinline__ void storeB(int slot, const f32x4 (&r)[B_PT]) const {
#pragma unroll
    for (int i = 0; i < B_PT; ++i) *(f32x4*)(lds + 2 * ABUF + slot * BBUF + b_lds[i]) = r[i];
  }
  // fragments of step (c, m), whose weights are in `slot`
  __device__ __forceinline__ void readF(int c, int m, int slot, s16x8 (&af)[TM][3], s16x8 (&bfr)[TN][3]) const {
    const int off = m * p.in_step - lo_rel;
    const auto* A = lds + (c & 1) * ABUF;
    const auto* Bsm = lds + 2 * ABUF + slot * BBUF;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const auto* ap = A + (wm * WR + i * 32 + lrow + off) * XROW + hoff;
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) af[i][pl] = *(const s16x8*)(ap + pl * 8);
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const auto* bp = Bsm + (wn * WC + j * 32 + lrow) * XROW + hoff;
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) bfr[j][pl] = *(const s16x8*)(bp + pl * 8);
    }
  }
};

// ---------------------------------------------------------------------------------------------
// grouped launches: up to 3 independent convs with the same tiling in one grid
// ---------------------------------------------------------------------------------------------
// member of block t of a ConvGroup / SplitEpiGroup (blocks [start[k], start[k + 1]) are member k's)
template <typename Group>
__device__ __forceinline__ int member_index(const Group& g, int t) {
  return t >= g.start[1] ? (t >= g.start[2] ? 2 : 1) : 0;
}
// Member by raw block index, so every XCD (block index mod 8) gets its share of each member's
// tiles; a remap of the whole grid would hand the 11-tap tiles to the first XCDs and the 3-tap
// ones to the last.  The XCD remap runs inside the member.  Out: p, a private copy of the member's
// main-loop fields; local, the tile within its clip; b, the clip.  Returns pr, the member in place
// (the range fields, read there by the epilogue); as the return value, since handed back through an
// out pointer hipcc kept a 1.5 KB stack copy of the whole group.
__device__ __forceinline__ const ConvParams& group_member(const ConvGroup& g, ConvParams& p, int& local, int& b) {
  const int t = blockIdx.x;
  const int k = member_index(g, t);
  local = xcd_remap(t - g.start[k], g.start[k + 1] - g.start[k]);
  b = local / g.tiles_per_clip[k];
  local -= b * g.tiles_per_clip[k];
  // a private copy: the tile body's inline-asm barriers clobber memory, which would make the
  // compiler re-read every field of a kernarg-resident struct after each of them
  if (k == 0) p = g.p[0];
  else if (k == 1) p = g.p[1];
  else p = g.p[2];
  return k == 0 ? g.p[0] : k == 1 ? g.p[1] : g.p[2];
}

// ---------------------------------------------------------------------------------------------
// diagnostic builds (dcx_conv_common.h): the main loop's clocks and a tile's stamps
// ---------------------------------------------------------------------------------------------
#ifdef DCX_CLOCK_DIAG
__device__ __forceinline__ void clock_diag_add(unsigned long long t0, unsigned long long r0, unsigned long long steps) {
  if (threadIdx.x == 0) {
    atomicAdd(&g_clock_diag[0], __builtin_amdgcn_s_memtime() - t0);
    atomicAdd(&g_clock_diag[1], __builtin_amdgcn_s_memrealtime() - r0);
    atomicAdd(&g_clock_diag[2], steps);
  }
}
#define DCX_CLOCK_BEGIN \
  const unsigned long long clk_t0 = __builtin_amdgcn_s_memtime(), clk_r0 = __builtin_amdgcn_s_memrealtime()
#define DCX_CLOCK_END(steps) clock_diag_add(clk_t0, clk_r0, (unsigned long long)(steps))
#else
#define DCX_CLOCK_BEGIN
#define DCX_CLOCK_END(steps)
#endif
#ifdef DCX_TILE_DIAG
// after the epilogue: entry, main loop start, main loop end, exit and the CU's hardware ids
// (extra: the tile's steps, for the kernels whose tools read them)
__device__ __forceinline__ void tile_diag_write(unsigned long long t0, unsigned long long t1, unsigned long long t2,
                                                unsigned long long extra) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long t3 = __builtin_amdgcn_s_memrealtime();
    const unsigned int k = atomicAdd(&g_tile_cnt, 1u);
    if (k < (unsigned)kTileDiagMax) {
      unsigned long long* o = g_tile_diag + 6ull * k;
      o[0] = t0; o[1] = t1; o[2] = t2; o[3] = t3;
      o[4] = __builtin_amdgcn_s_getreg((31 << 11) | 4);
      o[5] = __builtin_amdgcn_s_getreg((15 << 11) | 20) | (extra << 16);
    }
  }
}
#define DCX_TILE_END(extra) tile_diag_write(tile_t0, tile_t1, tile_t2, (unsigned long long)(extra))
#else
#define DCX_TILE_END(extra)
#endif

// ---------------------------------------------------------------------------------------------
// The two-group, three-slot LDS-DMA loop (conv_gemm_x3dq / x3dm, bf16dm, vq_prefilter_dm; conv_gemm_x6dm
// and x6dq_tile run the same schedule written out in place, where it measured 0.4-1.9 % faster).
//
// Ring: step t in slot t % 3.  Segment 2s: group 0 MFMA(s), group 1 MEM1(s); 2s + 1: group 0
// MEM0(s), group 1 MFMA(s), separated by barriers all 8 waves execute.
//   MEM0(s): fragments of step s + 1, issue step s + 3, retire step s + 2.
//   MEM1(s): fragments of step s,     issue step s + 2 (s >= 1), retire step s + 1.
// The kernel supplies  dma_step(c, m, slot) -> pieces this wave issued,  readF(c, m, slot)  and
// mfma().  One-tap streams (bf16dm, vq_prefilter_dm) pass taps = 1, so c counts the steps.
// DMA_FIRST: whether a memory segment issues its DMA before its fragment reads.  Fragments first
// in the x6 kernels (issuing the loads before the fragment reads was slower in conv_gemm_x6pp:
// 2480 vs 2048 cycles per step at k11); the DMA first in x3dq (the fragment reads' latency then
// hides behind the DMA issue, C2 192.8 -> 190.3 ms, r05k).
// DCX_SEG_DIAG stamps of wave 0 / wave 4 into g_seg_diag[group * 6 ..]: MFMA issue, barrier wait,
// memory segment, barrier wait, then the memory segment's first and second part (DMA_FIRST: DMA
// issue, fragment reads); [12] steps.
// ---------------------------------------------------------------------------------------------
struct StepPos {
  int c, m;
};
// prologue: steps 0, 1, 2 issued (both groups their pieces); returns step 3, the next either group issues
template <typename Dma>
__device__ __forceinline__ StepPos pingpong3_prologue(int nsteps, int taps, Dma&& dma_step) {
  StepPos l{0, 0};
  for (int t = 0; t < 3; ++t) {
    if (t < nsteps) dma_step(l.c, l.m, t);
    step_adv(l.c, l.m, taps);
  }
  return l;
}
// the prologue drained, for every wave
__device__ __forceinline__ void pingpong3_drain() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  seg_barrier();
}
template <bool DMA_FIRST, typename Dma, typename Read, typename Mfma>
__device__ __forceinline__ void pingpong3_loop(int group, int nsteps, int taps, StepPos l, Dma&& dma_step, Read&& readF,
                                               Mfma&& mfma) {
  int cl = l.c, ml = l.m;
  int cr = 0, mr = 0;  // the step whose fragments are read next
#ifdef DCX_SEG_DIAG
  unsigned long long sd[6] = {};
#endif
  if (group == 0) {
    readF(0, 0, 0);
    step_adv(cr, mr, taps);
    int rs = 1, ws = 0;  // slot of the step read next (s + 1), of the step issued next (s + 3)
    for (int s = 0; s < nsteps; ++s) {
      DCX_SEGT(ta);
      mfma();  // MFMA(s)
      DCX_SEGT(tb);
      seg_barrier();
      DCX_SEGT(tc);
      int n = 0;
      auto rd = [&]() { if (s + 1 < nsteps) readF(cr, mr, rs); };
      auto issue = [&]() { if (s + 3 < nsteps) n = dma_step(cl, ml, ws); };
      if constexpr (DMA_FIRST) issue();
      else rd();
      DCX_SEGT(tr);
      if constexpr (DMA_FIRST) rd();
      else issue();
      DCX_SEGT(tq);
      wait_dma(n);
      DCX_SEGT(td);
      seg_barrier();
      DCX_SEGT(te);
#ifdef DCX_SEG_DIAG
      sd[0] += tb - ta; sd[1] += tc - tb; sd[2] += td - tc; sd[3] += te - td; sd[4] += tr - tc; sd[5] += tq - tr;
#endif
      step_adv(cr, mr, taps);
      step_adv(cl, ml, taps);
      ring_inc(rs);
      ring_inc(ws);
    }
  } else {
    int rs = 0, ws = 0;  // slot of step s, of step s + 2
    for (int s = 0; s < nsteps; ++s) {
      DCX_SEGT(ta);
      int n = 0;
      auto issue = [&]() {
        if (s >= 1 && s + 2 < nsteps) {
          n = dma_step(cl, ml, ws);
          step_adv(cl, ml, taps);
        }
      };
      if constexpr (DMA_FIRST) issue();
      else readF(cr, mr, rs);
      DCX_SEGT(tr);
      if constexpr (DMA_FIRST) readF(cr, mr, rs);
      else issue();
      DCX_SEGT(tq);
      wait_dma(n);
      DCX_SEGT(tb);
      seg_barrier();
      DCX_SEGT(tc);
      mfma();  // MFMA(s)
      DCX_SEGT(td);
      seg_barrier();
      DCX_SEGT(te);
#ifdef DCX_SEG_DIAG
      sd[2] += tb - ta; sd[3] += tc - tb; sd[0] += td - tc; sd[1] += te - td; sd[4] += tr - ta; sd[5] += tq - tr;
#endif
      step_adv(cr, mr, taps);
      ring_inc(rs);
      ring_inc_issue1(ws, s);
    }
  }
#ifdef DCX_SEG_DIAG
  if ((threadIdx.x & 255) == 0) {
#pragma unroll
    for (int i = 0; i < 6; ++i) atomicAdd(&g_seg_diag[group * 6 + i], sd[i]);
    if (group == 0) atomicAdd(&g_seg_diag[12], (unsigned long long)nsteps);
  }
#endif
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

}  // namespace dcx
