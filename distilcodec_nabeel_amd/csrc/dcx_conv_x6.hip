// The ping-pong x6 conv kernels on 64K-output and 256 x 128 tiles: conv_gemm_x6pp (register-staged;
// x6pf its fp32-input form), conv_gemm_x6lm (one tap), conv_gemm_x6dm and conv_gemm_x6dq (LDS-DMA
// staging), their grouped forms and launchers.  Arithmetic modes and fragment maps: dcx_conv.hip.
#include "dcx_conv_common.h"
#include "dcx_conv_launch.h"
#include "dcx_conv_pingpong.h"

namespace dcx {

DCX_DIAG_FILE(x6)

// ---------------------------------------------------------------------------------------------
// Ping-pong x6 conv kernel for the dominant shape (256 x 128 tile, tap halo, planes input).
//
// The two waves on each SIMD (wave w and w + 4) belong to different groups: group 0 = waves 0-3
// (tile rows 0-127), group 1 = waves 4-7 (rows 128-255).  Segments are separated by barriers that
// all 8 waves execute; group 0 runs  MFMA(s) | MEM0(s)  and group 1 runs  MEM1(s) | MFMA(s),  so
// in every segment one wave per SIMD issues its 24 MFMAs while its partner reads fragments,
// stores staged tiles and issues global loads, and the matrix pipe no longer idles while both
// waves of a SIMD do their memory work at the same time (conv_gemm_x6w8: ~1/3 of each step).
//
// Segment k = 2s: group 0 MFMA(s), group 1 MEM1(s);  k = 2s+1: group 0 MEM0(s), group 1 MFMA(s).
//   MEM0(s): fragments of step s+1; store its half of step s+2; load its half of step s+3.
//   MEM1(s): fragments of step s;   store its half of step s+1; load its half of step s+2.
// Step t's data is complete after segment 2t-2 and is read in segments 2t-1 (group 0) and 2t
// (group 1), so the weight ring needs only 2 slots (t & 1): step t+2 is written in segments 2t+1
// and 2t+2.  Input tiles are double-buffered by chunk parity and follow the schedule of their
// chunk's first step.  Each group stages half of every tile (both halves with the same maps).
// ---------------------------------------------------------------------------------------------
// AF32 (Cout = 64, fp32 input split while staging, as conv_gemm_x6w4f): 512 x 64 tiles, 8 x 1
// waves with the same 64 x 64 wave tiles, so the staging VALU of one group overlaps the other
// group's MFMAs.
template <int HALO, int BN, bool AF32 = false>
__device__ __forceinline__ void x6pp_tile(const ConvParams& p, const ConvParams& pr, const int wg, const int b, const int ph) {
  // wave tiles 64 x (BN / 2): 24 MFMAs per segment at BN = 128
  static_assert(BN == 128 || BN == 256 || (AF32 && BN == 64), "column tile");
  constexpr int BM = AF32 ? 512 : 256, WN = AF32 ? 1 : 2, WM = 8 / WN;
  using S = X6Stage<BM, BN, HALO, WN, AF32>;  // the staging maps, loads / stores and fragment reads
  constexpr int TM = S::TM, TN = S::TN;
  __shared__ __attribute__((aligned(16))) unsigned short lds[S::LDS_US];

  int clip, c0, nchunks;
  ksplit_slice(p, b, clip, c0, nchunks);  // split-K slice (AF32 launches never split)
  const TileGeo g = tile_geo<BM, BN, WN>(p, wg, ph, nchunks);
  const int group = g.group, taps = g.taps, nsteps = g.nsteps;
  const S st(p, lds, g, clip, c0, ph);
  f32x4 ra[S::A_PT], rb[S::B_PT];  // one staging register set
  s16x8 af[TM][3], bfr[TN][3];
  f32x16 acc[TM][TN];
  DCX_ZERO_ACC16(acc, TM, TN);
  auto mfma = [&]() { x6_mfma_segment(acc, af, bfr); };

  // ---- prologue: both groups stage their halves of A(0), B(0), B(1); A(1) when step 1 opens it
  st.loadA(0, ra);
  st.loadB(0, 0, rb);
  st.storeA(0, ra);
  st.storeB(0, rb);
  int c1 = 0, m1 = 0;  // position of step 1
  step_adv(c1, m1, taps);
  st.loadB(c1, m1, rb);
  st.storeB(1, rb);
  if (m1 == 0) {  // taps == 1
    st.loadA(1, ra);
    st.storeA(1, ra);
  }
  // position of the step this group stores next (group 0: step 2 in MEM0(0); group 1: step 2 in
  // MEM1(1)) and of the step it reads next; both groups start their loads for step 2
  int cw = c1, mw = m1;
  step_adv(cw, mw, taps);             // step 2
  int cl = cw, ml = mw;               // next load: step 2
  if (nsteps > 2) {
    st.loadB(cl, ml, rb);
    if (ml == 0) st.loadA(cl, ra);
  }
  step_adv(cl, ml, taps);             // step 3
  __syncthreads();
  DCX_CLOCK_BEGIN;
  int cr = 0, mr = 0;                 // position of the step whose fragments are read next
#ifdef DCX_SEG_DIAG
  unsigned long long sd[6] = {}, tprev = 0;
#endif
  if (group == 0) {
    st.readF(0, 0, 0, af, bfr);
    step_adv(cr, mr, taps);           // group 0 reads step 1 in MEM0(0)
    for (int s = 0; s < nsteps; ++s) {
      DCX_SEGT(ta);
#ifdef DCX_SEG_DIAG
      if (s) sd[5] += ta - tprev;
#endif
      mfma();                         // MFMA(s)
      DCX_SEGT(tb);
      __syncthreads();
      DCX_SEGT(tc);
      // MEM0(s): fragments of step s+1, store step s+2, load step s+3 (issuing the loads before
      // the fragment reads was slower: 2480 vs 2048 cycles per step at k11)
      if (s + 1 < nsteps) st.readF(cr, mr, (s + 1) & 1, af, bfr);
      DCX_SEGT(tc1);
      if (s + 2 < nsteps) {
        st.storeB((s + 2) & 1, rb);
        if (mw == 0) st.storeA(cw & 1, ra);
      }
      DCX_SEGT(tc2);
      if (s + 3 < nsteps) {
        st.loadB(cl, ml, rb);
        if (ml == 0) st.loadA(cl, ra);
      }
      step_adv(cr, mr, taps);
      step_adv(cw, mw, taps);
      step_adv(cl, ml, taps);
      DCX_SEGT(td);
      __syncthreads();
#ifdef DCX_SEG_DIAG
      sd[0] += tb - ta;
      sd[1] += tc - tb;
      sd[2] += tc1 - tc;
      sd[3] += tc2 - tc1;
      sd[4] += td - tc2;
      tprev = td;
#endif
    }
  } else {
    for (int s = 0; s < nsteps; ++s) {
      // MEM1(s): fragments of step s, store step s+1 (steps 0, 1 came from the prologue),
      // load step s+2 (step 2 was loaded in the prologue)
      DCX_SEGT(ta);
#ifdef DCX_SEG_DIAG
      if (s) sd[1] += ta - tprev;
#endif
      st.readF(cr, mr, s & 1, af, bfr);
      DCX_SEGT(ta1);
      if (s >= 1 && s + 1 < nsteps) {
        st.storeB((s + 1) & 1, rb);
        if (mw == 0) st.storeA(cw & 1, ra);
        step_adv(cw, mw, taps);
      }
      DCX_SEGT(ta2);
      if (s >= 1 && s + 2 < nsteps) {
        st.loadB(cl, ml, rb);
        if (ml == 0) st.loadA(cl, ra);
        step_adv(cl, ml, taps);
      }
      step_adv(cr, mr, taps);
      DCX_SEGT(tb);
      __syncthreads();
      DCX_SEGT(tc);
      mfma();                         // MFMA(s)
      DCX_SEGT(td);
      __syncthreads();
#ifdef DCX_SEG_DIAG
      sd[2] += ta1 - ta;
      sd[3] += ta2 - ta1;
      sd[4] += tb - ta2;
      sd[5] += tc - tb;
      sd[0] += td - tc;
      tprev = td;
#endif
    }
  }
#ifdef DCX_SEG_DIAG
  if ((threadIdx.x & 255) == 0) {
    const int o = group * 6;
#pragma unroll
    for (int i = 0; i < 6; ++i) atomicAdd(&g_seg_diag[o + i], sd[i]);
    if (group == 0) atomicAdd(&g_seg_diag[12], (unsigned long long)nsteps);
  }
#endif
  DCX_CLOCK_END(nsteps);
  epilogue_lds<BM, BN, WM, WN, S::LDS_US / 2, 512, HALO ? 0 : 2>(p, pr, acc, g.q0, g.co0, b, ph, reinterpret_cast<float*>(lds));
}

// ---------------------------------------------------------------------------------------------
// conv_gemm_x6lm: conv_gemm_x6pp with the global loads moved into the MFMA segments.
//
// Per-segment stamps of conv_gemm_x6pp (tools/seg_diag.py) show its MEM segment, not the MFMA
// segment, setting the pace: at k11 a wave spends ~310 cycles issuing its 12 fragment reads,
// ~180 on its LDS stores and ~570 issuing 2-6 global loads behind them, against ~800 for 24
// MFMAs, so the MFMA wave then waits ~250-450 cycles at the barrier.  Here each wave issues its
// next loads at the head of its MFMA segment, while its SIMD partner is the one using LDS, into
// a second staging register set: step t is loaded in MFMA(t - 3) into set t & 1 and stored by
// group 0 in MEM0(t - 2), by group 1 in MEM1(t - 1) (three segments of latency cover either way).
// The loop is unrolled by two so the register sets are static.  Input-chunk loads (conditional)
// go before the weight loads (unconditional, index clamped at the tail), so the weight loads are
// always the youngest and the stores' vmcnt waits stay counted.
// ---------------------------------------------------------------------------------------------
template <int HALO>
__global__ void __launch_bounds__(512, 2) conv_gemm_x6lm(const ConvParams p) {
  constexpr int BM = 256, BN = 128, WN = 2;
  using S = X6Stage<BM, BN, HALO, WN, false>;
  constexpr int TM = S::TM, TN = S::TN, A_PT = S::A_PT, B_PT = S::B_PT;
  __shared__ __attribute__((aligned(16))) unsigned short lds[S::LDS_US];

  int wg, b, ph;
  flat_tile(((p.Lq + BM - 1) / BM) * (p.Cout / BN), p.batch, wg, b, ph);
  int clip, c0, nchunks;
  ksplit_slice(p, b, clip, c0, nchunks);  // split-K slice
  const TileGeo g = tile_geo<BM, BN, WN>(p, wg, ph, nchunks);
  const int group = g.group, taps = g.taps, nsteps = g.nsteps;
  const S st(p, lds, g, clip, c0, ph);
  f32x4 ra[2][A_PT], rb[2][B_PT];  // two staging register sets
  s16x8 af[TM][3], bfr[TN][3];
  f32x16 acc[TM][TN];
  DCX_ZERO_ACC16(acc, TM, TN);
  // MFMA cluster of one step with the staging loads `ld` spread through it: NL loads, one after
  // every 24 / (NL + 1) MFMAs (sched_group_barrier pins the order), so their issue overlaps MFMAs
  // instead of holding back the first one
  auto mfma_with = [&](auto nl_tag, auto&& ld) {
    constexpr int NL = decltype(nl_tag)::value;
    __builtin_amdgcn_s_setprio(1);
    ld();
    x6_products(acc, af, bfr);
    if constexpr (NL > 0) {
      constexpr int G = 24 / (NL + 1);
#pragma unroll
      for (int k = 0; k < NL; ++k) {
        __builtin_amdgcn_sched_group_barrier(0x008, G, 0);  // MFMA
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);  // VMEM read
      }
      __builtin_amdgcn_sched_group_barrier(0x008, 24 - NL * G, 0);
    }
    __builtin_amdgcn_s_setprio(0);
  };
  // loads of step (cl, ml) into register set Q: the input chunk when the step opens one (1-tap:
  // every step, clamped past the end, so unconditional), then the weight tile (clamped past the
  // end, unconditional).  With a halo the input-chunk loads go out before the MFMA cluster and
  // only the weight loads are spread through it.
  int cl, ml;
  constexpr int NL = HALO ? B_PT : A_PT + B_PT;
  auto load_pre = [&](auto qtag) {
    constexpr int Q = decltype(qtag)::value;
    if constexpr (HALO > 0)
      if (ml == 0 && cl < nchunks) st.loadA(cl, ra[Q]);
  };
  auto load_in = [&](auto qtag) {
    constexpr int Q = decltype(qtag)::value;
    return [&]() {
      if constexpr (HALO == 0) st.loadA(min(cl, nchunks - 1), ra[Q]);
      st.loadB(min(cl, nchunks - 1), cl < nchunks ? ml : taps - 1, rb[Q]);
    };
  };
  auto load_step = [&](auto qtag) {  // prologue: plain
    constexpr int Q = decltype(qtag)::value;
    if (ml == 0 && cl < nchunks) st.loadA(cl, ra[Q]);
    st.loadB(min(cl, nchunks - 1), cl < nchunks ? ml : taps - 1, rb[Q]);
    step_adv(cl, ml, taps);
  };

  // ---- prologue: steps 0 and 1 to LDS, step 2 into register set 0
  st.loadA(0, ra[0]);
  st.loadB(0, 0, rb[0]);
  st.storeA(0, ra[0]);
  st.storeB(0, rb[0]);
  int c1 = 0, m1 = 0;  // position of step 1
  step_adv(c1, m1, taps);
  st.loadB(c1, m1, rb[1]);
  if (m1 == 0) st.loadA(1, ra[1]);  // taps == 1
  st.storeB(1, rb[1]);
  if (m1 == 0) st.storeA(1, ra[1]);
  cl = c1;
  ml = m1;
  step_adv(cl, ml, taps);        // step 2
  int cw = cl, mw = ml;          // next step this group stores: 2
  load_step(std::integral_constant<int, 0>{});  // step 2 -> set 0; next load: step 3
  __syncthreads();
  DCX_CLOCK_BEGIN;
  int cr = 0, mr = 0;
  if (group == 0) {
    st.readF(0, 0, 0, af, bfr);
    step_adv(cr, mr, taps);
    // iteration s: MFMA(s) (after loading step s+3 into set (s+1) & 1), then MEM0(s): fragments
    // of step s+1, store step s+2 from set s & 1
    auto iter = [&](int s, auto qtag) {
      constexpr int Q = decltype(qtag)::value;  // s & 1
      load_pre(std::integral_constant<int, 1 - Q>{});
      mfma_with(std::integral_constant<int, NL>{}, load_in(std::integral_constant<int, 1 - Q>{}));
      step_adv(cl, ml, taps);
      __syncthreads();
      if (s + 1 < nsteps) st.readF(cr, mr, (s + 1) & 1, af, bfr);
      if (s + 2 < nsteps) {
        st.storeB((s + 2) & 1, rb[Q]);
        if (mw == 0) st.storeA(cw & 1, ra[Q]);
      }
      step_adv(cr, mr, taps);
      step_adv(cw, mw, taps);
      __syncthreads();
    };
    for (int s = 0; s < nsteps; s += 2) {
      iter(s, std::integral_constant<int, 0>{});
      iter(s + 1, std::integral_constant<int, 1>{});
    }
  } else {
    // iteration s: MEM1(s): fragments of step s, store step s+1 from set (s+1) & 1 (step 1 came
    // from the prologue); then MFMA(s) after loading step s+3 into set (s+1) & 1
    auto iter = [&](int s, auto qtag) {
      constexpr int Q = decltype(qtag)::value;  // s & 1
      st.readF(cr, mr, s & 1, af, bfr);
      if (s >= 1 && s + 1 < nsteps) {
        st.storeB((s + 1) & 1, rb[1 - Q]);
        if (mw == 0) st.storeA(cw & 1, ra[1 - Q]);
      }
      if (s >= 1) step_adv(cw, mw, taps);
      step_adv(cr, mr, taps);
      __syncthreads();
      load_pre(std::integral_constant<int, 1 - Q>{});
      mfma_with(std::integral_constant<int, NL>{}, load_in(std::integral_constant<int, 1 - Q>{}));
      step_adv(cl, ml, taps);
      __syncthreads();
    };
    for (int s = 0; s < nsteps; s += 2) {
      iter(s, std::integral_constant<int, 0>{});
      iter(s + 1, std::integral_constant<int, 1>{});
    }
  }
  DCX_CLOCK_END(nsteps);
  epilogue_lds<BM, BN, 4, WN, S::LDS_US / 2, 512, HALO ? 0 : 2>(p, p, acc, g.q0, g.co0, b, ph, reinterpret_cast<float*>(lds));
}

template <int HALO, int BN, bool AF32 = false>
__global__ void __launch_bounds__(512, 2) conv_gemm_x6pp(const ConvParams p) {
  constexpr int BM = AF32 ? 512 : 256;
  int wg, b, ph;
  flat_tile(((p.Lq + BM - 1) / BM) * (p.Cout / BN), p.batch, wg, b, ph);
  x6pp_tile<HALO, BN, AF32>(p, p, wg, b, ph);
}

// Grouped split-K launch (round 4, the split-K latency mode): up to 3 independent halo convs (the
// three ResBlocks' convs of one dilation index) in one grid, member k with its own K-slice count
// (ConvParams::ksplit; its clips are virtual: slice * clips + clip).  Members as group_member deals them.
__global__ void __launch_bounds__(512, 2) conv_gemm_x6pp_group(const ConvGroup g) {
  ConvParams p;
  int local, b;
  const ConvParams& pr = group_member(g, p, local, b);
  x6pp_tile<64, 128>(p, pr, local, b, 0);
}

template <int HALO>
hipError_t launch_x6pp(const ConvParams& p, int batch, int phases, hipStream_t s, const char** kname) {
  // (BN = 256 needs 128 accumulator + 72 fragment VGPRs and spills at 2 waves per SIMD).  1-tap
  // convs take conv_gemm_x6lm (loads spread through the MFMA segments): 151 -> 161 TF/s at
  // 1024 -> 4096; with a halo it measured equal at k11 and 4-5 % slower at k3 / taps 2.
  if constexpr (HALO == 0) {
    if (kname) *kname = "conv_gemm_x6lm<256,128>";
    return launch_flat<256, 128>(conv_gemm_x6lm<0>, p, batch, phases, 512, s);
  } else {
    if (kname) *kname = "conv_gemm_x6pp<256,128,halo>";
    return launch_flat<256, 128>(conv_gemm_x6pp<HALO, 128>, p, batch, phases, 512, s);
  }
}

// ---------------------------------------------------------------------------------------------
// conv_gemm_x6dm: ping-pong x6 conv on 256 x 256 (or 512 x 128) tiles with LDS-DMA staging.
//
// conv_gemm_x6pp's per-segment stamps put its memory segment (12 fragment reads, register-staged
// LDS stores, global loads: ~1050 cycles at k11) above its MFMA segment (24 MFMAs, ~800), so the
// matrix pipe waited at every barrier.  Here:
//  * staging is LDS-DMA (buffer_load_dwordx4 ... lds): no staging registers and no ds_write
//    pass in the memory segment; each wave issues its pieces and retires them one segment later
//    with a counted vmcnt;
//  * the freed registers buy 64 x 128 wave tiles (256 x 256 block tile): 48 MFMAs per segment
//    against 18 fragment reads (a quarter fewer LDS reads per MFMA than 64 x 64), and each input
//    tile is re-read by half as many column tiles.
// LDS images are lane-linear per DMA instruction (1 KiB = 64 x 16 B): the unpadded 96-byte rows
// of XRow<true> (rows with bit 3 set hold their two K halves swapped, conflict-free fragment
// reads at any tap offset), the swizzle applied on the per-lane SOURCE offsets.  Out-of-range
// input rows (the conv's zero padding) are out of the buffer descriptor's range and load zeros.
// Ring: 3 weight slots (step t in slot t % 3) and 2 input-chunk buffers (chunk parity); step t
// is issued by group 0 in MEM0(t - 3) and by group 1 in MEM1(t - 2), retired at the end of each
// wave's next memory segment, first read in segment 2t - 1 (the schedule of conv_gemm_x6pp).
// ---------------------------------------------------------------------------------------------

// BN = 256: 256 x 256 tiles, 64 x 128 wave tiles; BN = 128: 512 x 128 tiles, 128 x 64 wave tiles
// (the same 48 MFMAs and 18 fragment reads per segment).
template <int HALO, int BN>
__global__ void __launch_bounds__(512, 2) conv_gemm_x6dm(const ConvParams p) {
  constexpr int BM = 65536 / BN, WN = 2;
  constexpr int WR = BM / 4, WC = BN / 2, TM = WR / 32, TN = WC / 32;
  constexpr int XS = XRow<true>::kStride;  // 48 ushorts = 96-byte rows
  // DMA instructions (1 KiB each) per group per tile; a group's instructions are dealt round-robin
  // to its 4 waves.  Halo: input chunks double-buffered by chunk parity; 1-tap: every step opens a
  // chunk, so the input tiles ride the weight ring's 3 slots.
  constexpr int A_G = (BM + HALO) * 6 / 128, B_G = BN * 6 / 128;
  constexpr int A_PW = (A_G + 3) / 4, B_PW = (B_G + 3) / 4;
  constexpr int NA = HALO ? 2 : 3;
  constexpr int ABUF = 2 * A_G * 512;  // ushorts
  constexpr int BBUF = BN * XS;
  constexpr int LDS_US = NA * ABUF + 3 * BBUF;
  static_assert((BM + HALO) * 6 % 128 == 0 && 2 * B_G * 512 == BBUF && A_PW + B_PW <= 11, "DMA piece counts");
  static_assert(LDS_US * 2 <= 160 * 1024, "LDS");
  __shared__ __attribute__((aligned(16))) unsigned short lds[LDS_US];

  int wg, b, ph;
  flat_tile(((p.Lq + BM - 1) / BM) * (p.Cout / BN), p.batch, wg, b, ph);
  const TileGeo g = tile_geo<BM, BN, WN>(p, wg, ph, p.Cin / BK);
  const int lane = g.lane, group = g.group, gw = g.gw, wm = g.wm, wn = g.wn, q0 = g.q0, co0 = g.co0;
  const int nchunks = g.nchunks, taps = g.taps, nsteps = g.nsteps, lo_rel = g.lo_rel, row0 = g.row0;
  const int arow = p.ldx * 6;  // bytes per planes row
  const __amdgpu_buffer_rsrc_t rx = x_desc<6, HALO>(p, b, row0, BM);
  const int rbase = HALO ? row0 : 0;  // row of image row 0 relative to the descriptor
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(p.w6 + (long long)ph * taps * nchunks * p.Cout * 48), 0, taps * nchunks * p.Cout * 96, 0x00020000);

  // per-lane source offsets of this wave's pieces (lane-linear LDS, swizzle on the source); the
  // wave's i-th instruction is its group's instruction i * 4 + gw
  const int a_cnt = (A_G - gw + 3) / 4, b_cnt = (B_G - gw + 3) / 4;  // wave-uniform
  int a_off[A_PW], b_off[B_PW];
#pragma unroll
  for (int i = 0; i < A_PW; ++i) {
    const int P = (group * A_G + i * 4 + gw) * 64 + lane;
    const int row = P / 6, s = P - row * 6;
    const int hl = (s >= 3) ^ ((row >> 3) & 1), pl = s >= 3 ? s - 3 : s;
    a_off[i] = (rbase + row) * arow + (hl * 3 + pl) * 16;  // negative rows: huge unsigned, out of range
  }
#pragma unroll
  for (int i = 0; i < B_PW; ++i) {
    const int P = (group * B_G + i * 4 + gw) * 64 + lane;
    const int col = P / 6, s = P - col * 6;
    const int sg = ((col >> 3) & 1) ? (s >= 3 ? s - 3 : s + 3) : s;
    b_off[i] = (co0 + col) * 96 + sg * 16;
  }
  unsigned short* const a_dst = lds + (group * A_G + gw) * 512;
  unsigned short* const b_dst = lds + NA * ABUF + (group * B_G + gw) * 512;
  auto dmaA = [&](int c, int abuf) {
#pragma unroll
    for (int i = 0; i < A_PW; ++i)
      if (A_G % 4 == 0 || i < a_cnt) dma16(rx, a_dst + abuf * ABUF + i * 2048, a_off[i] + c * 96, 0);
  };
  auto dmaB = [&](int c, int m, int slot) {
    const int soff = (m * nchunks + c) * p.Cout * 96;
#pragma unroll
    for (int i = 0; i < B_PW; ++i)
      if (B_G % 4 == 0 || i < b_cnt) dma16(rw, b_dst + slot * BBUF + i * 2048, b_off[i], soff);
  };
  // DMA of one step (its input chunk first when the step opens one); returns the pieces issued
  auto dma_step = [&](int c, int m, int slot) {
    int n = b_cnt;
    if (m == 0) {
      dmaA(c, HALO ? (c & 1) : slot);
      n += a_cnt;
    }
    dmaB(c, m, slot);
    return n;
  };

  const int lrow = lane & 31, h = lane >> 5;
  s16x8 af[TM][3], bfr[TN][3];
  auto readF = [&](int c, int m, int slot) {
    const int off = m * p.in_step - lo_rel;
    const unsigned short* A = lds + (HALO ? (c & 1) : slot) * ABUF;
    const unsigned short* Bs = lds + NA * ABUF + slot * BBUF;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int r = wm * WR + i * 32 + lrow + off;
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) af[i][pl] = *reinterpret_cast<const s16x8*>(A + XRow<true>::off(r, h * 3 + pl));
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = wn * WC + j * 32 + lrow;
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) bfr[j][pl] = *reinterpret_cast<const s16x8*>(Bs + XRow<true>::off(col, h * 3 + pl));
    }
  };
  f32x16 acc[TM][TN];
  DCX_ZERO_ACC16(acc, TM, TN);
  auto mfma = [&]() { x6_mfma_segment(acc, af, bfr); };

  // The schedule of pingpong3_loop (fragments first), written out: on the shared driver hipcc walked
  // the ring with other scalar code and this kernel measured 0.4-1.9 % slower at 1024 -> 4096
  // (profiles/conv_fold_ab.md).
  // ---- prologue: steps 0, 1, 2 (both groups their pieces), drained
  int cl = 0, ml = 0;
  for (int t = 0; t < 3; ++t) {
    if (t < nsteps) dma_step(cl, ml, t);
    step_adv(cl, ml, taps);
  }
  pingpong3_drain();
  DCX_CLOCK_BEGIN;
  // cl, ml: step 3, the next step either group issues
  int cr = 0, mr = 0;
  if (group == 0) {
    readF(0, 0, 0);
    step_adv(cr, mr, taps);
    int rs = 1, ws = 0;  // slot of the step read next (s + 1), of the step issued next (s + 3)
    for (int s = 0; s < nsteps; ++s) {
      mfma();  // MFMA(s)
      seg_barrier();
      // MEM0(s): fragments of step s + 1, issue step s + 3, retire step s + 2
      if (s + 1 < nsteps) readF(cr, mr, rs);
      int n = 0;
      if (s + 3 < nsteps) n = dma_step(cl, ml, ws);
      wait_dma(n);
      seg_barrier();
      step_adv(cr, mr, taps);
      step_adv(cl, ml, taps);
      ring_inc(rs);
      ring_inc(ws);
    }
  } else {
    int rs = 0, ws = 0;  // slot of step s, of step s + 2
    for (int s = 0; s < nsteps; ++s) {
      // MEM1(s): fragments of step s, issue step s + 2 (s >= 1), retire step s + 1
      readF(cr, mr, rs);
      int n = 0;
      if (s >= 1 && s + 2 < nsteps) {
        n = dma_step(cl, ml, ws);
        step_adv(cl, ml, taps);
      }
      wait_dma(n);
      seg_barrier();
      mfma();  // MFMA(s)
      seg_barrier();
      step_adv(cr, mr, taps);
      ring_inc(rs);
      ring_inc_issue1(ws, s);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  DCX_CLOCK_END(2ull * nsteps);  // steps counted in units of x6pp's (half the MFMAs)
  epilogue_lds<BM, BN, 4, WN, LDS_US / 2, 512, HALO ? 0 : 2>(p, p, acc, q0, co0, b, ph, reinterpret_cast<float*>(lds));
}

// ---------------------------------------------------------------------------------------------
// conv_gemm_x6dq: conv_gemm_x6dm on v_mfma_f32_16x16x32_bf16.
//
// The chip holds a lower clock under 32x32x16 MFMA load than under 16x16x32 at the same cycles per
// FLOP (MI355X_MICROARCH.md, DVFS item 7), and x6dm's loop runs at ~95 % MFMA issue, so what is
// left is the clock.  The six products of a K16 step fold into three K32 MFMAs by pairing terms in
// the K dimension: k = (t, c) with t = lane >> 5 selecting the term, c the channel (lane bits 4
// and 0-3 the channel half and row), so one MFMA sums x_t0 * y_t0 + x_t1 * y_t1 over 16 channels:
//   A{h,m} . B{h',m'} = hh' + mm',   A{m,h} . B{h',m'} = mh' + hm',   A{l,h} . B{h',l'} = lh' + hl'.
// Each operand set is one ds_read_b128 whose lanes pick their plane by t: 3 A sets per 16-row
// block, 2 B sets per 16-column block.  A 64 x 128 (128 x 64) wave tile holds 8 x 4 (4 x 8) f32x4
// accumulators; B fragments for the whole tile and the A fragments of RH row blocks fit in
// registers, the MFMA segment reading the later row blocks' A itself behind the MFMAs of the
// earlier ones.  A is then read in both segments of a step, so the input chunk buffer is reused
// one segment later than in x6dm: taps >= 3 (the ResBlock and conv_pre convs).
// LDS images: 16-row blocks, piece-major inside a block: 16-byte unit (r >> 4) * 96 + s * 16 +
// (r & 15) for piece s = half * 3 + plane of row r; every ds_read_b128 then touches 16
// consecutive rows of one piece per lane group (conflict-free at any tap offset).
// ---------------------------------------------------------------------------------------------
// One output tile (wg = row tile * column tiles + column tile, clip b, phase ph).
template <int BN>
__device__ __forceinline__ void x6dq_tile(const ConvParams& p, const ConvParams& pr, const int wg, const int b, const int ph) {
  DCX_TILET(tile_t0);
  constexpr int HALO = 64;
  constexpr int BM = 65536 / BN, WN = 2;
  constexpr int WR = BM / 4, WC = BN / 2, TM = WR / 16, TN = WC / 16;
  constexpr int RH = BN == 256 ? 2 : 4;  // A row blocks held from the memory segment
  constexpr int A_G = (BM + HALO) * 6 / 128, B_G = BN * 6 / 128;
  constexpr int A_PW = (A_G + 3) / 4, B_PW = (B_G + 3) / 4;
  constexpr int ABUF = 2 * A_G * 512;  // ushorts
  constexpr int BBUF = BN * 48;
  constexpr int LDS_US = 2 * ABUF + 3 * BBUF;
  static_assert((BM + HALO) * 6 % 128 == 0 && 2 * B_G * 512 == BBUF && A_PW + B_PW <= 11, "DMA piece counts");
  static_assert(LDS_US * 2 <= 160 * 1024, "LDS");
  __shared__ __attribute__((aligned(16))) unsigned short lds[LDS_US];

  const TileGeo g = tile_geo<BM, BN, WN>(p, wg, ph, p.Cin / BK);
  const int lane = g.lane, group = g.group, gw = g.gw, wm = g.wm, wn = g.wn, co0 = g.co0;
  const int nchunks = g.nchunks, taps = g.taps, nsteps = g.nsteps, lo_rel = g.lo_rel, row0 = g.row0;
  const int arow = p.ldx * 6;
  const __amdgpu_buffer_rsrc_t rx = x_desc_clip<6>(p, b);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(p.w6 + (long long)ph * taps * nchunks * p.Cout * 48), 0, taps * nchunks * p.Cout * 96, 0x00020000);

  // DMA pieces: unit u of a tile image -> row (u / 96) * 16 + (u & 15), piece (u % 96) >> 4
  const int a_cnt = (A_G - gw + 3) / 4, b_cnt = (B_G - gw + 3) / 4;
  int a_off[A_PW], b_off[B_PW];
#pragma unroll
  for (int i = 0; i < A_PW; ++i) {
    const int u = (group * A_G + i * 4 + gw) * 64 + lane;
    const int blk = u / 96, rem = u - blk * 96;
    a_off[i] = (row0 + blk * 16 + (rem & 15)) * arow + (rem >> 4) * 16;  // negative rows: out of range
  }
#pragma unroll
  for (int i = 0; i < B_PW; ++i) {
    const int u = (group * B_G + i * 4 + gw) * 64 + lane;
    const int blk = u / 96, rem = u - blk * 96;
    b_off[i] = (co0 + blk * 16 + (rem & 15)) * 96 + (rem >> 4) * 16;
  }
  unsigned short* const a_dst = lds + (group * A_G + gw) * 512;
  unsigned short* const b_dst = lds + 2 * ABUF + (group * B_G + gw) * 512;
  auto dma_step = [&](int c, int m, int slot) {
    int n = b_cnt;
    if (m == 0) {
#pragma unroll
      for (int i = 0; i < A_PW; ++i)
        if (A_G % 4 == 0 || i < a_cnt) dma16(rx, a_dst + (c & 1) * ABUF + i * 2048, a_off[i] + c * 96, 0);
      n += a_cnt;
    }
    const int soff = (m * nchunks + c) * p.Cout * 96;
#pragma unroll
    for (int i = 0; i < B_PW; ++i)
      if (B_G % 4 == 0 || i < b_cnt) dma16(rw, b_dst + slot * BBUF + i * 2048, b_off[i], soff);
    return n;
  };

  // fragment sets: lane picks plane by t = lane >> 5, channel half hf = (lane >> 4) & 1
  const int l15 = lane & 15, hf = (lane >> 4) & 1, t = lane >> 5;
  const int soA0 = (hf * 3 + t) * 256, soA1 = (hf * 3 + (t ? 0 : 1)) * 256, soA2 = (hf * 3 + (t ? 0 : 2)) * 256;
  const int soB0 = (hf * 3 + t) * 256, soB1 = (hf * 3 + (t ? 2 : 0)) * 256;  // bytes (piece stride 256)
  const char* const ldsb = reinterpret_cast<const char*>(lds);
  const int bcol = (wn * WC / 16) * 1536 + l15 * 16 + 4 * ABUF;  // bytes, B image of slot 0
  s16x8 aq[RH][3], bq[TN][2];
  int abase = 0;  // bytes: this lane's row in the A image of the step being read
  auto readA1 = [&](int rb, int k, int set) {
    const char* a = ldsb + abase + rb * 1536 + (set == 0 ? soA0 : set == 1 ? soA1 : soA2);
    aq[k][set] = *reinterpret_cast<const s16x8*>(a);
  };
  auto readA = [&](int rb, int k) {
    readA1(rb, k, 0);
    readA1(rb, k, 1);
    readA1(rb, k, 2);
  };
  auto readF = [&](int c, int m, int slot) {
    const int r = wm * WR + m * p.in_step - lo_rel + l15;
    abase = (c & 1) * ABUF * 2 + (r >> 4) * 1536 + (r & 15) * 16;
    const char* bb = ldsb + bcol + slot * BBUF * 2;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      bq[j][0] = *reinterpret_cast<const s16x8*>(bb + j * 1536 + soB0);
      bq[j][1] = *reinterpret_cast<const s16x8*>(bb + j * 1536 + soB1);
    }
#pragma unroll
    for (int k = 0; k < RH; ++k) readA(k, k);
  };
  f32x4 acc[TM][TN];
  zero_acc(acc);
  // MFMA segment: row block by row block, and within a block operand set by operand set (per
  // accumulator: lh' + hl', then mh' + hm', then hh' + mm'); as soon as a set's MFMAs are issued,
  // its registers take the same set of row block rb + RH (read from the same step's image), so the
  // reads are spread through the segment and land 2..3 sets' worth of MFMAs before their use
  auto mfma = [&]() {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int rb = 0; rb < TM; ++rb) {
      const int k = rb % RH;
#pragma unroll
      for (int set = 2; set >= 0; --set) {
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[rb][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, aq[k][set]),
                                                               __builtin_bit_cast(bf16x8, bq[j][set == 2 ? 1 : 0]),
                                                               acc[rb][j], 0, 0, 0);
        if (rb + RH < TM) readA1(rb + RH, k, set);
      }
    }
#pragma unroll
    for (int rb = 0; rb < TM; ++rb)
#pragma unroll
      for (int set = 0; set < 3; ++set) {
        __builtin_amdgcn_sched_group_barrier(0x008, TN, 0);
        if (rb + RH < TM) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
    __builtin_amdgcn_s_setprio(0);
  };

  // conv_gemm_x6dm's loop (written out for the same reason: res128_k11 measured 0.7-1.0 % slower on
  // the shared driver), with the first four DCX_SEG_DIAG slots of pingpong3_loop
  int cl = 0, ml = 0;
  for (int tt = 0; tt < 3; ++tt) {
    if (tt < nsteps) dma_step(cl, ml, tt);
    step_adv(cl, ml, taps);
  }
  pingpong3_drain();
  DCX_TILET(tile_t1);
  DCX_CLOCK_BEGIN;
  int cr = 0, mr = 0;
#ifdef DCX_SEG_DIAG
  unsigned long long sd[4] = {};
#endif
  if (group == 0) {
    readF(0, 0, 0);
    step_adv(cr, mr, taps);
    int rs = 1, ws = 0;
    for (int s = 0; s < nsteps; ++s) {
      DCX_SEGT(ta);
      mfma();  // MFMA(s)
      DCX_SEGT(tb);
      seg_barrier();
      DCX_SEGT(tc);
      if (s + 1 < nsteps) readF(cr, mr, rs);
      int n = 0;
      if (s + 3 < nsteps) n = dma_step(cl, ml, ws);
      wait_dma(n);
      DCX_SEGT(td);
      seg_barrier();
      DCX_SEGT(te);
#ifdef DCX_SEG_DIAG
      sd[0] += tb - ta; sd[1] += tc - tb; sd[2] += td - tc; sd[3] += te - td;
#endif
      step_adv(cr, mr, taps);
      step_adv(cl, ml, taps);
      ring_inc(rs);
      ring_inc(ws);
    }
  } else {
    int rs = 0, ws = 0;
    for (int s = 0; s < nsteps; ++s) {
      DCX_SEGT(ta);
      readF(cr, mr, rs);
      int n = 0;
      if (s >= 1 && s + 2 < nsteps) {
        n = dma_step(cl, ml, ws);
        step_adv(cl, ml, taps);
      }
      wait_dma(n);
      DCX_SEGT(tb);
      seg_barrier();
      DCX_SEGT(tc);
      mfma();  // MFMA(s)
      DCX_SEGT(td);
      seg_barrier();
      DCX_SEGT(te);
#ifdef DCX_SEG_DIAG
      sd[2] += tb - ta; sd[3] += tc - tb; sd[0] += td - tc; sd[1] += te - td;
#endif
      step_adv(cr, mr, taps);
      ring_inc(rs);
      ring_inc_issue1(ws, s);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#ifdef DCX_SEG_DIAG
  if ((threadIdx.x & 255) == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) atomicAdd(&g_seg_diag[group * 6 + i], sd[i]);
    if (group == 0) atomicAdd(&g_seg_diag[12], (unsigned long long)nsteps);
  }
#endif
  DCX_CLOCK_END(2ull * nsteps);
  DCX_TILET(tile_t2);
  epilogue_lds<BM, BN, 4, WN, LDS_US / 2, 512, 0>(p, pr, acc, g.q0, co0, b, ph, reinterpret_cast<float*>(lds));
  DCX_TILE_END(0);
}

template <int BN>
__global__ void __launch_bounds__(512, 2) conv_gemm_x6dq(const ConvParams p) {
  int wg, b, ph;
  flat_tile(((p.Lq + 65536 / BN - 1) / (65536 / BN)) * (p.Cout / BN), p.batch, wg, b, ph);
  x6dq_tile<BN>(p, p, wg, b, ph);
}

// Grouped launch: up to 3 independent convs with the same tiling (the three ResBlocks' convs of one
// dilation index, tap counts 3 / 7 / 11), longest first, so the short ones fill the last round.
template <int BN>
__global__ void __launch_bounds__(512, 2) conv_gemm_x6dq_group(const ConvGroup g) {
  ConvParams p;
  int local, b;
  const ConvParams& pr = group_member(g, p, local, b);
  x6dq_tile<BN>(p, pr, local, b, 0);
}

template <int BN>
hipError_t launch_x6dq(const ConvParams& p, int batch, int phases, hipStream_t s, const char** kname) {
  if (kname) *kname = BN == 256 ? "conv_gemm_x6dq<256,256,halo>" : "conv_gemm_x6dq<512,128,halo>";
  return launch_flat<65536 / BN, BN>(conv_gemm_x6dq<BN>, p, batch, phases, 512, s);
}

template <int HALO, int BN>
hipError_t launch_x6dm(const ConvParams& p, int batch, int phases, hipStream_t s, const char** kname) {
  if (kname)
    *kname = BN == 256 ? (HALO ? "conv_gemm_x6dm<256,256,halo>" : "conv_gemm_x6dm<256,256>") : "conv_gemm_x6dm<512,128,halo>";
  return launch_flat<65536 / BN, BN>(conv_gemm_x6dm<HALO, BN>, p, batch, phases, 512, s);
}

// x6 with an fp32 input at Cout = 64: ping-pong, 512 x 64 tiles
hipError_t launch_x6pf(const ConvParams& p, int batch, int phases, hipStream_t s, const char** kname) {
  if (kname) *kname = "conv_gemm_x6pf<512,64,halo>";
  return launch_flat<512, 64>(conv_gemm_x6pp<64, 64, true>, p, batch, phases, 512, s);
}

hipError_t launch_x6dq_group(const ConvGroup& g, int bn, unsigned blocks, hipStream_t s, const char** kname) {
  if (bn == 256) {
    if (kname) *kname = "conv_gemm_x6dq_group<256,256,halo>";
    hipLaunchKernelGGL((conv_gemm_x6dq_group<256>), dim3(blocks), dim3(512), 0, s, g);
  } else {
    if (kname) *kname = "conv_gemm_x6dq_group<512,128,halo>";
    hipLaunchKernelGGL((conv_gemm_x6dq_group<128>), dim3(blocks), dim3(512), 0, s, g);
  }
  return hipGetLastError();
}

hipError_t launch_x6pp_group(const ConvGroup& g, unsigned blocks, hipStream_t s, const char** kname) {
  if (kname) *kname = "conv_gemm_x6pp_group<256,128,halo>";
  hipLaunchKernelGGL(conv_gemm_x6pp_group, dim3(blocks), dim3(512), 0, s, g);
  return hipGetLastError();
}

// the shapes launch_conv names
template hipError_t launch_x6pp<0>(const ConvParams&, int, int, hipStream_t, const char**);
template hipError_t launch_x6pp<64>(const ConvParams&, int, int, hipStream_t, const char**);
template hipError_t launch_x6dm<0, 256>(const ConvParams&, int, int, hipStream_t, const char**);
template hipError_t launch_x6dm<64, 256>(const ConvParams&, int, int, hipStream_t, const char**);
template hipError_t launch_x6dm<64, 128>(const ConvParams&, int, int, hipStream_t, const char**);
template hipError_t launch_x6dq<256>(const ConvParams&, int, int, hipStream_t, const char**);
template hipError_t launch_x6dq<128>(const ConvParams&, int, int, hipStream_t, const char**);

}  // namespace dcx
