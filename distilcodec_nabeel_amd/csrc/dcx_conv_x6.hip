// The ping-pong x6 conv kernels on 64K-output and 256 x 128 tiles: conv_gemm_x6pp (register-staged;
// x6pf its fp32-input form), conv_gemm_x6lm (one tap), conv_gemm_x6dm and conv_gemm_x6dq (LDS-DMA
// staging), their grouped forms and launchers.  Arithmetic modes and fragment maps: dcx_conv.hip.
#include "dcx_conv_common.h"
#include "dcx_conv_launch.h"

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
  constexpr int WR = 64, WC = BN / WN, TM = 2, TN = WC / 32;
  constexpr int XROW = 56;  // padded 112-byte rows
  constexpr int AROWS = BM + HALO;
  constexpr int APC = AF32 ? 4 : 6;  // staged 16-byte pieces per input row per chunk
  constexpr int A_P = AROWS * APC, B_P = BN * 6;        // 16-byte pieces per tile
  constexpr int A_H = A_P / 2, B_H = B_P / 2;           // per group
  constexpr int A_PT = (A_H + 255) / 256, B_PT = (B_H + 255) / 256;
  constexpr int ABUF = AROWS * XROW, BBUF = BN * XROW;
  static_assert(A_P % 2 == 0 && B_P % 2 == 0, "halves");
  __shared__ __attribute__((aligned(16))) unsigned short lds[2 * ABUF + 2 * BBUF];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int group = __builtin_amdgcn_readfirstlane(tid >> 8), gt = tid & 255;
  const int wm = wave / WN, wn = wave % WN;
  const int ntiles = p.Cout / BN;
  const int mt = wg / ntiles, nt = wg - mt * ntiles;
  const int q0 = mt * BM, co0 = nt * BN;
  int clip, c0, nchunks;
  ksplit_slice(p, b, clip, c0, nchunks);  // split-K slice (AF32 launches never split)
  const unsigned short* __restrict__ xb6 = AF32 ? nullptr : p.x6 + (long long)clip * p.x_bstride * 3 + c0 * 48;
  const float* __restrict__ xbf = AF32 ? p.x + (long long)clip * p.x_bstride : nullptr;
  const long long ldx6 = (long long)p.ldx * 3;
  const int wchunks = p.Cin / BK;  // weight layout
  const int taps = p.taps;
  const int nsteps = nchunks * taps;
  const int lo_rel = p.in_step < 0 ? (taps - 1) * p.in_step : 0;
  const int row0 = q0 + p.in_base[ph] + lo_rel;
  const unsigned short* __restrict__ wbase =
      p.w6 + ((long long)ph * taps * wchunks + c0) * p.Cout * 48 + (long long)co0 * 48;
  const long long wslab = (long long)p.Cout * 48;
  const int lin = p.Lin;

  // this thread's staging slots in its group's half of each tile (surplus slots repeat the last)
  int a_row[A_PT], a_k[A_PT], b_off[B_PT], b_lds[B_PT];
#pragma unroll
  for (int i = 0; i < A_PT; ++i) {
    const int idx = group * A_H + min(gt + 256 * i, A_H - 1);
    a_row[i] = idx / APC;
    a_k[i] = idx - a_row[i] * APC;  // AF32: 4-channel group
  }
#pragma unroll
  for (int i = 0; i < B_PT; ++i) {
    const int idx = group * B_H + min(gt + 256 * i, B_H - 1);
    const int col = idx / 6, piece = idx - col * 6;
    b_off[i] = idx * 8;
    b_lds[i] = col * XROW + piece * 8;
  }
  f32x4 ra[A_PT], rb[B_PT];
  auto loadA = [&](int c) {
#pragma unroll
    for (int i = 0; i < A_PT; ++i) {
      const int ir = row0 + a_row[i];
      const bool ok = ir >= 0 && ir < lin;
      if constexpr (AF32) {
        const float* src = ok ? xbf + (long long)ir * p.ldx + c * 16 + a_k[i] * 4 : g_zero_row;
        ra[i] = *reinterpret_cast<const f32x4*>(src);
      } else {
        const unsigned short* src =
            ok ? xb6 + (long long)ir * ldx6 + c * 48 + a_k[i] * 8 : reinterpret_cast<const unsigned short*>(g_zero_row);
        ra[i] = *reinterpret_cast<const f32x4*>(src);
      }
    }
  };
  auto storeA = [&](int buf) {
#pragma unroll
    for (int i = 0; i < A_PT; ++i) {
      if constexpr (AF32) {  // silu (optional) and the 3-plane split of 4 channels: three 8-byte stores
        s16x4 hv, mv, lv;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          unsigned short hb, mb, lb;
          split3(p.silu_in ? silu_f(ra[i][e]) : ra[i][e], hb, mb, lb);  // silu(0) = 0: padding stays 0
          hv[e] = (short)hb;
          mv[e] = (short)mb;
          lv[e] = (short)lb;
        }
        unsigned short* d = lds + buf * ABUF + a_row[i] * XROW + (a_k[i] >> 1) * 24 + (a_k[i] & 1) * 4;
        *reinterpret_cast<s16x4*>(d) = hv;
        *reinterpret_cast<s16x4*>(d + 8) = mv;
        *reinterpret_cast<s16x4*>(d + 16) = lv;
      } else {
        *reinterpret_cast<f32x4*>(lds + buf * ABUF + a_row[i] * XROW + a_k[i] * 8) = ra[i];
      }
    }
  };
  auto loadB = [&](int c, int m) {
    const unsigned short* src = wbase + ((long long)m * wchunks + c) * wslab;
#pragma unroll
    for (int i = 0; i < B_PT; ++i) rb[i] = *reinterpret_cast<const f32x4*>(src + b_off[i]);
  };
  auto storeB = [&](int slot) {
#pragma unroll
    for (int i = 0; i < B_PT; ++i) *reinterpret_cast<f32x4*>(lds + 2 * ABUF + slot * BBUF + b_lds[i]) = rb[i];
  };

  const int lrow = lane & 31, hoff = (lane >> 5) * 24;
  s16x8 af[TM][3], bfr[TN][3];
  auto readF = [&](int c, int m, int slot) {
    const int off = m * p.in_step - lo_rel;
    const unsigned short* A = lds + (c & 1) * ABUF;
    const unsigned short* Bsm = lds + 2 * ABUF + slot * BBUF;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const unsigned short* ap = A + (wm * WR + i * 32 + lrow + off) * XROW + hoff;
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) af[i][pl] = *reinterpret_cast<const s16x8*>(ap + pl * 8);
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const unsigned short* bp = Bsm + (wn * WC + j * 32 + lrow) * XROW + hoff;
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) bfr[j][pl] = *reinterpret_cast<const s16x8*>(bp + pl * 8);
    }
  };
  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  // s_setprio around the cluster keeps hipcc from moving MFMAs across the segment barriers
  // (cdna_hip_programming.md T5), which would collapse the ping-pong
  auto mfma = [&]() {
    __builtin_amdgcn_s_setprio(1);
#define DCX_MF(i, j, x, y) \
  acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[i][x]), \
                                                      __builtin_bit_cast(bf16x8, bfr[j][y]), acc[i][j], 0, 0, 0)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        DCX_MF(i, j, 2, 0);
        DCX_MF(i, j, 1, 1);
        DCX_MF(i, j, 0, 2);
        DCX_MF(i, j, 1, 0);
        DCX_MF(i, j, 0, 1);
        DCX_MF(i, j, 0, 0);
      }
#undef DCX_MF
    __builtin_amdgcn_s_setprio(0);
  };
  auto adv = [&](int& c_, int& m_) {
    if (++m_ == taps) { m_ = 0; ++c_; }
  };

  // ---- prologue: both groups stage their halves of A(0), B(0), B(1); A(1) when step 1 opens it
  loadA(0);
  loadB(0, 0);
  storeA(0);
  storeB(0);
  int c1 = 0, m1 = 0;  // position of step 1
  adv(c1, m1);
  loadB(c1, m1);
  storeB(1);
  if (m1 == 0) {  // taps == 1
    loadA(1);
    storeA(1);
  }
  // position of the step this group stores next (group 0: step 2 in MEM0(0); group 1: step 2 in
  // MEM1(1)) and of the step it reads next; both groups start their loads for step 2
  int cw = c1, mw = m1;
  adv(cw, mw);                        // step 2
  int cl = cw, ml = mw;               // next load: step 2
  if (nsteps > 2) {
    loadB(cl, ml);
    if (ml == 0) loadA(cl);
  }
  adv(cl, ml);                        // step 3
  __syncthreads();
#ifdef DCX_CLOCK_DIAG
  const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
#endif
  int cr = 0, mr = 0;                 // position of the step whose fragments are read next
#ifdef DCX_SEG_DIAG
  unsigned long long sd[6] = {}, tprev = 0;
#endif
  if (group == 0) {
    readF(0, 0, 0);
    adv(cr, mr);                      // group 0 reads step 1 in MEM0(0)
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
      if (s + 1 < nsteps) readF(cr, mr, (s + 1) & 1);
      DCX_SEGT(tc1);
      if (s + 2 < nsteps) {
        storeB((s + 2) & 1);
        if (mw == 0) storeA(cw & 1);
      }
      DCX_SEGT(tc2);
      if (s + 3 < nsteps) {
        loadB(cl, ml);
        if (ml == 0) loadA(cl);
      }
      adv(cr, mr);
      adv(cw, mw);
      adv(cl, ml);
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
      readF(cr, mr, s & 1);
      DCX_SEGT(ta1);
      if (s >= 1 && s + 1 < nsteps) {
        storeB((s + 1) & 1);
        if (mw == 0) storeA(cw & 1);
        adv(cw, mw);
      }
      DCX_SEGT(ta2);
      if (s >= 1 && s + 2 < nsteps) {
        loadB(cl, ml);
        if (ml == 0) loadA(cl);
        adv(cl, ml);
      }
      adv(cr, mr);
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
#ifdef DCX_CLOCK_DIAG
  if (threadIdx.x == 0) {
    atomicAdd(&g_clock_diag[0], __builtin_amdgcn_s_memtime() - t0);
    atomicAdd(&g_clock_diag[1], __builtin_amdgcn_s_memrealtime() - r0);
    atomicAdd(&g_clock_diag[2], (unsigned long long)nsteps);
  }
#endif
  epilogue_lds<BM, BN, WM, WN, (2 * ABUF + 2 * BBUF) / 2, 512, HALO ? 0 : 2>(p, pr, acc, q0, co0, b, ph, reinterpret_cast<float*>(lds));
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
  constexpr int WR = 64, WC = BN / WN, TM = 2, TN = WC / 32;
  constexpr int XROW = 56;  // padded 112-byte rows
  constexpr int AROWS = BM + HALO;
  constexpr int A_P = AROWS * 6, B_P = BN * 6;
  constexpr int A_H = A_P / 2, B_H = B_P / 2;
  constexpr int A_PT = (A_H + 255) / 256, B_PT = (B_H + 255) / 256;
  constexpr int ABUF = AROWS * XROW, BBUF = BN * XROW;
  __shared__ __attribute__((aligned(16))) unsigned short lds[2 * ABUF + 2 * BBUF];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int group = __builtin_amdgcn_readfirstlane(tid >> 8), gt = tid & 255;
  const int wm = wave / WN, wn = wave % WN;
  const int ntiles = p.Cout / BN;
  int wg, b, ph;
  flat_tile(((p.Lq + BM - 1) / BM) * ntiles, p.batch, wg, b, ph);
  const int mt = wg / ntiles, nt = wg - mt * ntiles;
  const int q0 = mt * BM, co0 = nt * BN;
  int clip, c0, nchunks;
  ksplit_slice(p, b, clip, c0, nchunks);  // split-K slice
  const unsigned short* __restrict__ xb6 = p.x6 + (long long)clip * p.x_bstride * 3 + c0 * 48;
  const long long ldx6 = (long long)p.ldx * 3;
  const int wchunks = p.Cin / BK;  // weight layout
  const int taps = p.taps;
  const int nsteps = nchunks * taps;
  const int lo_rel = p.in_step < 0 ? (taps - 1) * p.in_step : 0;
  const int row0 = q0 + p.in_base[ph] + lo_rel;
  const unsigned short* __restrict__ wbase =
      p.w6 + ((long long)ph * taps * wchunks + c0) * p.Cout * 48 + (long long)co0 * 48;
  const long long wslab = (long long)p.Cout * 48;
  const int lin = p.Lin;

  int a_row[A_PT], a_k[A_PT], b_off[B_PT], b_lds[B_PT];
#pragma unroll
  for (int i = 0; i < A_PT; ++i) {
    const int idx = group * A_H + min(gt + 256 * i, A_H - 1);
    a_row[i] = idx / 6;
    a_k[i] = idx - a_row[i] * 6;
  }
#pragma unroll
  for (int i = 0; i < B_PT; ++i) {
    const int idx = group * B_H + min(gt + 256 * i, B_H - 1);
    const int col = idx / 6, piece = idx - col * 6;
    b_off[i] = idx * 8;
    b_lds[i] = col * XROW + piece * 8;
  }
  f32x4 ra[2][A_PT], rb[2][B_PT];
  auto loadA = [&](int c, f32x4(&r)[A_PT]) {
#pragma unroll
    for (int i = 0; i < A_PT; ++i) {
      const int ir = row0 + a_row[i];
      const bool ok = ir >= 0 && ir < lin;
      const unsigned short* src =
          ok ? xb6 + (long long)ir * ldx6 + c * 48 + a_k[i] * 8 : reinterpret_cast<const unsigned short*>(g_zero_row);
      r[i] = *reinterpret_cast<const f32x4*>(src);
    }
  };
  auto storeA = [&](int buf, const f32x4(&r)[A_PT]) {
#pragma unroll
    for (int i = 0; i < A_PT; ++i)
      *reinterpret_cast<f32x4*>(lds + buf * ABUF + a_row[i] * XROW + a_k[i] * 8) = r[i];
  };
  auto loadB = [&](int c, int m, f32x4(&r)[B_PT]) {
    const unsigned short* src = wbase + ((long long)m * wchunks + c) * wslab;
#pragma unroll
    for (int i = 0; i < B_PT; ++i) r[i] = *reinterpret_cast<const f32x4*>(src + b_off[i]);
  };
  auto storeB = [&](int slot, const f32x4(&r)[B_PT]) {
#pragma unroll
    for (int i = 0; i < B_PT; ++i) *reinterpret_cast<f32x4*>(lds + 2 * ABUF + slot * BBUF + b_lds[i]) = r[i];
  };

  const int lrow = lane & 31, hoff = (lane >> 5) * 24;
  s16x8 af[TM][3], bfr[TN][3];
  auto readF = [&](int c, int m, int slot) {
    const int off = m * p.in_step - lo_rel;
    const unsigned short* A = lds + (c & 1) * ABUF;
    const unsigned short* Bsm = lds + 2 * ABUF + slot * BBUF;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const unsigned short* ap = A + (wm * WR + i * 32 + lrow + off) * XROW + hoff;
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) af[i][pl] = *reinterpret_cast<const s16x8*>(ap + pl * 8);
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const unsigned short* bp = Bsm + (wn * WC + j * 32 + lrow) * XROW + hoff;
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) bfr[j][pl] = *reinterpret_cast<const s16x8*>(bp + pl * 8);
    }
  };
  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  // MFMA cluster of one step with the staging loads `ld` spread through it: NL loads, one after
  // every 24 / (NL + 1) MFMAs (sched_group_barrier pins the order), so their issue overlaps MFMAs
  // instead of holding back the first one
  auto mfma_with = [&](auto nl_tag, auto&& ld) {
    constexpr int NL = decltype(nl_tag)::value;
    __builtin_amdgcn_s_setprio(1);
    ld();
#define DCX_MF(i, j, x, y) \
  acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[i][x]), \
                                                      __builtin_bit_cast(bf16x8, bfr[j][y]), acc[i][j], 0, 0, 0)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        DCX_MF(i, j, 2, 0);
        DCX_MF(i, j, 1, 1);
        DCX_MF(i, j, 0, 2);
        DCX_MF(i, j, 1, 0);
        DCX_MF(i, j, 0, 1);
        DCX_MF(i, j, 0, 0);
      }
#undef DCX_MF
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
  auto adv = [&](int& c_, int& m_) {
    if (++m_ == taps) { m_ = 0; ++c_; }
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
      if (ml == 0 && cl < nchunks) loadA(cl, ra[Q]);
  };
  auto load_in = [&](auto qtag) {
    constexpr int Q = decltype(qtag)::value;
    return [&]() {
      if constexpr (HALO == 0) loadA(min(cl, nchunks - 1), ra[Q]);
      loadB(min(cl, nchunks - 1), cl < nchunks ? ml : taps - 1, rb[Q]);
    };
  };
  auto load_step = [&](auto qtag) {  // prologue: plain
    constexpr int Q = decltype(qtag)::value;
    if (ml == 0 && cl < nchunks) loadA(cl, ra[Q]);
    loadB(min(cl, nchunks - 1), cl < nchunks ? ml : taps - 1, rb[Q]);
    adv(cl, ml);
  };

  // ---- prologue: steps 0 and 1 to LDS, step 2 into register set 0
  loadA(0, ra[0]);
  loadB(0, 0, rb[0]);
  storeA(0, ra[0]);
  storeB(0, rb[0]);
  int c1 = 0, m1 = 0;  // position of step 1
  adv(c1, m1);
  loadB(c1, m1, rb[1]);
  if (m1 == 0) loadA(1, ra[1]);  // taps == 1
  storeB(1, rb[1]);
  if (m1 == 0) storeA(1, ra[1]);
  cl = c1;
  ml = m1;
  adv(cl, ml);                   // step 2
  int cw = cl, mw = ml;          // next step this group stores: 2
  load_step(std::integral_constant<int, 0>{});  // step 2 -> set 0; next load: step 3
  __syncthreads();
#ifdef DCX_CLOCK_DIAG
  const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
#endif
  int cr = 0, mr = 0;
  if (group == 0) {
    readF(0, 0, 0);
    adv(cr, mr);
    // iteration s: MFMA(s) (after loading step s+3 into set (s+1) & 1), then MEM0(s): fragments
    // of step s+1, store step s+2 from set s & 1
    auto iter = [&](int s, auto qtag) {
      constexpr int Q = decltype(qtag)::value;  // s & 1
      load_pre(std::integral_constant<int, 1 - Q>{});
      mfma_with(std::integral_constant<int, NL>{}, load_in(std::integral_constant<int, 1 - Q>{}));
      adv(cl, ml);
      __syncthreads();
      if (s + 1 < nsteps) readF(cr, mr, (s + 1) & 1);
      if (s + 2 < nsteps) {
        storeB((s + 2) & 1, rb[Q]);
        if (mw == 0) storeA(cw & 1, ra[Q]);
      }
      adv(cr, mr);
      adv(cw, mw);
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
      readF(cr, mr, s & 1);
      if (s >= 1 && s + 1 < nsteps) {
        storeB((s + 1) & 1, rb[1 - Q]);
        if (mw == 0) storeA(cw & 1, ra[1 - Q]);
      }
      if (s >= 1) adv(cw, mw);
      adv(cr, mr);
      __syncthreads();
      load_pre(std::integral_constant<int, 1 - Q>{});
      mfma_with(std::integral_constant<int, NL>{}, load_in(std::integral_constant<int, 1 - Q>{}));
      adv(cl, ml);
      __syncthreads();
    };
    for (int s = 0; s < nsteps; s += 2) {
      iter(s, std::integral_constant<int, 0>{});
      iter(s + 1, std::integral_constant<int, 1>{});
    }
  }
#ifdef DCX_CLOCK_DIAG
  if (threadIdx.x == 0) {
    atomicAdd(&g_clock_diag[0], __builtin_amdgcn_s_memtime() - t0);
    atomicAdd(&g_clock_diag[1], __builtin_amdgcn_s_memrealtime() - r0);
    atomicAdd(&g_clock_diag[2], (unsigned long long)nsteps);
  }
#endif
  epilogue_lds<BM, BN, 4, WN, (2 * ABUF + 2 * BBUF) / 2, 512, HALO ? 0 : 2>(p, p, acc, q0, co0, b, ph, reinterpret_cast<float*>(lds));
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
// (ConvParams::ksplit; its clips are virtual: slice * clips + clip).  Member by raw block index, the
// XCD remap inside the member, as conv_gemm_x6dq_group.
__global__ void __launch_bounds__(512, 2) conv_gemm_x6pp_group(const ConvGroup g) {
  const int t = blockIdx.x;
  const int k = t >= g.start[1] ? (t >= g.start[2] ? 2 : 1) : 0;
  const int local = xcd_remap(t - g.start[k], g.start[k + 1] - g.start[k]);
  const int b = local / g.tiles_per_clip[k];
  ConvParams p;  // a private copy of the main-loop fields (pr: the range fields, read in place by the epilogue)
  if (k == 0) p = g.p[0];
  else if (k == 1) p = g.p[1];
  else p = g.p[2];
  const ConvParams& pr = k == 0 ? g.p[0] : k == 1 ? g.p[1] : g.p[2];
  x6pp_tile<64, 128>(p, pr, local - b * g.tiles_per_clip[k], b, 0);
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

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int group = __builtin_amdgcn_readfirstlane(tid >> 8);
  const int gw = __builtin_amdgcn_readfirstlane((tid >> 6) & 3);
  const int wm = wave >> 1, wn = wave & 1;
  const int ntiles = p.Cout / BN;
  int wg, b, ph;
  flat_tile(((p.Lq + BM - 1) / BM) * ntiles, p.batch, wg, b, ph);
  const int mt = wg / ntiles, nt = wg - mt * ntiles;
  const int q0 = mt * BM, co0 = nt * BN;
  const int nchunks = p.Cin / BK;
  const int taps = p.taps;
  const int nsteps = nchunks * taps;
  const int lo_rel = p.in_step < 0 ? (taps - 1) * p.in_step : 0;
  const int row0 = q0 + p.in_base[ph] + lo_rel;
  const int arow = p.ldx * 6;  // bytes per planes row
  // halo: descriptor over the clip (negative rows wrap past its range: zeros); 1-tap: over the
  // tile's rows only, so clips of any length keep 32-bit offsets (row0 >= 0 without a halo)
  const __amdgpu_buffer_rsrc_t rx =
      HALO ? __builtin_amdgcn_make_buffer_rsrc((void*)(p.x6 + (long long)b * p.x_bstride * 3), 0, p.Lin * arow, 0x00020000)
           : __builtin_amdgcn_make_buffer_rsrc((void*)(p.x6 + ((long long)b * p.x_bstride + (long long)row0 * p.ldx) * 3), 0,
                                               max(0, min(BM, p.Lin - row0)) * arow, 0x00020000);
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
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  auto mfma = [&]() {
    __builtin_amdgcn_s_setprio(1);
#define DCX_MF(i, j, x, y) \
  acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[i][x]), \
                                                      __builtin_bit_cast(bf16x8, bfr[j][y]), acc[i][j], 0, 0, 0)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        DCX_MF(i, j, 2, 0);
        DCX_MF(i, j, 1, 1);
        DCX_MF(i, j, 0, 2);
        DCX_MF(i, j, 1, 0);
        DCX_MF(i, j, 0, 1);
        DCX_MF(i, j, 0, 0);
      }
#undef DCX_MF
    __builtin_amdgcn_s_setprio(0);
  };
  auto adv = [&](int& c_, int& m_) {
    if (++m_ == taps) { m_ = 0; ++c_; }
  };
  auto inc3 = [](int& slot) { slot = slot == 2 ? 0 : slot + 1; };

  // ---- prologue: steps 0, 1, 2 (both groups their pieces), drained
  int cl = 0, ml = 0;
  for (int t = 0; t < 3; ++t) {
    if (t < nsteps) dma_step(cl, ml, t);
    adv(cl, ml);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  seg_barrier();
#ifdef DCX_CLOCK_DIAG
  const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
#endif
  // cl, ml: step 3, the next step either group issues
  int cr = 0, mr = 0;
  if (group == 0) {
    readF(0, 0, 0);
    adv(cr, mr);
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
      adv(cr, mr);
      adv(cl, ml);
      inc3(rs);
      inc3(ws);
    }
  } else {
    int rs = 0, ws = 0;  // slot of step s, of step s + 2
    for (int s = 0; s < nsteps; ++s) {
      // MEM1(s): fragments of step s, issue step s + 2 (s >= 1), retire step s + 1
      readF(cr, mr, rs);
      int n = 0;
      if (s >= 1 && s + 2 < nsteps) {
        n = dma_step(cl, ml, ws);
        adv(cl, ml);
      }
      wait_dma(n);
      seg_barrier();
      mfma();  // MFMA(s)
      seg_barrier();
      adv(cr, mr);
      inc3(rs);
      if (s >= 1) inc3(ws);
      else ws = 0;  // step 3's slot
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#ifdef DCX_CLOCK_DIAG
  if (threadIdx.x == 0) {  // steps counted in units of x6pp's (half the MFMAs)
    atomicAdd(&g_clock_diag[0], __builtin_amdgcn_s_memtime() - t0);
    atomicAdd(&g_clock_diag[1], __builtin_amdgcn_s_memrealtime() - r0);
    atomicAdd(&g_clock_diag[2], 2ull * nsteps);
  }
#endif
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

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int group = __builtin_amdgcn_readfirstlane(tid >> 8);
  const int gw = __builtin_amdgcn_readfirstlane((tid >> 6) & 3);
  const int wm = wave >> 1, wn = wave & 1;
  const int ntiles = p.Cout / BN;
  const int mt = wg / ntiles, nt = wg - mt * ntiles;
  const int q0 = mt * BM, co0 = nt * BN;
  const int nchunks = p.Cin / BK;
  const int taps = p.taps;
  const int nsteps = nchunks * taps;
  const int lo_rel = p.in_step < 0 ? (taps - 1) * p.in_step : 0;
  const int row0 = q0 + p.in_base[ph] + lo_rel;
  const int arow = p.ldx * 6;
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(p.x6 + (long long)b * p.x_bstride * 3), 0, p.Lin * arow, 0x00020000);
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
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
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
  auto adv = [&](int& c_, int& m_) {
    if (++m_ == taps) { m_ = 0; ++c_; }
  };
  auto inc3 = [](int& slot) { slot = slot == 2 ? 0 : slot + 1; };

  int cl = 0, ml = 0;
  for (int tt = 0; tt < 3; ++tt) {
    if (tt < nsteps) dma_step(cl, ml, tt);
    adv(cl, ml);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  seg_barrier();
  DCX_TILET(tile_t1);
#ifdef DCX_CLOCK_DIAG
  const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
#endif
  int cr = 0, mr = 0;
#ifdef DCX_SEG_DIAG
  unsigned long long sd[4] = {};
#endif
  if (group == 0) {
    readF(0, 0, 0);
    adv(cr, mr);
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
      adv(cr, mr);
      adv(cl, ml);
      inc3(rs);
      inc3(ws);
    }
  } else {
    int rs = 0, ws = 0;
    for (int s = 0; s < nsteps; ++s) {
      DCX_SEGT(ta);
      readF(cr, mr, rs);
      int n = 0;
      if (s >= 1 && s + 2 < nsteps) {
        n = dma_step(cl, ml, ws);
        adv(cl, ml);
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
      adv(cr, mr);
      inc3(rs);
      if (s >= 1) inc3(ws);
      else ws = 0;
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
#ifdef DCX_CLOCK_DIAG
  if (threadIdx.x == 0) {
    atomicAdd(&g_clock_diag[0], __builtin_amdgcn_s_memtime() - t0);
    atomicAdd(&g_clock_diag[1], __builtin_amdgcn_s_memrealtime() - r0);
    atomicAdd(&g_clock_diag[2], 2ull * nsteps);
  }
#endif
  DCX_TILET(tile_t2);
  epilogue_lds<BM, BN, 4, WN, LDS_US / 2, 512, 0>(p, pr, acc, q0, co0, b, ph, reinterpret_cast<float*>(lds));
#ifdef DCX_TILE_DIAG
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long t3 = __builtin_amdgcn_s_memrealtime();
    const unsigned int k = atomicAdd(&g_tile_cnt, 1u);
    if (k < (unsigned)kTileDiagMax) {
      unsigned long long* o = g_tile_diag + 6ull * k;
      o[0] = tile_t0; o[1] = tile_t1; o[2] = tile_t2; o[3] = t3;
      o[4] = __builtin_amdgcn_s_getreg((31 << 11) | 4);
      o[5] = __builtin_amdgcn_s_getreg((15 << 11) | 20);
    }
  }
#endif
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
  // member by raw block index, so every XCD (block index mod 8) gets its share of each member's
  // tiles; a remap of the whole grid would hand the 11-tap tiles to the first XCDs and the 3-tap
  // ones to the last
  const int t = blockIdx.x;
  const int k = t >= g.start[1] ? (t >= g.start[2] ? 2 : 1) : 0;
  const int local = xcd_remap(t - g.start[k], g.start[k + 1] - g.start[k]);
  const int b = local / g.tiles_per_clip[k];
  // a private copy: the tile body's inline-asm barriers clobber memory, which would make the
  // compiler re-read every field of a kernarg-resident struct after each of them
  ConvParams p;  // a private copy of the main-loop fields (pr: the range fields, read in place by the epilogue)
  if (k == 0) p = g.p[0];
  else if (k == 1) p = g.p[1];
  else p = g.p[2];
  const ConvParams& pr = k == 0 ? g.p[0] : k == 1 ? g.p[1] : g.p[2];
  x6dq_tile<BN>(p, pr, local - b * g.tiles_per_clip[k], b, 0);
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
