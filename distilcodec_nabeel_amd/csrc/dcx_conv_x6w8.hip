// conv_gemm_x6w8: the register-staged persistent x6 / bf16 conv kernel (the small-Cout tiles, the
// 4-wave 128 x 128 one-tap tiles and the 256 x 128 fallback) and its launchers.  Arithmetic modes and
// fragment maps: dcx_conv.hip.
#include <mutex>

#include "dcx_conv_common.h"
#include "dcx_conv_launch.h"
#include "dcx_conv_pingpong.h"

namespace dcx {

DCX_DIAG_FILE(x6w8)

// ---------------------------------------------------------------------------------------------
// x6 kernel, WM x WN = 8 waves (512 threads) or 4 waves (256 threads, two workgroups per CU for
// the small-Cout tiles); 2 waves per SIMD either way.  Block tile 256 x 128 has wave tile 64 x 64.
// Same arithmetic and LDS images as conv_gemm_x6; the loads run two K16 steps ahead of their use
// (two register sets, loop unrolled by two), so a step's MFMAs (2 waves x 24 per SIMD = 1536
// cycles) cover the L2 / Infinity-Cache latency of the tiles two steps out.
// ---------------------------------------------------------------------------------------------
// AF32: the input is fp32 (p.x6 == nullptr) and is split into planes while staging (4 channels
// per 16-byte load, three 8-byte LDS stores).  Used for the small-Cout convs (Cout <= 64, Cin <= 128),
// which are bound by HBM traffic (planes cost 6 B per element against 4) and whose planes-input
// variant would need more than 256 VGPRs.
template <int BM, int BN, int WM, int WN, int HALO, bool ARGMIN, int PROD = 6, bool AF32 = false>
__global__ void __launch_bounds__(64 * WM * WN, 2) conv_gemm_x6w8(const ConvParams p) {
  static_assert(WM * WN == 8 || WM * WN == 4, "4 or 8 waves per workgroup");
  static_assert(PROD == 6 || PROD == 1, "x6 or bf16 products");
  constexpr int NT = 64 * WM * WN;
  using XR = XRow<WM * WN == 4>;
  constexpr int XROW = XR::kStride;
  // staged 16-byte pieces per row per K chunk: all (half, plane) pairs, or the two hi pieces
  constexpr int NPC = PROD == 6 ? 6 : 2;
  constexpr int NPL = PROD == 6 ? 3 : 1;  // planes read into fragments
  constexpr int APC = AF32 ? 4 : NPC;     // staged 16-byte pieces per input row per K chunk
  constexpr int WR = BM / WM, WC = BN / WN;
  constexpr int TM = WR / 32, TN = WC / 32;
  constexpr int AROWS = BM + HALO;
  constexpr int A_P = AROWS * APC;  // 16-byte pieces of a staged input tile
  constexpr int B_P = BN * NPC;
  constexpr int A_PT = (A_P + NT - 1) / NT, B_PT = (B_P + NT - 1) / NT;
  constexpr int ABUF = AROWS * XROW, BBUF = BN * XROW;

  // LDS: input tiles (2, by chunk parity) + weight-tile ring (3, by step mod 3).
  __shared__ __attribute__((aligned(16))) unsigned short lds[2 * ABUF + 3 * BBUF];

  static_assert(!ARGMIN, "x6 VQ search uses vq_prefilter_x3");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const long long ldx6 = (long long)p.ldx * 3;
  const int nchunks = p.Cin / BK;
  const int wchunks = nchunks;
  const int taps = p.taps;
  const int nsteps = nchunks * taps;
  const int lo_rel = p.in_step < 0 ? (taps - 1) * p.in_step : 0;
  const long long wslab = (long long)p.Cout * 48;
  const int lin = p.Lin;

  // Persistent tiles.  Iteration `it` of block w takes logical tile
  //   it * G + (w & 7) * (G / 8) + (w >> 3)      (G = gridDim.x, a multiple of 8)
  // so the blocks of one XCD (w & 7 equal) work on G/8 consecutive tiles, column tiles fastest,
  // i.e. they share input row panels in their L2.  Logical tiles run over
  // (phase, clip, row tile, column tile).
  const int ntn = p.Cout / BN, mtiles = (p.Lq + BM - 1) / BM;
  const int per_img = mtiles * ntn, total = per_img * p.batch * p.phases;
  const int G = gridDim.x;
  const int tile_base = (blockIdx.x & 7) * (G >> 3) + (blockIdx.x >> 3);
  int q0 = 0, co0 = 0, b = 0, ph = 0, row0 = 0;
  const unsigned short* __restrict__ xb6 = nullptr;
  const float* __restrict__ xbf = nullptr;
  const unsigned short* __restrict__ wbase = nullptr;
  auto setup = [&](int L) {
    ph = L / (per_img * p.batch);
    const int rem = L - ph * per_img * p.batch;
    b = rem / per_img;
    const int wg = rem - b * per_img;
    const int mt = wg / ntn, nt = wg - mt * ntn;
    q0 = mt * BM;
    co0 = nt * BN;
    row0 = q0 + p.in_base[ph] + lo_rel;
    if constexpr (AF32) xbf = p.x + (long long)b * p.x_bstride;
    else xb6 = p.x6 + (long long)b * p.x_bstride * 3;
    wbase = p.w6 + ((long long)ph * taps * wchunks) * p.Cout * 48 + (long long)co0 * 48;
  };
  int L = tile_base;
  if (L >= total) return;  // whole workgroup, before any barrier
  setup(L);

  // Branch-free staging slots (surplus slots duplicate the last element).
  int a_row[A_PT], a_k[A_PT], a_lds[A_PT];
#pragma unroll
  for (int i = 0; i < A_PT; ++i) {
    const int idx = min(tid + NT * i, A_P - 1);
    a_row[i] = idx / APC;
    a_k[i] = idx - a_row[i] * APC;
    if constexpr (AF32) {  // a_k = 4-channel group; LDS: its half's hi plane + (a_k & 1) * 4
      a_lds[i] = XR::off(a_row[i], (a_k[i] >> 1) * 3) + (a_k[i] & 1) * 4;
    } else {
      if (PROD == 1) a_k[i] *= 3;  // piece = half * 3 + plane
      a_lds[i] = XR::off(a_row[i], a_k[i]);
    }
  }
  int b_off[B_PT], b_lds[B_PT];
#pragma unroll
  for (int i = 0; i < B_PT; ++i) {
    const int idx = min(tid + NT * i, B_P - 1);
    const int col = idx / NPC, piece = (idx - col * NPC) * (PROD == 1 ? 3 : 1);
    b_off[i] = (col * 6 + piece) * 8;
    b_lds[i] = XR::off(col, piece);
  }

  // With a tap halo (taps >= 2) at most one input-chunk load is in flight, so one register set
  // suffices; 1-tap convs load a chunk every step and alternate two sets.
  constexpr int RA_SETS = HALO > 0 ? 1 : 2;
  f32x4 ra[RA_SETS][A_PT];
  f32x4 rb[2][B_PT];

  auto loadA = [&](int c, f32x4(&r)[A_PT]) {
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
  };
  auto storeA = [&](int buf, const f32x4(&r)[A_PT]) {
    unsigned short* A = lds + buf * ABUF;
#pragma unroll
    for (int i = 0; i < A_PT; ++i) {
      if constexpr (AF32) {
        s16x4 hv, mv, lv;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          unsigned short hb, mb, lb;
          split3(p.silu_in ? silu_f(r[i][e]) : r[i][e], hb, mb, lb);  // silu(0) = 0: padding stays 0
          hv[e] = (short)hb;
          mv[e] = (short)mb;
          lv[e] = (short)lb;
        }
        *reinterpret_cast<s16x4*>(A + a_lds[i]) = hv;
        if constexpr (PROD == 6) {
          *reinterpret_cast<s16x4*>(A + a_lds[i] + 8) = mv;
          *reinterpret_cast<s16x4*>(A + a_lds[i] + 16) = lv;
        }
      } else {
        *reinterpret_cast<f32x4*>(A + a_lds[i]) = r[i];
      }
    }
  };
  auto loadB = [&](int c, int m, f32x4(&r)[B_PT]) {
    const unsigned short* src = wbase + ((long long)m * wchunks + c) * wslab;
#pragma unroll
    for (int i = 0; i < B_PT; ++i) r[i] = *reinterpret_cast<const f32x4*>(src + b_off[i]);
  };
  auto storeB = [&](int slot, const f32x4(&r)[B_PT]) {
    unsigned short* Bsm = lds + 2 * ABUF + slot * BBUF;
#pragma unroll
    for (int i = 0; i < B_PT; ++i) *reinterpret_cast<f32x4*>(Bsm + b_lds[i]) = r[i];
  };

  const int lrow = lane & 31;
  const int khalf = lane >> 5;
  int b_frag[TN];  // LDS offsets of this lane's weight-fragment rows (bit 3 is fixed per lane)
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int cc = wn * WC + j * 32 + lrow;
    b_frag[j] = cc * XROW + XR::half(cc, khalf) * 24;
  }
  s16x8 af[2][TM][3], bfr[2][TN][3];
  // fragments of step (c, m) in ring slot `slot` -> register set F
  auto readF = [&](int c, int m, int slot, s16x8(&a)[TM][3], s16x8(&bb)[TN][3]) {
    const int off = m * p.in_step - lo_rel;
    const unsigned short* A = lds + (c & 1) * ABUF;
    const unsigned short* Bsm = lds + 2 * ABUF + slot * BBUF;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int rr = wm * WR + i * 32 + lrow + off;
      const unsigned short* ap = A + rr * XROW + XR::half(rr, khalf) * 24;
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl) a[i][pl] = *reinterpret_cast<const s16x8*>(ap + pl * 8);
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const unsigned short* bp = Bsm + b_frag[j];
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl) bb[j][pl] = *reinterpret_cast<const s16x8*>(bp + pl * 8);
    }
  };

  f32x16 acc[TM][TN];
  DCX_ZERO_ACC16(acc, TM, TN);

  // step positions (chunk, tap) of s+1, s+2, s+3 and the ring slot of step s
  int c1, m1, c2, m2, c3, m3, slot;
  // ---- prologue, part 1 (issued before the previous tile's epilogue): A(0), B(0), B(1), and
  //      for 1-tap convs A(1), into the staging registers
  const int s1c = taps > 1 ? 0 : 1, s1m = taps > 1 ? 1 : 0;  // position of step 1 (nsteps >= 2)
  auto prologue_loads = [&]() {
    loadA(0, ra[0]);
    if constexpr (HALO == 0) loadA(1 < nchunks ? 1 : 0, ra[1 % RA_SETS]);
    loadB(0, 0, rb[0]);
    loadB(s1c, s1m, rb[1]);
  };
  // ---- part 2: to LDS, then the loads in flight for the first loop step: the input chunk
  //      staged next (1-tap: the one first used at step 2; with a halo: chunk 1, held in
  //      registers until step taps - 2 stores it) and B(2)
  auto prologue_stores = [&]() {
    storeA(0, ra[0]);
    if constexpr (HALO == 0) storeA(1, ra[1 % RA_SETS]);
    storeB(0, rb[0]);
    storeB(1, rb[1]);
    c1 = s1c;
    m1 = s1m;
    c2 = c1;
    m2 = m1;
    step_adv(c2, m2, taps);
    c3 = c2;
    m3 = m2;
    step_adv(c3, m3, taps);
    slot = 0;
    if constexpr (HALO > 0) {
      if (nchunks > 1) loadA(1, ra[0]);
    } else {
      if (m2 == 0 && c2 < nchunks) loadA(c2, ra[1 % RA_SETS]);
    }
    loadB(min(c2, nchunks - 1), c2 < nchunks ? m2 : taps - 1, rb[1]);
    __syncthreads();
    readF(0, 0, 0, af[0], bfr[0]);
  };
  prologue_loads();

  auto step = [&](int s, auto qtag) {
    constexpr int Q = decltype(qtag)::value;
    const int slot1 = slot == 2 ? 0 : slot + 1, slot2 = slot1 == 2 ? 0 : slot1 + 1;
    // 1. fragments of step s+1 (its data was made visible by the previous barrier; after the
    //    last step this reads unused LDS, which keeps the step free of branches)
    readF(c1, m1, slot1, af[1 - Q], bfr[1 - Q]);
    // 2. global loads: the input chunk first (so the compiler's merged wait for a chunk store never
    //    covers this step's weight loads), then B for step s+3.  1-tap: the chunk first used at
    //    step s+3.  With a halo: chunk c1 + 1 on the last step of a chunk, taps - 1 steps before
    //    step (c1, taps - 2) stores it (one register set: the previous chunk is stored by then).
    if constexpr (HALO > 0) {
      if (m1 == 0 && c1 + 1 < nchunks) loadA(c1 + 1, ra[0]);
    } else {
      if (m3 == 0 && c3 < nchunks) loadA(c3, ra[Q % RA_SETS]);
    }
    loadB(min(c3, nchunks - 1), c3 < nchunks ? m3 : taps - 1, rb[Q]);
    // 3. MFMAs of step s
    x6_products<PROD>(acc, af[Q], bfr[Q]);
    // 4. stage step s+2: weight tile into its ring slot; its input chunk if s+2 opens one
    storeB(slot2, rb[1 - Q]);
    if (m2 == 0 && c2 < nchunks) storeA(c2 & 1, ra[(1 - Q) % RA_SETS]);
    __syncthreads();
    step_adv(c1, m1, taps);
    step_adv(c2, m2, taps);
    step_adv(c3, m3, taps);
    slot = slot1;
  };
  for (;;) {
    prologue_stores();
    // nsteps is even (launcher): without an odd exit the loop header never merges a path on which
    // this iteration's loads are still in flight, which made the waitcnt pass emit vmcnt(0).
    DCX_CLOCK_BEGIN;
    for (int s = 0; s < nsteps; s += 2) {
      step(s, std::integral_constant<int, 0>{});
      step(s + 1, std::integral_constant<int, 1>{});
    }
    DCX_CLOCK_END(nsteps);
    // the next tile's first loads go out before this tile's epilogue, which hides their latency
    const int eq0 = q0, eco0 = co0, eb = b, eph = ph;
    const int Ln = L + G;
    const bool more = Ln < total;  // uniform over the workgroup
    if (more) {
      setup(Ln);
      prologue_loads();
    }
    epilogue_lds<BM, BN, WM, WN, (2 * ABUF + 3 * BBUF) / 2, NT, HALO ? 0 : 2>(p, p, acc, eq0, eco0, eb, eph,
                                                                reinterpret_cast<float*>(lds));
    if (!more) break;
    L = Ln;
    DCX_ZERO_ACC16(acc, TM, TN);
    __syncthreads();  // the epilogue's LDS reads are done before the next prologue writes LDS
  }
}

// Persistent launch: as many workgroups as fit on the device at once (occupancy from the
// runtime, once per kernel), a multiple of 8 (XCD grouping), at most the tile count rounded up.
template <int BM, int BN, int WM, int WN, int HALO, int PROD, bool AF32>
static hipError_t launch_x6_persistent(ConvParams p, int batch, int phases, hipStream_t s) {
  auto kern = conv_gemm_x6w8<BM, BN, WM, WN, HALO, false, PROD, AF32>;
  static std::once_flag once;  // workgroups resident per CU (per instantiation, queried once)
  static int per_cu = 0;
  std::call_once(once, [&] {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 64 * WM * WN, 0) != hipSuccess) per_cu = 0;
  });
  if (per_cu < 1) return hipErrorInvalidValue;
  const int resident = device_cus() * per_cu;
  p.batch = batch;
  p.phases = phases;
  const long long total = flat_tiles<BM, BN>(p, batch, phases);
  if (total > (1LL << 30)) return hipErrorInvalidValue;
  int g = (int)std::min<long long>(resident, (total + 7) / 8 * 8);
  g = std::max(8, g / 8 * 8);
  hipLaunchKernelGGL(kern, dim3(g), dim3(64 * WM * WN), 0, s, p);
  return hipGetLastError();
}

template <int BM, int BN, int WM, int WN, int HALO, bool ARGMIN>
hipError_t launch_x6w8(const ConvParams& p, int batch, int phases, hipStream_t s) {
  static_assert(!ARGMIN, "x6 VQ search uses vq_prefilter_x3");
  return p.nprod == 1 ? launch_x6_persistent<BM, BN, WM, WN, HALO, 1, false>(p, batch, phases, s)
                      : launch_x6_persistent<BM, BN, WM, WN, HALO, 6, false>(p, batch, phases, s);
}

// fp32-input variant (Cin <= 64 convs, see conv_gemm_x6w8)
template <int BM, int BN, int WM, int WN, int HALO>
hipError_t launch_x6w8_af32(const ConvParams& p, int batch, int phases, hipStream_t s) {
  return p.nprod == 1 ? launch_x6_persistent<BM, BN, WM, WN, HALO, 1, true>(p, batch, phases, s)
                      : launch_x6_persistent<BM, BN, WM, WN, HALO, 6, true>(p, batch, phases, s);
}

// the shapes launch_conv names
#define DCX_INST(...) template hipError_t launch_x6w8<__VA_ARGS__, false>(const ConvParams&, int, int, hipStream_t)
DCX_INST(128, 128, 2, 2, 0);
DCX_INST(256, 128, 4, 2, 64);
DCX_INST(256, 64, 4, 1, 64);
DCX_INST(256, 64, 4, 1, 0);
DCX_INST(256, 32, 4, 1, 64);
DCX_INST(256, 32, 4, 1, 0);
#undef DCX_INST
template hipError_t launch_x6w8_af32<256, 64, 4, 1, 64>(const ConvParams&, int, int, hipStream_t);
template hipError_t launch_x6w8_af32<256, 32, 4, 1, 64>(const ConvParams&, int, int, hipStream_t);

}  // namespace dcx
