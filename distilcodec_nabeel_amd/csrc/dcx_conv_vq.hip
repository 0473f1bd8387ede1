// The VQ search's prefilter kernels (launch_vq_prefilter): approximate squared distances on the matrix
// cores, per-tile top 2 per row, for vq_rescore (dcx_misc.hip) to certify or rescore.  The exact fp32
// search (launch_vq_argmin) is an instantiation of conv_gemm_f32 and stays in dcx_conv.hip.
#include "dcx_conv_common.h"
#include "dcx_conv_launch.h"
#include "dcx_conv_pingpong.h"

namespace dcx {

DCX_DIAG_FILE(vq)

// ---------------------------------------------------------------------------------------------
// VQ prefilter epilogue: per row of the tile, the smallest and second-smallest approximate
// squared distance (x2 + e2) - 2 x.e and the code of the smallest (lowest index on ties).
// vq_rescore_kernel (dcx_misc.hip) certifies the winner or rescores the candidates from these.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void top2_merge(float& v1, int& i1, float& v2, float ov1, int oi1, float ov2) {
  if (ov1 < v1 || (ov1 == v1 && oi1 < i1)) {
    v2 = fminf(v1, ov2);
    v1 = ov1;
    i1 = oi1;
  } else {
    v2 = fminf(v2, ov1);
  }
}

// top2_merge as selects (no divergent branch: the epilogues run it on every lane), same results
__device__ __forceinline__ void top2_merge_sel(float& v1, int& i1, float& v2, float ov1, int oi1, float ov2) {
  const bool take = (ov1 < v1) | ((ov1 == v1) & (oi1 < i1));  // (bitwise: no short-circuit branch)
  const float nv2 = take ? fminf(v1, ov2) : fminf(v2, ov1);
  v1 = take ? ov1 : v1;
  i1 = take ? oi1 : i1;
  v2 = nv2;
}
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) { return __builtin_amdgcn_mov_dpp(v, CTRL, 0xF, 0xF, false); }
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __builtin_bit_cast(float, dpp_i<CTRL>(__builtin_bit_cast(int, v)));
}
template <int CTRL>
__device__ __forceinline__ void top2_dpp_step(float& v1, int& i1, float& v2) {
  top2_merge_sel(v1, i1, v2, dpp_f<CTRL>(v1), dpp_i<CTRL>(i1), dpp_f<CTRL>(v2));
}
// the top 2 over the 16 lanes of a DPP row (lanes 16 k .. 16 k + 15), left in every lane of it: quad
// xor 1, quad xor 2 (quad_perm), then the half-row mirror (quad 0 <-> 1, 2 <-> 3) and the row mirror
// (the two halves); VALU moves instead of four ds_bpermute round trips per value
__device__ __forceinline__ void top2_row16(float& v1, int& i1, float& v2) {
  top2_dpp_step<0xB1>(v1, i1, v2);   // quad_perm [1, 0, 3, 2]
  top2_dpp_step<0x4E>(v1, i1, v2);   // quad_perm [2, 3, 0, 1]
  top2_dpp_step<0x141>(v1, i1, v2);  // row_half_mirror
  top2_dpp_step<0x140>(v1, i1, v2);  // row_mirror
}

template <int BM, int BN, int WM, int WN>
__device__ __forceinline__ void epilogue_top2(const ConvParams& p, f32x16 (&acc)[BM / WM / 32][BN / WN / 32], int q0,
                                              int co0, int nt, int ntiles, float* smem) {
  constexpr int WR = BM / WM, WC = BN / WN;
  constexpr int TM = WR / 32, TN = WC / 32;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int lrow = lane & 31;
  const int rhalf = 4 * (lane >> 5);
  // every |x|^2 and |e|^2 this lane needs, loaded up front (unconditional, row index clamped: rows
  // past Lq are never stored), so their latency is paid once rather than once per row
  float xxv[TM][16], e2v[TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      xxv[i][r] = p.x2[min(q0 + wm * WR + i * 32 + (r & 3) + 8 * (r >> 2) + rhalf, p.Lq - 1)];
#pragma unroll
  for (int j = 0; j < TN; ++j) e2v[j] = p.e2[co0 + wn * WC + j * 32 + lrow];
  __syncthreads();
  float* rv = smem;                                      // [WN][BM]
  float* rv2 = smem + WN * BM;                           // [WN][BM]
  int* ri = reinterpret_cast<int*>(smem + 2 * WN * BM);  // [WN][BM]
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rloc = wm * WR + i * 32 + (r & 3) + 8 * (r >> 2) + rhalf;
      const float xx = xxv[i][r];
      float v1 = __builtin_inff(), v2 = __builtin_inff();
      int i1 = 0x7fffffff;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int co = co0 + wn * WC + j * 32 + lrow;
        const float d2 = (xx + e2v[j]) + (-2.0f * acc[i][j][r]);
        top2_merge(v1, i1, v2, d2, co, __builtin_inff());
      }
#pragma unroll
      for (int off = 16; off >= 1; off >>= 1)
        top2_merge(v1, i1, v2, __shfl_xor(v1, off, 64), __shfl_xor(i1, off, 64), __shfl_xor(v2, off, 64));
      if (lrow == 0) {
        rv[wn * BM + rloc] = v1;
        rv2[wn * BM + rloc] = v2;
        ri[wn * BM + rloc] = i1;
      }
    }
  }
  __syncthreads();
  for (int rloc = tid; rloc < BM; rloc += blockDim.x) {
    const int q = q0 + rloc;
    if (q >= p.Lq) continue;
    float v1 = rv[rloc], v2 = rv2[rloc];
    int i1 = ri[rloc];
#pragma unroll
    for (int w = 1; w < WN; ++w) top2_merge(v1, i1, v2, rv[w * BM + rloc], ri[w * BM + rloc], rv2[w * BM + rloc]);
    const long long o = (long long)q * ntiles + nt;
    p.part_val[o] = v1;
    p.part_val2[o] = v2;
    p.part_idx[o] = i1;
  }
}

// Tile order of the VQ prefilters.  From 16 row panels on, groups of 16 row panels x 16 code tiles
// are resident together, 4 x 8 per XCD, so the blocks of an XCD stream the same panels through its
// L2 (ntiles % 16 == 0; grid vq_grid).  Below 16 row panels (short clips, a streaming hop) that
// order would leave most XCDs without work (a single row panel: two of eight), so the tiles are
// dealt round-robin over the blocks, code tiles spread over every XCD.  The order changes no result.
__device__ __forceinline__ void vq_tile(int mtiles, int ntiles, int& mt, int& nt) {
  const int bid = blockIdx.x;
  if (mtiles < 16) {
    mt = bid % mtiles;
    nt = bid / mtiles;
    return;
  }
  const int xc = bid & 7, l = (bid >> 3) & 31, sup = bid >> 8;
  const int nsm = (mtiles + 15) >> 4;
  mt = (sup % nsm) * 16 + (xc & 3) * 4 + (l & 3);
  nt = (sup / nsm) * 16 + (xc >> 2) * 8 + (l >> 2);
}
static unsigned vq_grid(int mtiles, int ntiles) {
  return mtiles < 16 ? (unsigned)(mtiles * ntiles) : (unsigned)(((mtiles + 15) / 16) * (ntiles / 16) * 256);
}

// ---------------------------------------------------------------------------------------------
// VQ prefilter GEMM (x6 mode): approximate x.e from hi*hi + hi*mid + mid*hi of the planes
// (bound in launch_vq_prefilter), per-tile top 2 of (x2 + e2) - 2 x.e (epilogue_top2).
//
// Same 8-wave / 256x128 / 64x64-per-wave shape as conv_gemm_x6w8, but a step covers K = 32 (two
// 16-deep sub-chunks, hi and mid planes only: 8 pieces of 16 B per row in a 144-byte LDS row,
// 36 dwords, conflict-free for b128 reads), so a step is 2 x 12 MFMAs per wave like the convs'.
// Fragments are single-buffered per sub-chunk: sub-chunk 0 of step s+1 is read from LDS while
// sub-chunk 1 of step s is on the matrix cores, and vice versa.  Loads run three steps ahead
// (input tile double buffer, weight ring of 3), stores two.
// ---------------------------------------------------------------------------------------------
// XMID = false: the rows of x are bf16 values (mid plane zero, bf16 mode), so only their hi pieces
// are staged and hi*hi + hi*mid' issued (2 products; the bound of launch_vq_prefilter still holds).
template <int BM, int BN, int WM, int WN, bool XMID>
__global__ void __launch_bounds__(512) vq_prefilter_x3(const ConvParams p) {
  static_assert(WM * WN == 8, "8 waves per workgroup");
  constexpr int WR = BM / WM, WC = BN / WN;
  constexpr int TM = WR / 32, TN = WC / 32;
  constexpr int ROW = 72;  // ushort per LDS row: 8 pieces + 1 pad piece
  constexpr int APC = XMID ? 8 : 4;  // staged pieces per input row per step
  constexpr int A_PT = BM * APC / 512, B_PT = BN * 8 / 512;
  static_assert(BM * APC % 512 == 0 && BN * 8 % 512 == 0, "staging pieces per thread");
  constexpr int ABUF = BM * ROW, BBUF = BN * ROW;
  __shared__ __attribute__((aligned(16))) unsigned short lds[2 * ABUF + 3 * BBUF];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int ntiles = p.Cout / BN;
  // grouped order: 16 row panels x 16 code tiles resident together, 4 x 8 per XCD (ntiles % 16 == 0)
  const int mtiles = (p.Lq + BM - 1) / BM;
  int mt, nt;
  vq_tile(mtiles, ntiles, mt, nt);
  if (mt >= mtiles) return;  // whole workgroup, before any barrier
    const int q0 = mt * BM, co0 = nt * BN;
  const int nsteps = p.Cin / 32;
  const long long ldx6 = (long long)p.ldx * 3;
  const long long wslab = (long long)p.Cout * 48;  // one 16-deep chunk of the split codebook

  // staging slots: piece k of a row = (sub u = k >> 2, half h = (k >> 1) & 1, plane k & 1)
  const unsigned short* a_src[A_PT];
  int a_lds[A_PT];
#pragma unroll
  for (int i = 0; i < A_PT; ++i) {
    const int idx = tid + 512 * i, row = idx / APC, k = XMID ? idx & 7 : (idx & 3) * 2;  // hi pieces only
    const int q = q0 + row;
    const int goff = (k >> 2) * 48 + ((k >> 1) & 1) * 24 + (k & 1) * 8;
    a_src[i] = q < p.Lq ? p.x6 + (long long)q * ldx6 + goff : reinterpret_cast<const unsigned short*>(g_zero_row);
    a_lds[i] = row * ROW + k * 8;
  }
  const int a_step = 96;  // ushort per step along a row (zero-page rows must not advance)
  bool a_live[A_PT];
#pragma unroll
  for (int i = 0; i < A_PT; ++i) a_live[i] = q0 + (tid + 512 * i) / APC < p.Lq;
  long long b_off[B_PT];
  int b_lds[B_PT];
#pragma unroll
  for (int i = 0; i < B_PT; ++i) {
    const int idx = tid + 512 * i, col = idx >> 3, k = idx & 7;
    b_off[i] = (long long)(co0 + col) * 48 + (k >> 2) * wslab + ((k >> 1) & 1) * 24 + (k & 1) * 8;
    b_lds[i] = col * ROW + k * 8;
  }

  f32x4 ra[2][A_PT], rb[2][B_PT];
  auto loadA = [&](int s, f32x4(&r)[A_PT]) {
#pragma unroll
    for (int i = 0; i < A_PT; ++i)
      r[i] = *reinterpret_cast<const f32x4*>(a_src[i] + (a_live[i] ? s * a_step : 0));
  };
  auto loadB = [&](int s, f32x4(&r)[B_PT]) {
    const unsigned short* base = p.w6 + (long long)s * 2 * wslab;
#pragma unroll
    for (int i = 0; i < B_PT; ++i) r[i] = *reinterpret_cast<const f32x4*>(base + b_off[i]);
  };
  auto storeA = [&](int buf, const f32x4(&r)[A_PT]) {
#pragma unroll
    for (int i = 0; i < A_PT; ++i) *reinterpret_cast<f32x4*>(lds + buf * ABUF + a_lds[i]) = r[i];
  };
  auto storeB = [&](int slot, const f32x4(&r)[B_PT]) {
#pragma unroll
    for (int i = 0; i < B_PT; ++i) *reinterpret_cast<f32x4*>(lds + 2 * ABUF + slot * BBUF + b_lds[i]) = r[i];
  };

  const int lrow = lane & 31;
  const int hoff = (lane >> 5) * 16;  // K half: pieces (h, hi), (h, mid)
  s16x8 fa[2][TM][2], fb[2][TN][2];   // [sub][tile][plane]
  auto readSub = [&](int buf, int slot, int u) {
    const unsigned short* A = lds + buf * ABUF + u * 32 + hoff;
    const unsigned short* Bs = lds + 2 * ABUF + slot * BBUF + u * 32 + hoff;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const unsigned short* ap = A + (wm * WR + i * 32 + lrow) * ROW;
      fa[u][i][0] = *reinterpret_cast<const s16x8*>(ap);
      if constexpr (XMID) fa[u][i][1] = *reinterpret_cast<const s16x8*>(ap + 8);
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const unsigned short* bp = Bs + (wn * WC + j * 32 + lrow) * ROW;
      fb[u][j][0] = *reinterpret_cast<const s16x8*>(bp);
      fb[u][j][1] = *reinterpret_cast<const s16x8*>(bp + 8);
    }
  };

  f32x16 acc[TM][TN];
  DCX_ZERO_ACC16(acc, TM, TN);
  auto mfmaSub = [&](int u) {
    __builtin_amdgcn_s_setprio(1);  // keeps the MFMA cluster together (measured +5 %)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        if constexpr (XMID)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[u][i][1]),
                                                              __builtin_bit_cast(bf16x8, fb[u][j][0]), acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[u][i][0]),
                                                            __builtin_bit_cast(bf16x8, fb[u][j][1]), acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[u][i][0]),
                                                            __builtin_bit_cast(bf16x8, fb[u][j][0]), acc[i][j], 0, 0, 0);
      }
    __builtin_amdgcn_s_setprio(0);
  };

  // prologue: steps 0 and 1 staged, step 2 in flight
  loadA(0, ra[0]);
  loadB(0, rb[0]);
  storeA(0, ra[0]);
  storeB(0, rb[0]);
  const int s1 = min(1, nsteps - 1), s2 = min(2, nsteps - 1);
  loadA(s1, ra[0]);
  loadB(s1, rb[0]);
  storeA(1, ra[0]);
  storeB(1, rb[0]);
  loadA(s2, ra[1]);
  loadB(s2, rb[1]);
  __syncthreads();
  readSub(0, 0, 0);
  readSub(0, 0, 1);

  int slot = 0;
  auto step = [&](int s, auto qtag) {
    constexpr int Q = decltype(qtag)::value;
    const int slot1 = slot == 2 ? 0 : slot + 1, slot2 = slot1 == 2 ? 0 : slot1 + 1;
    const int s3 = min(s + 3, nsteps - 1);
    loadA(s3, ra[Q]);
    loadB(s3, rb[Q]);
    mfmaSub(0);
    readSub((s + 1) & 1, slot1, 0);  // after the last step: reads unused data, no branch
    mfmaSub(1);
    readSub((s + 1) & 1, slot1, 1);
    storeB(slot2, rb[1 - Q]);
    storeA(s & 1, ra[1 - Q]);  // step s+2's tile into the buffer step s used
    __syncthreads();
    slot = slot1;
  };
  // nsteps is even (launcher): no odd exit, so the loop header never merges a path with this
  // step's loads still in flight (which made the waitcnt pass drain everything, vmcnt(0))
  DCX_CLOCK_BEGIN;
  for (int s = 0; s < nsteps; s += 2) {
    step(s, std::integral_constant<int, 0>{});
    step(s + 1, std::integral_constant<int, 1>{});
  }
  DCX_CLOCK_END(nsteps);  // steps counted in units of 1536 ideal cycles (24 MFMAs x 2 waves per SIMD)
  epilogue_top2<BM, BN, WM, WN>(p, acc, q0, co0, nt, ntiles, reinterpret_cast<float*>(lds));
}

// ---------------------------------------------------------------------------------------------
// vq_prefilter_dm: the VQ prefilter on the conv_gemm_x6dm schedule.
//
// vq_prefilter_x3 issues its MFMAs about half of the time: with 64 x 64 wave tiles its LDS traffic
// (16 fragment reads and 6 register-staged stores per 24 MFMAs) is close to the LDS bandwidth, and
// moving it to LDS-DMA alone did not help.  Here the tiles are 256 x 256 with 64 x 128 wave tiles
// (12 fragment reads per 24 MFMAs, no ds_write pass), staged by LDS-DMA into a 3-slot ring and
// run on the two-group ping-pong schedule of conv_gemm_x6dm (1-tap: every K16 step brings its own
// input and codebook tiles).  Each input row panel is also re-read by half as many code tiles.
// The products per K16 (m*h', h*m', h*h', in that order, on 32x32x16) and so the error bound of
// launch_vq_prefilter are those of vq_prefilter_x3.
// LDS images: 64-byte rows holding the hi and mid pieces of both K halves (piece = half * 2 +
// plane) in slot piece ^ ((row >> 2) & 3), which keeps every 16-lane group of a b128 fragment read
// on 64 distinct banks; lane-linear per DMA instruction, the swizzle applied on the source.
// Rows past the input end are outside the (per-tile) buffer descriptor and load zeros.
// XMID = false (bf16 mode, mid plane of x zero): the m*h' MFMA is skipped.
// ---------------------------------------------------------------------------------------------
template <bool XMID>
__global__ void __launch_bounds__(512, 2) vq_prefilter_dm(const ConvParams p) {
  constexpr int BM = 256, BN = 256, WN = 2;
  constexpr int WR = BM / 4, WC = BN / 2, TM = WR / 32, TN = WC / 32;
  constexpr int RW = 32;                          // ushorts per LDS row
  constexpr int G_I = BM * 4 / 64 / 2;            // DMA instructions per group per tile (A or B)
  constexpr int PW = G_I / 4;                     // ... per wave
  constexpr int ABUF = BM * RW, BBUF = BN * RW;
  constexpr int LDS_US = 3 * ABUF + 3 * BBUF;
  static_assert(BM == BN && G_I % 4 == 0 && LDS_US * 2 <= 160 * 1024, "tile shape");
  __shared__ __attribute__((aligned(16))) unsigned short lds[LDS_US];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int group = __builtin_amdgcn_readfirstlane(tid >> 8);
  const int gw = __builtin_amdgcn_readfirstlane((tid >> 6) & 3);
  const int wm = wave >> 1, wn = wave & 1;
  // grouped order (as vq_prefilter_x3): 16 row panels x 16 code tiles resident together, 4 x 8 per
  // XCD, so the blocks of one XCD stream the same panels through its L2 (ntiles % 16 == 0)
  const int ntiles = p.Cout / BN, mtiles = (p.Lq + BM - 1) / BM;
  int mt, nt;
  vq_tile(mtiles, ntiles, mt, nt);
  if (mt >= mtiles) return;  // whole workgroup, before any barrier
  const int q0 = mt * BM, co0 = nt * BN;
  const int nsteps = p.Cin / BK;
  // planes: a row's / code's four pieces of a K16 step are two 32-byte runs of its 96-byte chunk
  const int arow = p.ldx * 6;  // bytes per input row
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(p.x6 + (long long)q0 * p.ldx * 3), 0, min(BM, p.Lq - q0) * arow, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw =
      __builtin_amdgcn_make_buffer_rsrc((void*)p.w6, 0, nsteps * p.Cout * 96, 0x00020000);

  int a_off[PW], b_off[PW];
#pragma unroll
  for (int i = 0; i < PW; ++i) {
    const int u = (group * G_I + i * 4 + gw) * 64 + lane;
    const int row = u >> 2, pc = (u & 3) ^ ((row >> 2) & 3);
    const int poff = (pc >> 1) * 48 + (pc & 1) * 16;  // (half, plane) within a 96-byte K16 chunk
    a_off[i] = row * arow + poff;
    b_off[i] = (co0 + row) * 96 + poff;
  }
  // step c's byte offset: c * 96 (input) / c * Cout * 96 (codebook)
  const int a_step = 96;
  const int b_step = p.Cout * 96;
  unsigned short* const a_dst = lds + (group * G_I + gw) * 512;
  unsigned short* const b_dst = lds + 3 * ABUF + (group * G_I + gw) * 512;
  auto dma_step = [&](int c, int, int slot) {  // (step, tap 0, ring slot)
    const int ao = c * a_step;
    const int bo = c * b_step;
#pragma unroll
    for (int i = 0; i < PW; ++i) dma16(rx, a_dst + slot * ABUF + i * 2048, a_off[i] + ao, 0);
#pragma unroll
    for (int i = 0; i < PW; ++i) dma16(rw, b_dst + slot * BBUF + i * 2048, b_off[i], bo);
    return 2 * PW;
  };

  const int lrow = lane & 31, h = lane >> 5;
  s16x8 af[TM][2], bfr[TN][2];
  auto readF = [&](int, int, int slot) {
    const unsigned short* A = lds + slot * ABUF;
    const unsigned short* Bs = lds + 3 * ABUF + slot * BBUF;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int r = wm * WR + i * 32 + lrow;
#pragma unroll
      for (int pl = 0; pl < 2; ++pl)
        af[i][pl] = *reinterpret_cast<const s16x8*>(A + r * RW + (((h * 2 + pl) ^ ((r >> 2) & 3)) << 3));
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = wn * WC + j * 32 + lrow;
#pragma unroll
      for (int pl = 0; pl < 2; ++pl)
        bfr[j][pl] = *reinterpret_cast<const s16x8*>(Bs + col * RW + (((h * 2 + pl) ^ ((col >> 2) & 3)) << 3));
    }
  };
  f32x16 acc[TM][TN];
  DCX_ZERO_ACC16(acc, TM, TN);
  auto mfma = [&]() {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        if constexpr (XMID)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[i][1]),
                                                              __builtin_bit_cast(bf16x8, bfr[j][0]), acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[i][0]),
                                                            __builtin_bit_cast(bf16x8, bfr[j][1]), acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[i][0]),
                                                            __builtin_bit_cast(bf16x8, bfr[j][0]), acc[i][j], 0, 0, 0);
      }
    __builtin_amdgcn_s_setprio(0);
  };

  // the schedule of conv_gemm_x6dm with taps = 1 (pingpong3_loop): every step brings its own tiles
  const StepPos l3 = pingpong3_prologue(nsteps, 1, dma_step);
  pingpong3_drain();
  DCX_CLOCK_BEGIN;
  pingpong3_loop<false>(group, nsteps, 1, l3, dma_step, readF, mfma);
  DCX_CLOCK_END(nsteps / 2);  // steps counted in units of vq_prefilter_x3's (K32: twice these)
  epilogue_top2<BM, BN, 4, WN>(p, acc, q0, co0, nt, ntiles, reinterpret_cast<float*>(lds));
}

// epilogue_top2 for 16x16 accumulator blocks (v_mfma_f32_16x16x32_bf16: lane l holds column
// l & 15 of its block, rows 4 (l >> 4) + r): the same per-row top 2 and lowest index on ties.
template <int BM, int BN, int WM, int WN>
__device__ __forceinline__ void epilogue_top2_q(const ConvParams& p, f32x4 (&acc)[BM / WM / 16][BN / WN / 16], int q0,
                                                int co0, int nt, int ntiles, float* smem) {
  constexpr int WR = BM / WM, WC = BN / WN;
  constexpr int TM = WR / 16, TN = WC / 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int lc = lane & 15, r4 = 4 * (lane >> 4);
  float xxv[TM][4], e2v[TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) xxv[i][r] = p.x2[min(q0 + wm * WR + i * 16 + r4 + r, p.Lq - 1)];
#pragma unroll
  for (int j = 0; j < TN; ++j) e2v[j] = p.e2[co0 + wn * WC + j * 16 + lc];
  __syncthreads();
  float* rv = smem;                                      // [WN][BM]
  float* rv2 = smem + WN * BM;                           // [WN][BM]
  int* ri = reinterpret_cast<int*>(smem + 2 * WN * BM);  // [WN][BM]
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rloc = wm * WR + i * 16 + r4 + r;
      const float xx = xxv[i][r];
      float v1 = __builtin_inff(), v2 = __builtin_inff();
      int i1 = 0x7fffffff;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        // a lane's codes come in increasing order, so a strict < keeps the lowest index on ties; the
        // second smallest is min(v2, max(v1, d2)) (top2_merge with one new value, in 5 VALU ops)
        const int co = co0 + wn * WC + j * 16 + lc;
        const float d2 = (xx + e2v[j]) + (-2.0f * acc[i][j][r]);
        i1 = d2 < v1 ? co : i1;
        v2 = fminf(v2, fmaxf(v1, d2));
        v1 = fminf(v1, d2);
      }
      top2_row16(v1, i1, v2);
      if (lc == 0) {
        rv[wn * BM + rloc] = v1;
        rv2[wn * BM + rloc] = v2;
        ri[wn * BM + rloc] = i1;
      }
    }
  }
  __syncthreads();
  for (int rloc = tid; rloc < BM; rloc += blockDim.x) {
    const int q = q0 + rloc;
    if (q >= p.Lq) continue;
    float v1 = rv[rloc], v2 = rv2[rloc];
    int i1 = ri[rloc];
#pragma unroll
    for (int w = 1; w < WN; ++w) top2_merge(v1, i1, v2, rv[w * BM + rloc], ri[w * BM + rloc], rv2[w * BM + rloc]);
    const long long o = (long long)q * ntiles + nt;
    p.part_val[o] = v1;
    p.part_val2[o] = v2;
    p.part_idx[o] = i1;
  }
}

// 64-byte LDS rows of vq_prefilter_b1: the 16-byte piece q of row r sits in slot q ^ b1_swz(r), with
// b1_swz(r) = (0, 2, 3, 1)[(r >> 2) & 3].  A ds_read_b128 is serviced in four 16-lane groups,
// {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32 (MI355X_MICROARCH.md §LDS), and lane l
// reads piece l >> 4 of row l & 15: this map gives the 16 lanes of every group 16 distinct bank quads.
// (Round 3's (r >> 2) & 3 paired up two lanes per quad in every group: 2-way conflicts, 46 % of the
// kernel's LDS cycles in PMC, SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE.)
__device__ __forceinline__ int b1_swz(int r) { return (0x1320 >> (((r >> 2) & 3) * 4)) & 3; }

// ---------------------------------------------------------------------------------------------
// vq_prefilter_b1: one bf16 product per term, x_h . e_h', in both arithmetic modes (round 3).
//
// The search only needs a candidate set that provably holds the nearest code; vq_rescore_kernel
// settles it exactly in fp64.  With x = x_h + x_r and e = e_h + d (x_h, e_h the RNE bf16 values),
// x.e - x_h.e_h = x_r.e + x_h.d, so by Cauchy-Schwarz the dropped terms are at most
// |x_r| max|e| + |x_h| max|d|, where max|d| (0.17 % of max|e| on the synthetic codebook) is
// measured once at load and |x_r| per row by row_sqnorm (zero in bf16 mode).  That bound is
// looser than vq_prefilter_dm's (3 products), so more rows go on to the
// rescore (about 60-95 % instead of 10 %, 3-7 candidates each), but the distance GEMM, 99 % of the
// search's MFMA work, issues 1/3 (x6) or 1/2 (bf16) of the products.
//
// One v_mfma_f32_16x16x32_bf16 per 16 x 16 block and K32 step (lanes l >> 4 = 0..3 read the four
// 16-byte pieces of 8 channels).  Both operands arrive as 64-byte runs per row / code and step:
// x_pjt_in compact ([rows][CD] bf16, the project_in epilogue's LAYOUT_BF16 output) and the
// codebook as compact_pack (dcx_api.cpp) packs it ([CD/32][NC][32] bf16).  LDS images: 64-byte
// rows, piece q in slot q ^ b1_swz(row), conflict-free for the four lane groups of a ds_read_b128.
// Ring: NS slots of 16 + 16 KiB on the ping-pong schedule of vq_prefilter_dm generalised to NS slots
// and K32 steps: step t is issued by group 0 in MEM0(t - NS) and by
// group 1 in MEM1(t - NS + 1), and each wave retires its pieces NS - 2 memory segments later.
// ---------------------------------------------------------------------------------------------
template <int NS>
__global__ void __launch_bounds__(512, 2) vq_prefilter_b1(const ConvParams p) {
  constexpr int BM = 256, BN = 256, WN = 2;
  constexpr int WR = BM / 4, WC = BN / 2, TM = WR / 16, TN = WC / 16;
  DCX_TILET(tile_t0);
  constexpr int RW = 32;                       // ushorts per LDS row (64 bytes)
  constexpr int A_G = BM * 4 / 64 / 2;         // DMA instructions per group per tile (8)
  constexpr int B_G = BN * 4 / 64 / 2;         // (8)
  constexpr int A_PW = A_G / 4, B_PW = B_G / 4;  // per wave (2 + 2)
  constexpr int P = A_PW + B_PW;
  constexpr int ABUF = BM * RW, BBUF = BN * RW;
  constexpr int LDS_US = NS * (ABUF + BBUF);   // NS * 32 KiB
  static_assert(A_G % 4 == 0 && B_G % 4 == 0 && LDS_US * 2 <= 160 * 1024 && NS >= 3, "tile shape");
  static_assert(P * (NS - 1) <= 23, "wait_dma range");
  __shared__ __attribute__((aligned(16))) unsigned short lds[LDS_US];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int group = __builtin_amdgcn_readfirstlane(tid >> 8);
  const int gw = __builtin_amdgcn_readfirstlane((tid >> 6) & 3);
  const int wm = wave >> 1, wn = wave & 1;
  const int ntiles = p.Cout / BN, mtiles = (p.Lq + BM - 1) / BM;
  int mt, nt;
  vq_tile(mtiles, ntiles, mt, nt);
  if (mt >= mtiles) return;  // whole workgroup, before any barrier
  const int q0 = mt * BM, co0 = nt * BN;
  const int nsteps = p.Cin / 32;
  const int arow = p.ldx * 2;  // bytes per compact row
#ifdef DCX_VQ_DIAG_L2  // timing build: every tile loads row panel 0 and code tile 0 (L2-resident operands)
  const int lq0 = 0, lco0 = 0;
#else
  const int lq0 = q0, lco0 = co0;
#endif
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(p.x6 + (long long)lq0 * p.ldx), 0, min(BM, p.Lq - lq0) * arow, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)p.wc, 0, nsteps * p.Cout * 64, 0x00020000);

  int a_off[A_PW], b_off[B_PW];
#pragma unroll
  for (int i = 0; i < A_PW; ++i) {
    const int u = (group * A_G + i * 4 + gw) * 64 + lane;
    const int row = u >> 2, pc = (u & 3) ^ b1_swz(row);
    a_off[i] = row * arow + pc * 16;
  }
#pragma unroll
  for (int i = 0; i < B_PW; ++i) {
    const int u = (group * B_G + i * 4 + gw) * 64 + lane;
    const int code = u >> 2, pc = (u & 3) ^ b1_swz(code);
    b_off[i] = (lco0 + code) * 64 + pc * 16;
  }
  unsigned short* const a_dst = lds + (group * A_G + gw) * 512;
  unsigned short* const b_dst = lds + NS * ABUF + (group * B_G + gw) * 512;
  auto dma_step = [&](int c, int slot) {
#pragma unroll
    for (int i = 0; i < A_PW; ++i) dma16(rx, a_dst + slot * ABUF + i * 2048, a_off[i] + c * 64, 0);
#pragma unroll
    for (int i = 0; i < B_PW; ++i) dma16(rw, b_dst + slot * BBUF + i * 2048, b_off[i], c * p.Cout * 64);
  };

  // lane roles: row / code l & 15 of a 16-block, piece (8 channels) q = l >> 4
  const int l16 = lane & 15, pq = lane >> 4;
  s16x8 af[TM], bfr[TN];
  auto readF = [&](int slot) {
    const unsigned short* A = lds + slot * ABUF;
    const unsigned short* Bs = lds + NS * ABUF + slot * BBUF;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int r = wm * WR + i * 16 + l16;
      af[i] = *reinterpret_cast<const s16x8*>(A + r * RW + ((pq ^ b1_swz(r)) << 3));
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = wn * WC + j * 16 + l16;
      bfr[j] = *reinterpret_cast<const s16x8*>(Bs + col * RW + ((pq ^ b1_swz(col)) << 3));
    }
  };
  f32x4 acc[TM][TN];
  zero_acc(acc);
  auto mfma = [&]() {
#ifdef DCX_VQ_STATICPRIO  // A/B: group 1 at priority 1 throughout, no per-segment flips (MI355X_MICROARCH.md
                          // "Two waves per SIMD" item 4); the MFMA cluster fenced for the scheduler instead
    __builtin_amdgcn_sched_barrier(0);
#else
    __builtin_amdgcn_s_setprio(1);
#endif
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[i]),
                                                            __builtin_bit_cast(bf16x8, bfr[j]), acc[i][j], 0, 0, 0);
#ifdef DCX_VQ_STATICPRIO
    __builtin_amdgcn_sched_barrier(0);
#else
    __builtin_amdgcn_s_setprio(0);
#endif
  };
  // pieces this wave may leave in flight at the end of a memory segment: its shares of the steps
  // after the ones the next two segments read (lo..hi inclusive, clipped to the steps that exist)
  auto in_flight = [&](int lo, int hi) { return P * max(0, min(hi, nsteps - 1) - lo + 1); };

  for (int t = 0; t < NS && t < nsteps; ++t) dma_step(t, t);
  // group 0 reads step 0 now and step 1 in segment 1 (its own MFMA segment 0 comes first)
  wait_dma(group == 0 ? in_flight(2, NS - 1) : in_flight(1, NS - 1));
#ifdef DCX_TILE_DIAG
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (timing build: the prologue's DMA landed)
#endif
  DCX_TILET(tile_t1);
#ifdef DCX_VQ_STATICPRIO
  if (group == 1) __builtin_amdgcn_s_setprio(1);
#endif
  seg_barrier();
#ifdef DCX_SEG_DIAG
  unsigned long long sd[5] = {};  // per step: mfma issue, barrier, reads + DMA issue, DMA wait, barrier
#endif
  if (group == 0) {
    readF(0);
    int rs = 1, ws = 0;
    for (int s = 0; s < nsteps; ++s) {
      DCX_SEGT(ta);
      mfma();  // MFMA(s)
      DCX_SEGT(tb);
      seg_barrier();
      DCX_SEGT(tc);
      if (s + 1 < nsteps) readF(rs);  // MEM0(s): fragments of step s + 1, issue step s + NS
      if (s + NS < nsteps) dma_step(s + NS, ws);
      DCX_SEGT(td);
      wait_dma(in_flight(s + 3, s + NS));
      DCX_SEGT(te);
      seg_barrier();
      DCX_SEGT(tf);
#ifdef DCX_SEG_DIAG
      sd[0] += tb - ta; sd[1] += tc - tb; sd[2] += td - tc; sd[3] += te - td; sd[4] += tf - te;
#endif
      ring_inc<NS>(rs);
      ring_inc<NS>(ws);
    }
  } else {
    int rs = 0, ws = 0;
    for (int s = 0; s < nsteps; ++s) {
      DCX_SEGT(ta);
      readF(rs);  // MEM1(s): fragments of step s, issue step s + NS - 1 (s >= 1)
      if (s >= 1 && s + NS - 1 < nsteps) dma_step(s + NS - 1, ws);
      DCX_SEGT(tb);
      wait_dma(in_flight(s + 2, s >= 1 ? s + NS - 1 : NS - 1));
      DCX_SEGT(tc);
      seg_barrier();
      DCX_SEGT(td);
      mfma();  // MFMA(s)
      DCX_SEGT(te);
      seg_barrier();
      DCX_SEGT(tf);
#ifdef DCX_SEG_DIAG
      sd[0] += te - td; sd[1] += tf - te; sd[2] += tb - ta; sd[3] += tc - tb; sd[4] += td - tc;
#endif
      ring_inc<NS>(rs);
      ring_inc_issue1<NS>(ws, s);
    }
  }
#ifdef DCX_SEG_DIAG
  if ((threadIdx.x & 255) == 0) {
#pragma unroll
    for (int i = 0; i < 5; ++i) atomicAdd(&g_seg_diag[group * 6 + i], sd[i]);
    if (group == 0) atomicAdd(&g_seg_diag[12], (unsigned long long)nsteps);
  }
#endif
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  DCX_TILET(tile_t2);
  epilogue_top2_q<BM, BN, 4, WN>(p, acc, q0, co0, nt, ntiles, reinterpret_cast<float*>(lds));
  DCX_TILE_END(nsteps);
}

// ---------------------------------------------------------------------------------------------
// launcher
// ---------------------------------------------------------------------------------------------
// code tile of the x6-mode prefilter: 256 (vq_prefilter_dm) where its shape limits hold, else 128
static bool vq_dm_ok(int ncodes, int dim) {
#ifdef DCX_NO_VQDM
  return false;
#endif
  return ncodes % (256 * 16) == 0 && dim % BK == 0 && dim / BK >= 3 && (long long)dim * 6 * 256 < (1ll << 31) &&
         (long long)(dim / BK) * ncodes * 96 < (1ll << 31);
}
// Code tile of the prefilter launch_vq_prefilter picks: 256 for vq_prefilter_b1 / vq_prefilter_dm, 128
// for vq_prefilter_x3 (planes x_pjt_in where vq_prefilter_dm's limits fail).  (Routing searches of one
// row panel, a streaming hop, to the 128-code tiles for twice the workgroups measured 1.55 -> 2.55 ms.)
int vq_prefilter_ntiles(int ncodes, int dim, Layout x_layout) {
  return ncodes / (x_layout == LAYOUT_BF16 || vq_dm_ok(ncodes, dim) ? 256 : 128);
}

// vq_prefilter_b1's ring depth (slots of 32 KiB; DCX_VQ_NS=3..5 in A/B builds)
#ifndef DCX_VQ_NS
#define DCX_VQ_NS 4
#endif
bool vq_b1_takes(int ncodes, int dim) {
  return ncodes % (256 * 16) == 0 && dim % 32 == 0 && dim / 32 >= DCX_VQ_NS && (long long)dim * 2 * 256 < (1ll << 31) &&
         (long long)(dim / 32) * ncodes * 64 < (1ll << 31);
}

// The bf16x3 prefilters on planes (vq_prefilter_dm / _x3).  With x = h + m + l per operand
// (dcx_planes.h, u = 2^-8), dropping h*l', m*m', l*h' and smaller leaves an error <= 3.1 u^2
// sum_k |x_k e_k| (4.7e-5); fp32 accumulation of 672 MFMA partial sums adds <= 2688 * 2^-24 (1.6e-4,
// allowing 4 roundings per MFMA).  By Cauchy-Schwarz sum_k |x_k e_k| <= |x| max|e|, so each
// approximate squared distance is within 2 * kVqPrefilterBound * |x| max|e| + 8 * 2^-24 (|x|^2 +
// max|e|^2) of the exact one; vq_rescore_kernel uses that bound.
// vq_prefilter_b1 (LAYOUT_BF16): x.e - x_h.e_h = x_r.e + x_h.d with
// |x_r.e| <= |x_r| max|e| (the rescore's second term) and |x_h.d| <= |x_h| max|d| <= (1 + 2^-8)|x| dmax;
// fp32 summation of the dim exact products, in whatever order the MFMAs add them, errs by at most
// dim 2^-24 sum_k |x_h,k e_h,k| <= dim 2^-24 (1 + 2^-8)^2 |x| max|e|.
double vq_prefilter_cx(Layout x_layout, int ncodes, int dim, float emax, float dmax) {
  if (x_layout != LAYOUT_BF16 || !vq_b1_takes(ncodes, dim)) return (double)kVqPrefilterBound * emax;
  return (1.0 + 0x1p-8) * (double)dmax + (double)dim * 0x1p-24 * (1.0 + 0x1p-6) * (double)emax;
}

// compact x_pjt_in (either mode) with the [CD/32][NC][32] hi codebook p.wc: vq_prefilter_b1; planes
// with the planes codebook p.w6: vq_prefilter_dm where vq_dm_ok, else vq_prefilter_x3
hipError_t launch_vq_prefilter(const ConvParams& p, int rows, bool x_bf16, hipStream_t s, const char** kname) {
  constexpr int BM = 256, BN = 128;
  if (!p.x6 || !p.part_val2 || rows < 1 || (p.x_layout != LAYOUT_PLANES && p.x_layout != LAYOUT_BF16)) return hipErrorInvalidValue;
  ConvParams q = p;
  q.Lq = rows;
  q.Lin = rows;
  q.taps = 1;
  const dim3 grid256(vq_grid((rows + 255) / 256, p.Cout / 256));  // the 256 x 256 tiles of _b1 and _dm
  if (p.x_layout == LAYOUT_BF16) {
    if (!p.wc || !vq_b1_takes(p.Cout, p.Cin)) return hipErrorInvalidValue;
    if (kname) *kname = "vq_prefilter_b1<256,256>";
    hipLaunchKernelGGL(vq_prefilter_b1<DCX_VQ_NS>, grid256, dim3(512), 0, s, q);
    return hipGetLastError();
  }
  if (!p.w6 || p.Cin % BK || p.Cout % (BN * 16)) return hipErrorInvalidValue;
  if (vq_dm_ok(p.Cout, p.Cin)) {
    if (kname) *kname = x_bf16 ? "vq_prefilter_dm_x2<256,256>" : "vq_prefilter_dm<256,256>";
    if (x_bf16) hipLaunchKernelGGL((vq_prefilter_dm<false>), grid256, dim3(512), 0, s, q);
    else hipLaunchKernelGGL((vq_prefilter_dm<true>), grid256, dim3(512), 0, s, q);
    return hipGetLastError();
  }
  const dim3 grid(vq_grid((rows + BM - 1) / BM, p.Cout / BN));
  if (p.Cin % 64) return hipErrorInvalidValue;  // even number of K32 steps
  if (x_bf16) {
    if (kname) *kname = "vq_prefilter_x2<256,128>";
    hipLaunchKernelGGL((vq_prefilter_x3<BM, BN, 4, 2, false>), grid, dim3(512), 0, s, q);
  } else {
    if (kname) *kname = "vq_prefilter_x3<256,128>";
    hipLaunchKernelGGL((vq_prefilter_x3<BM, BN, 4, 2, true>), grid, dim3(512), 0, s, q);
  }
  return hipGetLastError();
}

}  // namespace dcx
