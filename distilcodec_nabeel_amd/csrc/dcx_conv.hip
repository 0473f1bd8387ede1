// Implicit-GEMM 1-D convolution on gfx950 matrix cores.
//
// One kernel family serves every contraction on the DistilCodec path:
//   Conv1d k>1 / dilated (stem k7, conv_pre k13, ResBlock1 k3/7/11 x dil 1/3/5),
//   1x1 convs and nn.Linear (taps = 1), ConvTranspose1d as `stride` polyphase convs
//   (one tile range per phase, flat_tile), the STFT as a 4-tap conv over 256-sample rows, the mel matmul,
//   and the VQ distance GEMM (argmin epilogue, never materialising rows x 32768).
//
// GEMM view: rows = output time positions q (M), cols = output channels (N),
// K = taps x Cin.  Channels-last activations make every A-tile row a contiguous Cin slice and
// every store a contiguous Cout slice (coalesced).
//
// Two arithmetic modes, identical epilogues:
//  * conv_gemm_f32: v_mfma_f32_32x32x2_f32 (exact fp32 fmaf chain, 157 TF peak).
//  * conv_gemm_x6:  fp32-accurate 3-plane bf16 split.  Every fp32 operand x is held as
//    x = hi + mid + lo (three bf16, RNE; residual <= 2^-27|x|) and a product uses the six terms
//    hi*hi + hi*mid + mid*hi + hi*lo + mid*mid + lo*hi, each exact in fp32 (8x8-bit
//    significands), accumulated in fp32 by v_mfma_f32_32x32x16_bf16.  The dropped terms are
//    <= 2^-24 relative, i.e. fp32 rounding level; the MFMA ceiling is 16/6 = 2.67x the fp32 one.
//    Weights are split once at load; activations arrive already split (every producer writes
//    the planes, dcx_planes.h), so staging is a plain copy, and each staged input tile (with its
//    tap halo) serves every tap of the conv.
//
// MFMA fragment maps (cdna_hip_programming.md §3): 32x32x2 f32: lane l supplies A[l&31][k=l>>5]
// and B[k=l>>5][l&31]; 32x32x16 bf16: A[l&31][k=8(l>>5)+j], B[k=8(l>>5)+j][l&31], j<8;
// C/D for both: col=l&31, row=(r&3)+8*(r>>2)+4*(l>>5).
//
// Files: this one holds conv_gemm_f32 (with the exact VQ argmin), the bf16-mode 1x1 kernels, the split-K
// reduce kernels and the dispatch (launch_conv and its grouped forms); the x6 and h3 kernels with their
// launchers are in dcx_conv_x6w8.hip, dcx_conv_x6.hip and dcx_conv_h3.hip (dcx_conv_launch.h), the VQ
// prefilters in dcx_conv_vq.hip, the device code they share in dcx_conv_common.h.
#include <cstdlib>
#include <mutex>

#include "dcx_conv_common.h"
#include "dcx_conv_launch.h"
#include "dcx_conv_pingpong.h"

namespace dcx {

// The bf16 mode's GELU as a table (round 4).  Its input is a bf16 value (the GEMM result rounded
// after the bias) and its output is rounded to bf16 by the store, so GELU + rounding is a function
// of 16 bits.  conv_gemm_bf16dp tabulates it once per workgroup in LDS with gelu_bf16_f2 itself (so
// an entry is the evaluated result's bits) over the magnitudes [2^-31, 2^16): entry
// 2 (m - kGeluLo) + s = GELU of the bf16 (s << 15) | m, entry 2 kGeluN a sentinel that inputs
// outside the table read.  An element then costs half a packed convert, five packed 16-bit ops shared
// by two elements and a ds_read_u16, against ~18 VALU instructions evaluated (the pwconv1 epilogues
// were bound by that VALU work: 11.6 of their 28.7 ms per C3 step, DCX_DIAG_DUP).  A wave with an
// input outside the table (zeros, |x| < 2^-31 or >= 2^16, inf, NaN) stores the evaluated epilogue.
constexpr int kBf16dpBiasMax = 4096;  // conv_gemm_bf16dp: Cout bound (its bias lives in LDS)
constexpr int kGeluLo = 96 << 7, kGeluN = 47 << 7;  // bf16 magnitude bits [0x3000, 0x4780)
constexpr int kGeluLutUs = (2 * kGeluN + 1 + 7) / 8 * 8;  // ushorts, 16-byte multiple
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void gelu_lut_fill(unsigned short* lut, int tid, int nthreads) {
  for (int i = 2 * tid; i < 2 * kGeluN; i += 2 * nthreads) {  // (s = 0, s = 1) pairs of one m
    const int m = kGeluLo + (i >> 1);
    const f32x2 g = gelu_bf16_f2(f32x2{bf16_val((unsigned short)m), bf16_val((unsigned short)(0x8000 | m))});
    lut[i] = bf16_bits(g[0]);
    lut[i + 1] = bf16_bits(g[1]);
  }
  if (tid == 0) lut[2 * kGeluN] = 0xffff;
}
// GELU bits of two values rounded to bf16 here (the RNE of round_bf16x4) from the table at LDS byte
// address 0; `hi` keeps the largest table offset seen (>= 2 kGeluN: outside the table)
__device__ __forceinline__ unsigned gelu_lut2(const unsigned short* lut, f32x2 x, u16x2& hi) {
  const u16x2 r = __builtin_bit_cast(u16x2, __builtin_convertvector(x, bf16x2));
  const u16x2 key = (r << (unsigned short)1) | (r >> (unsigned short)15);  // 2 m + s
  const u16x2 t = key - (unsigned short)(2 * kGeluLo);                     // wraps below the table
  hi = __builtin_elementwise_max(hi, t);
  const u16x2 tc = __builtin_elementwise_min(t, u16x2{(unsigned short)(2 * kGeluN), (unsigned short)(2 * kGeluN)});
  const unsigned a = __builtin_bit_cast(unsigned, (u16x2)(tc << (unsigned short)1));  // byte offsets
#ifdef DCX_LUT_DIAG  // timing build: the table lookups left out (wrong results)
  return a ^ __builtin_bit_cast(unsigned, r);
#endif
  const char* const lb = reinterpret_cast<const char*>(lut);
  const unsigned lo16 = *reinterpret_cast<const unsigned short*>(lb + (a & 0xffff));
  const unsigned hi16 = *reinterpret_cast<const unsigned short*>(lb + (a >> 16));
  return lo16 | (hi16 << 16);
}

DCX_DIAG_FILE(conv)

#ifdef DCX_DIAG
// the diagnostic counters of every kernel file (DCX_DIAG_FILE): sums, or (DIAG_TILES) the stamps of
// one file after the other, returning how many
static int diag_all(int set, unsigned long long* out, int n, int reset) {
  int (*const files[])(int, unsigned long long*, int, int) = {diag_conv, diag_vq, diag_x6w8, diag_x6, diag_h3};
  int got = 0;
  if (set != DIAG_TILES) std::fill(out, out + n, 0ull);
  for (auto f : files) {
    const int r = f(set, out + 6 * got, n - got, reset);  // (counter sets return 0: got stays 0)
    if (r < 0) return -1;
    got += r;
  }
  return got;
}
#endif
#ifdef DCX_CLOCK_DIAG
extern "C" int dcx_diag_clock(unsigned long long* out3, int reset) { return diag_all(DIAG_CLOCK, out3, 3, reset) < 0 ? -1 : 0; }
#endif
#ifdef DCX_SEG_DIAG
extern "C" int dcx_diag_seg(unsigned long long* out13, int reset) { return diag_all(DIAG_SEG, out13, 13, reset) < 0 ? -1 : 0; }
extern "C" int dcx_diag_seg8(unsigned long long* out49, int reset) { return diag_all(DIAG_SEG8, out49, 49, reset) < 0 ? -1 : 0; }
#endif
#ifdef DCX_TILE_DIAG
extern "C" int dcx_diag_tiles(unsigned long long* out, int max_tiles, int reset) { return diag_all(DIAG_TILES, out, max_tiles, reset); }
#endif

// ---------------------------------------------------------------------------------------------
// Split-K reduce: v = bias + sum of the K-slices' partial sums (in slice order), then the epilogue
// of epilogue_lds element by element (one thread per 4 output channels of a row).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void splitk_epi4(const ConvParams& p, const float* __restrict__ part, int splits,
                                            long long stride, long long i4) {
  const int c4n = p.Cout / 4;
  const long long rowi = i4 / c4n;  // (phase, clip, q)
  const int co = (int)(i4 - rowi * c4n) * 4;
  const long long per_ph = (long long)p.batch * p.Lq;
  const int ph = (int)(rowi / per_ph);
  const long long r2 = rowi - ph * per_ph;
  const int b = (int)(r2 / p.Lq), q = (int)(r2 - (long long)b * p.Lq);
  const long long ob = (long long)b * p.y_bstride;
  const long long orow = (long long)q * p.out_mul + ph;
  const long long o = ob + orow * p.ldy + co;
  f32x4 x = *reinterpret_cast<const f32x4*>(part + o);
  for (int s = 1; s < splits; ++s) x += *reinterpret_cast<const f32x4*>(part + s * stride + o);
  if (p.bias) x += *reinterpret_cast<const f32x4*>(p.bias + co);
  if (p.round_bf16) x = round_bf16x4(x);
  switch (p.epi) {
    case EPI_GELU:
#pragma unroll
      for (int e = 0; e < 4; ++e) x[e] = p.w6 ? gelu_bf16_f(x[e]) : gelu_f(x[e]);
      if (p.round_bf16) x = round_bf16x4(x);
      break;
    case EPI_GAMMA_RES:
      x = *reinterpret_cast<const f32x4*>(p.res + o) + *reinterpret_cast<const f32x4*>(p.gamma + co) * x;
      break;
    case EPI_RES: x = *reinterpret_cast<const f32x4*>(p.res + o) + x; break;
    case EPI_LOGCLAMP:
#pragma unroll
      for (int e = 0; e < 4; ++e) x[e] = logf(fmaxf(x[e], 1e-5f));
      break;
    default: break;
  }
  if (p.mean_mode == MEAN_FIRST) {
    *reinterpret_cast<f32x4*>(p.macc + o) = x;
    return;
  } else if (p.mean_mode == MEAN_MID) {
    *reinterpret_cast<f32x4*>(p.macc + o) = *reinterpret_cast<const f32x4*>(p.macc + o) + x;
    return;
  } else if (p.mean_mode == MEAN_LAST) {
    x = (*reinterpret_cast<const f32x4*>(p.macc + o) + x) / 3.0f;
  }
  if (p.y) *reinterpret_cast<f32x4*>(p.y + o) = x;
  // h2 outputs (not produced in the split-K mode, which runs no h3 conv; kept consistent): the clip's
  // range scale (epilogue_lds); no maxima are recorded here
  const float osc = (p.y6 && p.y_layout == LAYOUT_H2) || (p.y6s && p.ys_layout != LAYOUT_PLANES)
                        ? __builtin_ldexpf(1.0f, h2_shift(range_bound(p.yb, b))) : 1.0f;
  if (p.y6) {
    unsigned short* y6 = p.y6 + ob * layout_u16(p.y_layout);
    if (p.y_layout == LAYOUT_BF16) store_bf16x4(y6, orow, p.Cout, co, x[0], x[1], x[2], x[3]);
    // unreachable (run_conv rejects layout 2); kept: removing it moved registers / scratch in other kernels
    else if ((int)p.y_layout == 2) store_hm4(y6, orow, p.Cout, co, x[0], x[1], x[2], x[3]);
    else if (p.y_layout == LAYOUT_H2) store_h2_4(y6, orow, p.Cout, co, x[0], x[1], x[2], x[3], osc);
    else store_planes4(y6, orow, p.Cout, co, x[0], x[1], x[2], x[3]);
  }
  if (p.y2 || p.y6s) {
    f32x4 sv;
#pragma unroll
    for (int e = 0; e < 4; ++e) sv[e] = silu_f(x[e]);
    if (p.y2) *reinterpret_cast<f32x4*>(p.y2 + o) = sv;
    if (p.y6s && p.ys_layout != LAYOUT_PLANES) store_h2_4(p.y6s + ob * 2, orow, p.Cout, co, sv[0], sv[1], sv[2], sv[3], osc);
    else if (p.y6s) store_planes4(p.y6s + ob * 3, orow, p.Cout, co, sv[0], sv[1], sv[2], sv[3]);
  }
}

__global__ void __launch_bounds__(256) splitk_epilogue_kernel(const ConvParams p, const float* __restrict__ part,
                                                              int splits, long long stride, long long total4) {
  const long long i4 = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i4 < total4) splitk_epi4(p, part, splits, stride, i4);
}

// the reduces of a grouped split-K launch in one grid (member k: blocks [start[k], start[k + 1]))
__global__ void __launch_bounds__(256) splitk_epilogue_group_kernel(const SplitEpiGroup g) {
  const int t = blockIdx.x;
  const int k = member_index(g, t);
  const long long i4 = (long long)(t - g.start[k]) * 256 + threadIdx.x;
  if (i4 >= g.total4[k]) return;
  if (g.chain) {  // g.chain members, one range of blocks (member 0's), every member in order
    splitk_epi4(g.p[0], g.part[0], g.splits[0], g.stride[0], i4);
    if (g.chain > 1) splitk_epi4(g.p[1], g.part[1], g.splits[1], g.stride[1], i4);
    if (g.chain > 2) splitk_epi4(g.p[2], g.part[2], g.splits[2], g.stride[2], i4);
    return;
  }
  if (k == 0) splitk_epi4(g.p[0], g.part[0], g.splits[0], g.stride[0], i4);
  else if (k == 1) splitk_epi4(g.p[1], g.part[1], g.splits[1], g.stride[1], i4);
  else splitk_epi4(g.p[2], g.part[2], g.splits[2], g.stride[2], i4);
}

// ---------------------------------------------------------------------------------------------
// VQ search epilogue (registers): per-row argmin of the distance tile.
// ---------------------------------------------------------------------------------------------
template <int BM, int BN, int WM, int WN, bool ARGMIN>
__device__ __forceinline__ void epilogue(const ConvParams& p, f32x16 (&acc)[BM / WM / 32][BN / WN / 32], int q0,
                                         int co0, int nt, int ntiles, int b, int ph, float* smem) {
  constexpr int WR = BM / WM, WC = BN / WN;
  constexpr int TM = WR / 32, TN = WC / 32;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int lrow = lane & 31;
  const int rhalf = 4 * (lane >> 5);
  static_assert(ARGMIN, "register epilogue is the VQ search's; convs use epilogue_lds");
  {
    // VQ search: dist = sqrt(clamp((|x|^2 + |e|^2) + (-2 x.e), 0)) exactly in the reference's
    // operation order (vector_quantize_pytorch.py:41-45); per row keep the smallest distance,
    // lowest code index on ties (torch argmax of -dist returns the first).
    __syncthreads();
    float* rv = smem;                                  // [WN][BM]
    int* ri = reinterpret_cast<int*>(smem + WN * BM);  // [WN][BM]
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rloc = wm * WR + i * 32 + (r & 3) + 8 * (r >> 2) + rhalf;
        const int q = q0 + rloc;
        const float xx = (q < p.Lq) ? p.x2[(long long)b * p.Lq + q] : 0.f;
        float bv = __builtin_inff();
        int bi = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int co = co0 + wn * WC + j * 32 + lrow;
          const float d2 = (xx + p.e2[co]) + (-2.0f * acc[i][j][r]);
          const float d = sqrtf(fmaxf(d2, 0.0f));
          if (d < bv || (d == bv && co < bi)) { bv = d; bi = co; }
        }
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) {
          const float ov = __shfl_xor(bv, off, 64);
          const int oi = __shfl_xor(bi, off, 64);
          if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (lrow == 0) { rv[wn * BM + rloc] = bv; ri[wn * BM + rloc] = bi; }
      }
    }
    __syncthreads();
    for (int rloc = tid; rloc < BM; rloc += 256) {
      const int q = q0 + rloc;
      if (q >= p.Lq) continue;
      float bv = rv[rloc];
      int bi = ri[rloc];
#pragma unroll
      for (int w = 1; w < WN; ++w) {
        const float ov = rv[w * BM + rloc];
        const int oi = ri[w * BM + rloc];
        if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
      }
      const long long o = ((long long)b * p.Lq + q) * ntiles + nt;
      p.part_val[o] = bv;
      p.part_idx[o] = bi;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// fp32 MFMA kernel.  Register-staged double buffer, one barrier per 16-deep K chunk.
// ---------------------------------------------------------------------------------------------
template <int BM, int BN, int WM, int WN, bool ARGMIN>
__global__ void __launch_bounds__(256) conv_gemm_f32(const ConvParams p) {
  static_assert(WM * WN == 4, "4 waves per workgroup");
  constexpr int WR = BM / WM, WC = BN / WN;
  constexpr int TM = WR / 32, TN = WC / 32;
  static_assert(TM >= 1 && TN >= 1 && WR % 32 == 0 && WC % 32 == 0, "wave tile");
  constexpr int A_F4 = BM * (BK / 4), B_F4 = BN * (BK / 4);
  constexpr int A_PT = (A_F4 + 255) / 256, B_PT = (B_F4 + 255) / 256;

  __shared__ __attribute__((aligned(16))) float smem[2 * (BM + BN) * LDSK];
  float(*As)[BM][LDSK] = reinterpret_cast<float(*)[BM][LDSK]>(smem);
  float(*Bs)[BN][LDSK] = reinterpret_cast<float(*)[BN][LDSK]>(smem + 2 * BM * LDSK);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int ntiles = p.Cout / BN;
  int wg, b, ph;
  flat_tile(((p.Lq + BM - 1) / BM) * ntiles, p.batch, wg, b, ph);
  const int mt = wg / ntiles, nt = wg - mt * ntiles;
  const int q0 = mt * BM, co0 = nt * BN;
  const float* __restrict__ xb = p.x + (long long)b * p.x_bstride;
  const float* __restrict__ wp = p.w + (long long)ph * p.w_phase_stride + (long long)co0 * p.taps * p.Cin;
  const int inb = p.in_base[ph];
  const int kchunks = p.Cin / BK;
  const int nk = p.taps * kchunks;
  const long long wrow = (long long)p.taps * p.Cin;

  f32x4 ra[A_PT], rb[B_PT];

  auto gload = [&](int kt) {
    const int m = kt / kchunks;
    const int ci0 = (kt - m * kchunks) * BK;
    const int shift = inb + m * p.in_step;
#pragma unroll
    for (int i = 0; i < A_PT; ++i) {
      const int idx = tid + 256 * i;
      ra[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (A_F4 % 256 == 0 || idx < A_F4) {
        const int row = idx >> 2, c4 = idx & 3;
        const int q = q0 + row, ir = q + shift;
        if (q < p.Lq && ir >= 0 && ir < p.Lin)
          ra[i] = *reinterpret_cast<const f32x4*>(xb + (long long)ir * p.ldx + ci0 + c4 * 4);
      }
    }
#pragma unroll
    for (int i = 0; i < B_PT; ++i) {
      const int idx = tid + 256 * i;
      if (B_F4 % 256 == 0 || idx < B_F4) {
        const int row = idx >> 2, c4 = idx & 3;
        rb[i] = *reinterpret_cast<const f32x4*>(wp + (long long)row * wrow + m * p.Cin + ci0 + c4 * 4);
      }
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < A_PT; ++i) {
      const int idx = tid + 256 * i;
      if (A_F4 % 256 == 0 || idx < A_F4) *reinterpret_cast<f32x4*>(&As[buf][idx >> 2][(idx & 3) * 4]) = ra[i];
    }
#pragma unroll
    for (int i = 0; i < B_PT; ++i) {
      const int idx = tid + 256 * i;
      if (B_F4 % 256 == 0 || idx < B_F4) *reinterpret_cast<f32x4*>(&Bs[buf][idx >> 2][(idx & 3) * 4]) = rb[i];
    }
  };

  f32x16 acc[TM][TN];
  DCX_ZERO_ACC16(acc, TM, TN);

  gload(0);
  sstore(0);
  __syncthreads();

  const int kof = (lane >> 5) * 8;
  const int lrow = lane & 31;
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) gload(kt + 1);
    f32x4 a0[TM], a1[TM], b0[TN], b1[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const float* ap = &As[buf][wm * WR + i * 32 + lrow][kof];
      a0[i] = *reinterpret_cast<const f32x4*>(ap);
      a1[i] = *reinterpret_cast<const f32x4*>(ap + 4);
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const float* bp = &Bs[buf][wn * WC + j * 32 + lrow][kof];
      b0[j] = *reinterpret_cast<const f32x4*>(bp);
      b1[j] = *reinterpret_cast<const f32x4*>(bp + 4);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[i][s], b0[j][s], acc[i][j], 0, 0, 0);
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[i][s], b1[j][s], acc[i][j], 0, 0, 0);
    if (kt + 1 < nk) sstore(buf ^ 1);
    __syncthreads();
  }
  if constexpr (ARGMIN)
    epilogue<BM, BN, WM, WN, true>(p, acc, q0, co0, nt, ntiles, b, ph, smem);
  else
    epilogue_lds<BM, BN, WM, WN, 2 * (BM + BN) * LDSK, 256>(p, p, acc, q0, co0, b, ph, smem);
}

// ---------------------------------------------------------------------------------------------
// conv_gemm_bf16dm: the DCX_GEMM_BF16 mode's 1x1 convs (one hi * hi' product, the reference's
// enable_bfloat16 autocast) on the LDS-DMA ping-pong schedule of conv_gemm_x6dm.
//
// A step is K32 (two K16 chunks, hi planes only: 4 pieces of 16 B per row), 16x16x32 MFMAs on
// 64 x 128 wave tiles: 32 MFMAs against 12 fragment reads per segment.  A and B ride one 3-slot
// ring (step t in slot t % 3, 16 + 16 KiB per slot), issued by group 0 in MEM0(t - 3) and group 1
// in MEM1(t - 2) and retired one memory segment later.  LDS images: 16-row blocks, piece-major
// (16-byte unit (r >> 4) * 64 + piece * 16 + (r & 15), piece = 8-channel group of the step).
// ---------------------------------------------------------------------------------------------
//
// REG (round 3): launches whose epilogue is bias or GELU with a compact bf16 output only (the
// encoder's pwconv1) swap the MFMA operands, so a lane's 16x16 accumulator holds 4 consecutive
// output channels of one row, and finish the tile straight from registers (8-byte compact stores):
// no LDS staging, no barriers.  The pwconv1 launches had spent 24 us per tile in the LDS-staged
// epilogue against 8 us in their K loop (C = 256).  The swap transposes each 16x16 product (the
// same K products summed per element), so the bits are those of the staged epilogue.
template <bool REG>
__global__ void __launch_bounds__(512, 2) conv_gemm_bf16dm(const ConvParams p) {
  DCX_TILET(tile_t0);
  constexpr int BM = 256, BN = 256, WN = 2, WM = 4;
  constexpr int WR = 64, WC = 128, TM = WR / 16, TN = WC / 16;
  constexpr int A_G = BM * 4 / 128, B_G = BN * 4 / 128;  // DMA instructions per group per step
  constexpr int A_PW = A_G / 4, B_PW = B_G / 4;
  constexpr int ABUF = BM * 4 * 8, BBUF = BN * 4 * 8;    // ushorts
  constexpr int LDS_US = 3 * (ABUF + BBUF);               // 96 KiB
  __shared__ __attribute__((aligned(16))) unsigned short lds[LDS_US];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int group = __builtin_amdgcn_readfirstlane(tid >> 8);
  const int gw = __builtin_amdgcn_readfirstlane((tid >> 6) & 3);
  const int wm = wave / WN, wn = wave % WN;
  const int ntiles = p.Cout / BN;
  int wg, b, ph;
  flat_tile(((p.Lq + BM - 1) / BM) * ntiles, p.batch, wg, b, ph);
  const int mt = wg / ntiles, nt = wg - mt * ntiles;
  const int q0 = mt * BM, co0 = nt * BN;
  const int nsteps = p.Cin / 32;
  // input: planes (hi pieces at 48-byte strides, 6 bytes per element) or compact bf16 (x_layout:
  // one contiguous 64-byte run per row and step); weights: planes w6 or compact wc likewise
  const int xc = p.x_layout == LAYOUT_BF16 ? 1 : 3;
  const int arow = p.ldx * 2 * xc, a_kq = 16 * xc, a_step = 64 * xc;
  const int row0 = q0 + p.in_base[ph];  // >= 0 for 1x1 convs; the descriptor covers the tile's rows
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(p.x6 + ((long long)b * p.x_bstride + (long long)row0 * p.ldx) * xc), 0,
      max(0, min(BM, p.Lin - row0)) * arow, 0x00020000);
  const bool wc = p.wc != nullptr;
  const __amdgpu_buffer_rsrc_t rw =
      wc ? __builtin_amdgcn_make_buffer_rsrc((void*)(p.wc + (long long)ph * (p.Cin / 32) * p.Cout * 32), 0,
                                             (p.Cin / 32) * p.Cout * 64, 0x00020000)
         : __builtin_amdgcn_make_buffer_rsrc((void*)(p.w6 + (long long)ph * (p.Cin / 16) * p.Cout * 48), 0,
                                             (p.Cin / 16) * p.Cout * 96, 0x00020000);
  const int b_step = wc ? p.Cout * 64 : p.Cout * 192;

  // DMA pieces (bytes, step 0): unit u -> row (u / 64) * 16 + (u & 15), piece (u % 64) >> 4 = the
  // 8-channel group kq; step s adds s * a_step (input) and s * b_step (weights: two K16 chunks)
  int a_off[A_PW], b_off[B_PW];
#pragma unroll
  for (int i = 0; i < A_PW; ++i) {
    const int u = (group * A_G + i * 4 + gw) * 64 + lane;
    const int r = (u >> 6) * 16 + (u & 15), kq = (u & 63) >> 4;
    a_off[i] = r * arow + kq * a_kq;  // rows past Lin: out of range, zeros
  }
#pragma unroll
  for (int i = 0; i < B_PW; ++i) {
    const int u = (group * B_G + i * 4 + gw) * 64 + lane;
    const int c = (u >> 6) * 16 + (u & 15), kq = (u & 63) >> 4;
    b_off[i] = wc ? (co0 + c) * 64 + kq * 16 : (kq >> 1) * p.Cout * 96 + (co0 + c) * 96 + (kq & 1) * 48;
  }
  unsigned short* const a_dst = lds + (group * A_G + gw) * 512;
  unsigned short* const b_dst = lds + 3 * ABUF + (group * B_G + gw) * 512;
  auto dma_step = [&](int s, int, int slot) {  // (step, tap 0, ring slot)
#pragma unroll
    for (int i = 0; i < A_PW; ++i) dma16(rx, a_dst + slot * ABUF + i * 2048, a_off[i] + s * a_step, 0);
#pragma unroll
    for (int i = 0; i < B_PW; ++i) dma16(rw, b_dst + slot * BBUF + i * 2048, b_off[i], s * b_step);
    return A_PW + B_PW;
  };

  const int l15 = lane & 15, kq = lane >> 4;
  const char* const ldsb = reinterpret_cast<const char*>(lds);
  const int a_lane = (wm * WR / 16) * 1024 + kq * 256 + l15 * 16;           // bytes in an A image
  const int b_lane = 6 * ABUF + (wn * WC / 16) * 1024 + kq * 256 + l15 * 16;  // bytes, B image of slot 0
  s16x8 af[TM], bq[TN];
  auto readF = [&](int, int, int slot) {
#pragma unroll
    for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const s16x8*>(ldsb + slot * ABUF * 2 + a_lane + i * 1024);
#pragma unroll
    for (int j = 0; j < TN; ++j) bq[j] = *reinterpret_cast<const s16x8*>(ldsb + slot * BBUF * 2 + b_lane + j * 1024);
  };
  f32x4 acc[TM][TN];
  zero_acc(acc);
  auto mfma = [&]() {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
        if constexpr (REG)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, bq[j]),
                                                              __builtin_bit_cast(bf16x8, af[i]), acc[i][j], 0, 0, 0);
        else
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[i]),
                                                              __builtin_bit_cast(bf16x8, bq[j]), acc[i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  };

  // the ping-pong schedule of conv_gemm_x6dm with taps = 1: A and B of step t ride slot t % 3
  const StepPos l3 = pingpong3_prologue(nsteps, 1, dma_step);
  pingpong3_drain();
  DCX_TILET(tile_t1);
  DCX_CLOCK_BEGIN;
  pingpong3_loop<false>(group, nsteps, 1, l3, dma_step, readF, mfma);
  DCX_CLOCK_END(nsteps * 2 / 3);  // steps counted in units of 1536 ideal cycles (a K32 step is 1024)
  DCX_TILET(tile_t2);
  if constexpr (REG) {
    // lane l of block (i, j): output channels co0 + wn*WC + 16 j + 4 (l >> 4) + e of row 16 i + (l & 15)
    // of the wave's rows.  epilogue_lds's operations in its order: bias, bf16 rounding, GELU, the
    // RNE compact store.
#ifdef DCX_DIAG_DUP
    if (p.diag_skip == 2) return;  // the timing copy of a launch: main loop only
#endif
    unsigned short* const y6 = p.y6 + (long long)b * p.y_bstride;
    const int cq = co0 + wn * WC + 4 * (lane >> 4);
    f32x4 bias[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j)
      bias[j] = p.bias ? *reinterpret_cast<const f32x4*>(p.bias + cq + 16 * j) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int q = q0 + wm * WR + 16 * i + (lane & 15);
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        f32x4 x = acc[i][j] + bias[j];
        if (p.round_bf16) x = round_bf16x4(x);
        if (p.epi == EPI_GELU) {
          if (p.round_bf16) {
            const f32x2 g0 = gelu_bf16_f2(f32x2{x[0], x[1]}), g1 = gelu_bf16_f2(f32x2{x[2], x[3]});
            x = f32x4{g0[0], g0[1], g1[0], g1[1]};  // (the compact store rounds)
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = gelu_f(x[e]);
          }
        }
#ifdef DCX_DIAG_DUP
        if (p.diag_skip == 1 && x[0] != -0x1.234p-100f) continue;  // timing copy: computed, not stored
#endif
        if (q < p.Lq) store_bf16x4(y6, q, p.Cout, cq + 16 * j, x[0], x[1], x[2], x[3]);
      }
    }
  } else {
    epilogue_lds<BM, BN, WM, WN, LDS_US / 2, 512>(p, p, acc, q0, co0, b, ph, reinterpret_cast<float*>(lds));
  }
  DCX_TILE_END(nsteps);  // + K32 steps
}

// ---------------------------------------------------------------------------------------------
// conv_gemm_bf16dp (round 4): conv_gemm_bf16dm<REG> made persistent, with one step stream across
// tiles.  A workgroup walks its tiles (XCD-grouped logical order, as conv_gemm_x6w8) and the ping-pong
// step schedule never drains: the DMA of the next tile's first steps is issued during the current
// tile's last ones (the ring slot of global step g is g % 3), so a tile costs no prologue.  Each
// group finishes its tile from registers in the memory segment that follows its last MFMA segment,
// while the other group runs an MFMA segment: group 0 in MEM0 of the tile's last step, group 1 in
// MEM1 of the next tile's first step.  The register epilogue (bias, bf16 rounding, GELU, 8-byte RNE
// compact stores) is bf16dm<true>'s, after the segment's fragment reads and DMA wait, so its stores
// only have to have drained by the next memory segment's wait.  Same MFMAs in the same order per
// tile: the bits of conv_gemm_bf16dm<true> (tests/test_gpu_bf16.py::test_persistent_same_bits).
// GELU launches finish from the LDS table of the bf16 GELU (gelu_lut_fill, filled while the first
// steps' DMA is in flight).  Takes compact input and weights (LAYOUT_BF16, wc), bf16 rounding,
// >= 3 K32 steps, one phase.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(512, 2) conv_gemm_bf16dp(const ConvParams p) {
  constexpr int BM = 256, BN = 256, WN = 2;
  constexpr int WR = 64, WC = 128, TM = WR / 16, TN = WC / 16;
  constexpr int A_G = BM * 4 / 128, B_G = BN * 4 / 128;  // DMA instructions per group per step
  constexpr int A_PW = A_G / 4, B_PW = B_G / 4;
  constexpr int ABUF = BM * 4 * 8, BBUF = BN * 4 * 8;    // ushorts
  constexpr int LDS_US = 3 * (ABUF + BBUF);               // 96 KiB
  // LDS: the GELU table at byte 0, the launch's bias (fp32, Cout <= kBiasMax), the ring
  constexpr int BIAS_US = 2 * kBf16dpBiasMax, RING_US = kGeluLutUs + BIAS_US;
  __shared__ __attribute__((aligned(16))) unsigned short smem[RING_US + LDS_US];
  unsigned short* const lds = smem + RING_US;
  float* const bias_s = reinterpret_cast<float*>(smem + kGeluLutUs);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int group = __builtin_amdgcn_readfirstlane(tid >> 8);
  const int gw = __builtin_amdgcn_readfirstlane((tid >> 6) & 3);
  const int wm = wave / WN, wn = wave % WN;
  const int ntn = p.Cout / BN, mtiles = (p.Lq + BM - 1) / BM;
  const int per_img = mtiles * ntn, total = per_img * p.batch;
  const int G = gridDim.x;  // a multiple of 8
  const int tile_base = (blockIdx.x & 7) * (G >> 3) + (blockIdx.x >> 3);
  const int nt_block = tile_base < total ? (total - tile_base + G - 1) / G : 0;  // tiles of this block
  if (nt_block == 0) return;  // whole workgroup, before any barrier
  const bool lut = p.gelu_lut > 0 && p.epi == EPI_GELU;
  const int nsteps = p.Cin / 32;
  const int gtot = nt_block * nsteps;  // steps of the block's stream
  const int arow = p.ldx * 2;          // compact rows
  const int b_step = p.Cout * 64;

  // tile k of this block -> (clip, first row, first column)
  auto tile_of = [&](int k, int& b, int& q0, int& co0) {
    const int L = tile_base + k * G;
    b = L / per_img;
    const int wg = L - b * per_img;
    const int mt = wg / ntn;
    q0 = mt * BM;
    co0 = (wg - mt * ntn) * BN;
  };
  auto rx_of = [&](int b, int q0) {  // descriptor over the tile's rows (rows past Lin read zeros)
    const int row0 = q0 + p.in_base[0];
    return __builtin_amdgcn_make_buffer_rsrc((void*)(p.x6 + (long long)b * p.x_bstride + (long long)row0 * p.ldx), 0,
                                             max(0, min(BM, p.Lin - row0)) * arow, 0x00020000);
  };
  const __amdgpu_buffer_rsrc_t rw =
      __builtin_amdgcn_make_buffer_rsrc((void*)p.wc, 0, (p.Cin / 32) * p.Cout * 64, 0x00020000);

  int a_off[A_PW], b_off[B_PW];
#pragma unroll
  for (int i = 0; i < A_PW; ++i) {
    const int u = (group * A_G + i * 4 + gw) * 64 + lane;
    const int r = (u >> 6) * 16 + (u & 15), kq = (u & 63) >> 4;
    a_off[i] = r * arow + kq * 16;
  }
#pragma unroll
  for (int i = 0; i < B_PW; ++i) {
    const int u = (group * B_G + i * 4 + gw) * 64 + lane;
    const int c = (u >> 6) * 16 + (u & 15), kq = (u & 63) >> 4;
    b_off[i] = c * 64 + kq * 16;  // + co0 * 64 in the scalar offset
  }
  unsigned short* const a_dst = lds + (group * A_G + gw) * 512;
  unsigned short* const b_dst = lds + 3 * ABUF + (group * B_G + gw) * 512;
  // DMA of global step g (tile g / nsteps of the stream, K32 step g % nsteps)
  int dk = -1, db = 0, dq0 = 0, dco0 = 0;
  __amdgpu_buffer_rsrc_t drx = rw;
  auto dma_step = [&](int g, int slot) __attribute__((always_inline)) {
    const int k = g / nsteps, st = g - k * nsteps;
    if (k != dk) {  // wave-uniform
      dk = k;
      tile_of(k, db, dq0, dco0);
      drx = rx_of(db, dq0);
    }
#pragma unroll
    for (int i = 0; i < A_PW; ++i) dma16(drx, a_dst + slot * ABUF + i * 2048, a_off[i] + st * 64, 0);
#pragma unroll
    for (int i = 0; i < B_PW; ++i) dma16(rw, b_dst + slot * BBUF + i * 2048, b_off[i], st * b_step + dco0 * 64);
    return A_PW + B_PW;
  };

  const int l15 = lane & 15, kq = lane >> 4;
  const char* const ldsb = reinterpret_cast<const char*>(lds);
  const int a_lane = (wm * WR / 16) * 1024 + kq * 256 + l15 * 16;
  const int b_lane = 6 * ABUF + (wn * WC / 16) * 1024 + kq * 256 + l15 * 16;
  s16x8 af[TM], bq[TN];
  auto readF = [&](int slot) {
#pragma unroll
    for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const s16x8*>(ldsb + slot * ABUF * 2 + a_lane + i * 1024);
#pragma unroll
    for (int j = 0; j < TN; ++j) bq[j] = *reinterpret_cast<const s16x8*>(ldsb + slot * BBUF * 2 + b_lane + j * 1024);
  };
  f32x4 acc[TM][TN];
  zero_acc(acc);
  auto mfma = [&]() {  // operands swapped: a lane's accumulator holds 4 consecutive channels of a row
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, bq[j]),
                                                            __builtin_bit_cast(bf16x8, af[i]), acc[i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  };
  // the register epilogue of tile k, then the accumulators cleared.  GELU launches: from the table;
  // a wave with an element outside it stores the evaluated epilogue (conv_gemm_bf16dm<true>'s) over it
  auto epilogue = [&](int k) __attribute__((always_inline)) {
    int bb, q0, co0;
    tile_of(k, bb, q0, co0);
    const int cq = co0 + wn * WC + 4 * (lane >> 4);
    const int rq = wm * WR + (lane & 15);  // + 16 i: the lane's rows in the tile
    bool eval = !lut;
    if (lut) {
      // buffer stores over the tile's valid rows (rows past Lq are dropped by the descriptor)
      const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(p.y6 + (long long)bb * p.y_bstride + (long long)q0 * p.Cout), 0, min(BM, p.Lq - q0) * p.Cout * 2,
          0x00020000);
      u16x2 hi = {0, 0};
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const f32x4 bias = *reinterpret_cast<const f32x4*>(bias_s + cq + 16 * j);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const f32x4 x = acc[i][j] + bias;
          typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
          const u32x2 w = {gelu_lut2(smem, f32x2{x[0], x[1]}, hi), gelu_lut2(smem, f32x2{x[2], x[3]}, hi)};
          __builtin_amdgcn_raw_buffer_store_b64(w, ry, ((rq + 16 * i) * p.Cout + cq + 16 * j) * 2, 0, 0);
        }
      }
      eval = __builtin_amdgcn_ballot_w64(max(hi[0], hi[1]) >= p.gelu_lut) != 0;  // wave-uniform
      if (eval) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the table's stores first
    }
    if (eval) {  // conv_gemm_bf16dm<true>'s evaluated epilogue
      unsigned short* const y6 = p.y6 + (long long)bb * p.y_bstride;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const f32x4 bias = *reinterpret_cast<const f32x4*>(bias_s + cq + 16 * j);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int q = q0 + rq + 16 * i;
          f32x4 x = round_bf16x4(acc[i][j] + bias);
          if (p.epi == EPI_GELU) {
            const f32x2 g0 = gelu_bf16_f2(f32x2{x[0], x[1]}), g1 = gelu_bf16_f2(f32x2{x[2], x[3]});
            x = f32x4{g0[0], g0[1], g1[0], g1[1]};  // (the compact store rounds)
          }
          if (q < p.Lq) store_bf16x4(y6, q, p.Cout, cq + 16 * j, x[0], x[1], x[2], x[3]);
        }
      }
    }
    zero_acc(acc);
  };

  // prologue: steps 0, 1, 2 of the stream (both groups their pieces) and the GELU table, drained
  for (int t = 0; t < 3; ++t)
    if (t < gtot) dma_step(t, t);
  if (lut) gelu_lut_fill(smem, tid, 512);
  for (int c = tid; c < p.Cout; c += 512) bias_s[c] = p.bias ? p.bias[c] : 0.0f;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  seg_barrier();
  if (group == 0) {
    readF(0);
    int rs = 1, ws = 0, st = 0, k = 0;  // st: step of the current tile k
    for (int g = 0; g < gtot; ++g) {
      mfma();  // MFMA(g)
      seg_barrier();
      // MEM0(g): fragments of g + 1, issue g + 3, retire g + 2; after a tile's last step, its epilogue
      if (g + 1 < gtot) readF(rs);
      int n = 0;
      if (g + 3 < gtot) n = dma_step(g + 3, ws);
      wait_dma(n);
      if (++st == nsteps) {
        epilogue(k);
        st = 0;
        ++k;
      }
      seg_barrier();
      ring_inc(rs);
      ring_inc(ws);
    }
  } else {
    int rs = 0, ws = 0, st = 0, k = 0;
    for (int g = 0;; ++g) {
      // MEM1(g): fragments of g, issue g + 2 (g >= 1), retire g + 1; at a tile's first step (and
      // after the stream), the previous tile's epilogue
      if (g < gtot) readF(rs);
      int n = 0;
      if (g >= 1 && g + 2 < gtot) n = dma_step(g + 2, ws);
      wait_dma(n);
      if (st == 0 && g > 0) epilogue(k - 1);
      if (g == gtot) break;
      seg_barrier();
      mfma();  // MFMA(g)
      seg_barrier();
      ring_inc(rs);
      ring_inc_issue1(ws, g);
      if (++st == nsteps) {
        st = 0;
        ++k;
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// whether conv_gemm_x6dm takes the conv: planes input, Cout % 256, taps >= 2 with a halo or one
// tap without, and 32-bit buffer offsets for the input rows (with the tile's halo) and the weights
static bool in_base_nonneg(const ConvParams& p) {  // every phase's input row offset (unused entries are 0)
  for (int i = 0; i < kMaxPhases; ++i)
    if (p.in_base[i] < 0) return false;
  return true;
}

static bool x6dm_ok(const ConvParams& p, bool halo, int bn) {
  if (!p.x6 || !p.w6 || p.nprod != 6 || p.Cout % bn || (halo ? p.taps < 2 : p.taps != 1)) return false;
  const long long arow = (long long)p.ldx * 6;
  const long long wbytes = (long long)p.taps * (p.Cin / BK) * p.Cout * 96;
  if (!halo) return in_base_nonneg(p) && 1024 * arow < (1LL << 31) && wbytes < (1LL << 31);  // per-tile descriptor
  return (long long)(p.Lin + 1024) * arow < (1LL << 31) && 1024 * arow < (1LL << 31) && wbytes < (1LL << 31);
}

// Whether the 64K-output tiles of the LDS-DMA kernels (BM x bn) or the 256 x 128 tiles of
// conv_gemm_x6pp / x6lm take a conv.  Both run one workgroup per CU; the smaller tiles take half the
// time at ~0.88 of the rate, so they win when a launch has few tiles (the C5 streaming hop, short
// clips, 1x1 convs with narrow outputs such as the encoder's 4C -> C).  The rule looks at one clip
// (rows x column tiles x phases), never at the batch size: the two families sum in different
// orders, and a clip must give the same bits alone as inside a batch of equal-length clips.
// At C2's batch of 32 the threshold picks what ceil(tiles / CUs) rounds would.
static bool big_tiles_pay(const ConvParams& p, int phases, int bn) {
  const int bm = 65536 / bn;
  return (long long)((p.Lq + bm - 1) / bm) * (p.Cout / bn) * phases >= 16;
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
template <int BM, int BN, int WM, int WN, bool ARGMIN>
static hipError_t launch_f32(const ConvParams& p, int batch, int phases, hipStream_t s) {
  return launch_flat<BM, BN>(conv_gemm_f32<BM, BN, WM, WN, ARGMIN>, p, batch, phases, 256, s);
}

static int tap_span(const ConvParams& p) { return (p.taps - 1) * (p.in_step < 0 ? -p.in_step : p.in_step); }

hipError_t launch_splitk_epilogue(const ConvParams& p, const float* partials, int splits, long long stride, int batch,
                                  int phases, hipStream_t s) {
  if (splits < 1 || p.Cout % 4 || p.ldy != p.Cout) return hipErrorInvalidValue;
  ConvParams q = p;
  q.batch = batch;
  q.phases = phases;
  const long long total4 = (long long)phases * batch * p.Lq * (p.Cout / 4);
  hipLaunchKernelGGL(splitk_epilogue_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, s, q, partials, splits,
                     stride, total4);
  return hipGetLastError();
}

// conv_gemm_bf16dp's GELU table: ConvParams::gelu_lut = the table offset from which a wave takes the
// evaluated epilogue (2 kGeluN, the table's end).  Knobs::gelu_lut (DCX_GELU_LUT at dcx_create): 0 =
// evaluated always (A/B); a smaller positive limit sends more waves through the evaluated epilogue (tests)
static int gelu_lut_limit(const Knobs& k) {
  if (k.gelu_lut < 0) return 2 * kGeluN;
  return std::min(k.gelu_lut, 2 * kGeluN);
}

// CU count per device, filled once per device (std::call_once per slot; devices past the table are
// queried each time)
int device_cus() {
  constexpr int kDev = 64;
  static std::once_flag once[kDev];
  static int cus[kDev];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  auto query = [dev] {
    int c = 0;
    if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c < 8) c = 256;
    return c;
  };
  if (dev < 0 || dev >= kDev) return query();
  std::call_once(once[dev], [&] { cus[dev] = query(); });
  return cus[dev];
}

bool bf16dm_takes(int cin, int cout, int lq, int ldx, int phases) {
#ifdef DCX_NO_BF16DM
  return false;
#endif
  ConvParams q{};
  q.Lq = lq;
  q.Cout = cout;
  return cout % 256 == 0 && cin % 32 == 0 && big_tiles_pay(q, phases, 256) && 1024LL * ldx * 6 < (1LL << 31) &&
         (long long)(cin / 16) * cout * 96 < (1LL << 31);
}

hipError_t launch_conv(const ConvParams& p, int batch, int phases, hipStream_t s, const char** kname) {
  if (p.Cin % BK || p.Cout % 32 || phases < 1 || phases > kMaxPhases) return hipErrorInvalidValue;
  if (p.x_layout == LAYOUT_H2) {  // h2 input: the h3 kernels only
    const int bn = x3dq_bn(p);
    if (!x3dq_ok(p, bn == 512 ? 256 : bn == 384 ? 128 : bn, bn >= 384)) return hipErrorInvalidValue;
    if (bn >= 384) return launch_x3dw(p, bn, batch, phases, s, kname);  // 384 x 128 (the C = 128 stage) or 256 x 256 tiles
    return bn == 256 ? launch_x3dq<256>(p, batch, phases, s, kname) : launch_x3dq<128>(p, batch, phases, s, kname);
  }
  if (p.w6) {
    if (p.nprod != 6 && p.nprod != 1) return hipErrorInvalidValue;
    // split-K runs on conv_gemm_x6pp / x6lm (the kernels that read ksplit), whatever the tile count
    const bool ks = p.ksplit > 1;
    if (ks && (p.nprod != 6 || !p.x6 || p.Cout % 128 || batch % p.ksplit || p.kunit < 1 || (p.Cin / BK) % p.kunit ||
               (p.Cin / BK) / p.kunit < p.ksplit))
      return hipErrorInvalidValue;
    const bool b1 = p.nprod == 1;  // profile names: conv_gemm_bf16w* for the one-product mode
    const int span = tap_span(p);
    if (span > 64 || (p.Cin / BK) * p.taps % 2) return hipErrorInvalidValue;
    const bool h = span > 0;
    auto name = [&](const char* x6, const char* bf) {
      if (kname) *kname = b1 ? bf : x6;
    };
    if (!p.x6) {  // fp32 input, split while staging: small-Cout tiles only
      if (!p.x || p.Cin > 128 || p.Cout > 64 || p.taps < 2) return hipErrorInvalidValue;
      if (p.Cout == 64) {
#ifndef DCX_NO_PF
        if (!b1) return launch_x6pf(p, batch, phases, s, kname);  // x6: ping-pong, 512 x 64 tiles
#endif
        name("conv_gemm_x6w4f<256,64,halo>", "conv_gemm_bf16w4f<256,64,halo>");
        return launch_x6w8_af32<256, 64, 4, 1, 64>(p, batch, phases, s);
      }
      name("conv_gemm_x6w4f<256,32,halo>", "conv_gemm_bf16w4f<256,32,halo>");
      return launch_x6w8_af32<256, 32, 4, 1, 64>(p, batch, phases, s);
    }
#ifndef DCX_NO_DM
    if (!ks && !h && !p.fixed_tiles && x6dm_ok(p, false, 256) && big_tiles_pay(p, phases, 256))
      return launch_x6dm<0, 256>(p, batch, phases, s, kname);  // x6 1-tap, Cout % 256
#endif
#ifndef DCX_NO_PP
    if (p.Cout % 128 == 0 && !h && !b1) return launch_x6pp<0>(p, batch, phases, s, kname);  // x6 1-tap
#endif
    const bool dm_b1 = b1 && !h && p.taps == 1 && !p.fixed_tiles && in_base_nonneg(p) && bf16dm_takes(p.Cin, p.Cout, p.Lq, p.ldx, phases);
    if (p.x_layout != LAYOUT_PLANES && (!dm_b1 || p.x_layout != LAYOUT_BF16)) return hipErrorInvalidValue;  // only conv_gemm_bf16dm reads it
#ifndef DCX_NO_BF16DM
    if (dm_b1) {
      ConvParams q = p;
      q.batch = batch;
      q.phases = phases;
      q.gelu_lut = gelu_lut_limit(knobs(p));
      const dim3 grid((unsigned)flat_tiles<256, 256>(p, batch, phases));
      // the register epilogue: bias / GELU epilogues with a compact bf16 output only.  With an fp32
      // output too (the VQ blocks' 1x1 convs) or a residual (pwconv2) it measured slower than the
      // staged epilogue, whose 16-byte stores cover 512 contiguous bytes of a row per instruction
      // (C3 bf16dm, A/B: pwconv1 only 52.5 ms, + the fp32-output convs 55.4, + pwconv2 56.6)
      const bool reg = (p.epi == EPI_BIAS || p.epi == EPI_GELU) && p.y6 && p.y_layout == LAYOUT_BF16 && !p.y && !p.y2 &&
                       !p.y6s && p.mean_mode == MEAN_NONE && phases == 1 && p.out_mul == 1 && knobs(p).bf16_reg_epi;
      // the persistent form (one step stream across tiles) for compact operands; Knobs::bf16_persist = 0
      // (DCX_BF16_PERSIST=0) keeps conv_gemm_bf16dm<true> (A/B, same bits)
      if (reg && p.x_layout == LAYOUT_BF16 && p.wc && p.round_bf16 && p.Cin / 32 >= 3 && p.Cout <= kBf16dpBiasMax &&
          (long long)std::min(256, p.Lq) * p.Cout * 2 < (1ll << 31) && knobs(p).bf16_persist) {
        if (kname) *kname = "conv_gemm_bf16dp<256,256,reg>";
        const long long tiles = (long long)grid.x;
        const int g = (int)std::min<long long>(device_cus(), (tiles + 7) / 8 * 8);
        hipLaunchKernelGGL(conv_gemm_bf16dp, dim3((unsigned)std::max(8, g / 8 * 8)), dim3(512), 0, s, q);
        return hipGetLastError();
      }
      if (kname) *kname = reg ? "conv_gemm_bf16dm<256,256,reg>" : "conv_gemm_bf16dm<256,256>";
      if (reg) hipLaunchKernelGGL(conv_gemm_bf16dm<true>, grid, dim3(512), 0, s, q);
      else hipLaunchKernelGGL(conv_gemm_bf16dm<false>, grid, dim3(512), 0, s, q);
      return hipGetLastError();
    }
#endif
    if (p.Cout % 128 == 0 && !h) {  // 1-tap: 4-wave 128 x 128 tiles, two workgroups per CU
      name("conv_gemm_x6w4<128,128>", "conv_gemm_bf16w4<128,128>");
      return launch_x6w8<128, 128, 2, 2, 0, false>(p, batch, phases, s);
    }
    if (p.Cout % 128 == 0) {
      const bool pay256 = !ks && big_tiles_pay(p, phases, 256), pay128 = !ks && big_tiles_pay(p, phases, 128);
#ifndef DCX_NO_DQ
      if (p.taps >= 3 && pay256 && x6dm_ok(p, true, 256)) return launch_x6dq<256>(p, batch, phases, s, kname);  // 16x16x32
      if (p.taps >= 3 && pay128 && x6dm_ok(p, true, 128)) return launch_x6dq<128>(p, batch, phases, s, kname);
#endif
#ifndef DCX_NO_DM
      if (pay256 && x6dm_ok(p, true, 256)) return launch_x6dm<64, 256>(p, batch, phases, s, kname);  // LDS-DMA ping-pong
      if (pay128 && x6dm_ok(p, true, 128)) return launch_x6dm<64, 128>(p, batch, phases, s, kname);
#endif
#ifndef DCX_NO_PP
      if (!b1) return launch_x6pp<64>(p, batch, phases, s, kname);  // x6: ping-pong kernel
#endif
      name("conv_gemm_x6w8<256,128,halo>", "conv_gemm_bf16w8<256,128,halo>");
      return launch_x6w8<256, 128, 4, 2, 64, false>(p, batch, phases, s);
    }
    // small Cout: 4-wave 256-row tiles (< 80 KB LDS), two workgroups per CU
    if (p.Cout % 64 == 0) {
      if (h) {
        name("conv_gemm_x6w4<256,64,halo>", "conv_gemm_bf16w4<256,64,halo>");
        return launch_x6w8<256, 64, 4, 1, 64, false>(p, batch, phases, s);
      }
      name("conv_gemm_x6w4<256,64>", "conv_gemm_bf16w4<256,64>");
      return launch_x6w8<256, 64, 4, 1, 0, false>(p, batch, phases, s);
    }
    if (h) {
      name("conv_gemm_x6w4<256,32,halo>", "conv_gemm_bf16w4<256,32,halo>");
      return launch_x6w8<256, 32, 4, 1, 64, false>(p, batch, phases, s);
    }
    name("conv_gemm_x6w4<256,32>", "conv_gemm_bf16w4<256,32>");
    return launch_x6w8<256, 32, 4, 1, 0, false>(p, batch, phases, s);
  }
  if (p.Cout % 128 == 0) {
    if (kname) *kname = "conv_gemm_f32<128,128>";
    return launch_f32<128, 128, 2, 2, false>(p, batch, phases, s);
  }
  if (p.Cout % 64 == 0) {
    if (kname) *kname = "conv_gemm_f32<256,64>";
    return launch_f32<256, 64, 4, 1, false>(p, batch, phases, s);
  }
  if (kname) *kname = "conv_gemm_f32<256,32>";
  return launch_f32<256, 32, 4, 1, false>(p, batch, phases, s);
}

// The members of a grouped launch in launch order, largest key first (the longest tiles start
// first): member k's params, its bm x bn tiles per clip and its range of logical tiles.  split: the
// member runs as batch * ksplit virtual clips of one phase (split-K).  Returns the block total, or
// -1 past 2^30.
template <class Key>
static long long fill_group(ConvGroup& g, const ConvParams* ps, int n, int batch, int bm, int bn, bool split, Key key) {
  int order[kMaxGroup] = {0, 1, 2};
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j)
      if (key(ps[order[j]]) > key(ps[order[i]])) std::swap(order[i], order[j]);
  long long start = 0;
  for (int k = 0; k < n; ++k) {
    ConvParams& p = g.p[k] = ps[order[k]];
    const int clips = split ? batch * std::max(1, p.ksplit) : batch;
    if (split) {
      p.batch = clips;
      p.phases = 1;
    }
    g.tiles_per_clip[k] = ((p.Lq + bm - 1) / bm) * (p.Cout / bn);
    g.start[k] = (int)start;
    start += (long long)g.tiles_per_clip[k] * clips;
  }
  if (start > (1LL << 30)) return -1;
  for (int k = n; k <= kMaxGroup; ++k) g.start[k] = (int)start;
  return start;
}

hipError_t launch_conv_group(const ConvParams* ps, int n, int batch, hipStream_t s, const char** kname) {
  if (n < 1 || n > kMaxGroup || batch < 1) return hipErrorInvalidValue;
  const int cout = ps[0].Cout;
  const bool h3 = ps[0].x_layout == LAYOUT_H2;  // h3 convs: conv_gemm_x3dw_group / x3dq_group (any tile count)
  const int bsel = h3 ? x3dq_bn(ps[0]) : 0;
  const int bn = h3 ? (bsel == 512 ? 256 : bsel == 384 ? 128 : bsel) : cout % 256 == 0 ? 256 : 128;
  const int bm = h3 ? (bsel == 512 ? 256 : bsel == 384 ? 384 : 32768 / bn) : 65536 / bn;
  for (int i = 0; i < n; ++i) {
    const ConvParams& p = ps[i];
    if (h3) {
      if (p.Cout != cout || p.x_layout != LAYOUT_H2 || p.taps < 3 || x3dq_bn(p) != bsel || !x3dq_ok(p, bn, bsel >= 384) ||
          (p.clip_len != nullptr) != (ps[0].clip_len != nullptr))
        return hipErrorNotSupported;
    } else if (p.Cout != cout || cout % 128 || p.Cin % BK || !p.x6 || !p.w6 || p.nprod != 6 || p.x_layout != LAYOUT_PLANES ||
               p.taps < 3 || tap_span(p) == 0 || tap_span(p) > 64 || (p.Cin / BK) * p.taps % 2 ||
               !x6dm_ok(p, true, bn) || !big_tiles_pay(p, 1, bn)) {
      return hipErrorNotSupported;  // not one launch_conv would give to conv_gemm_x6dq<bn> (same bits either way)
    }
  }
  ConvGroup g{};
  const long long blocks = fill_group(g, ps, n, batch, bm, bn, false, [](const ConvParams& p) { return (long long)p.taps; });
  if (blocks < 0) return hipErrorInvalidValue;
  if (h3) return launch_h3_group(g, bsel, knobs(ps[0]).h3_split, (unsigned)blocks, s, kname);
  return launch_x6dq_group(g, bn, (unsigned)blocks, s, kname);
}

hipError_t launch_conv_split_group(const ConvParams* ps, int n, int batch, hipStream_t s, const char** kname) {
  if (n < 1 || n > kMaxGroup || batch < 1) return hipErrorInvalidValue;
  for (int i = 0; i < n; ++i) {  // every member a conv launch_conv would give to conv_gemm_x6pp<64, 128>
    const ConvParams& p = ps[i];
    const int S = std::max(1, p.ksplit);
    const int span = tap_span(p);
    if (!p.x6 || !p.w6 || p.nprod != 6 || p.x_layout != LAYOUT_PLANES || p.Cout % 128 || p.Cin % BK || p.taps < 3 || span == 0 ||
        span > 64 || (p.Cin / BK) * p.taps % 2 || (S > 1 && (p.kunit < 1 || (p.Cin / BK) % p.kunit ||
                                                            (p.Cin / BK) / p.kunit < S)))
      return hipErrorNotSupported;
  }
  ConvGroup g{};
  const long long blocks = fill_group(g, ps, n, batch, 256, 128, true, [](const ConvParams& p) {
    return (long long)p.taps * (p.Cin / BK) / std::max(1, p.ksplit);  // work per slice
  });
  if (blocks < 0) return hipErrorInvalidValue;
  return launch_x6pp_group(g, (unsigned)blocks, s, kname);
}

hipError_t launch_splitk_epilogue_group(const ConvParams* ps, const float* const* partials, const int* splits,
                                        const long long* strides, int n, int batch, bool chain, hipStream_t s) {
  if (n < 1 || n > kMaxGroup || batch < 1) return hipErrorInvalidValue;
  SplitEpiGroup g{};
  g.chain = chain ? n : 0;
  long long start = 0;
  for (int k = 0; k < n; ++k) {
    const ConvParams& p = ps[k];
    if (splits[k] < 1 || p.Cout % 4 || p.ldy != p.Cout) return hipErrorInvalidValue;
    g.p[k] = p;
    g.p[k].batch = batch;
    g.p[k].phases = 1;
    g.part[k] = partials[k];
    g.splits[k] = splits[k];
    g.stride[k] = strides[k];
    g.total4[k] = (long long)batch * p.Lq * (p.Cout / 4);
    if (chain && (p.Lq != ps[0].Lq || p.Cout != ps[0].Cout)) return hipErrorInvalidValue;
    g.start[k] = (int)start;
    // chain: one range of blocks (member 0's) whose threads finish every member in order; the
    // other members' ranges are empty but start[] still marks which members exist
    start += chain && k > 0 ? 0 : (g.total4[k] + 255) / 256;
  }
  if (start > (1LL << 30)) return hipErrorInvalidValue;
  for (int k = n; k <= kMaxGroup; ++k) g.start[k] = (int)start;
  hipLaunchKernelGGL(splitk_epilogue_group_kernel, dim3((unsigned)start), dim3(256), 0, s, g);
  return hipGetLastError();
}

int vq_argmin_ntiles(int ncodes) { return ncodes / 128; }

hipError_t launch_vq_argmin(const ConvParams& p, int rows, hipStream_t s, const char** kname) {
  if (p.Cin % BK || p.Cout % 128) return hipErrorInvalidValue;
  ConvParams q = p;
  q.Lq = rows;
  q.Lin = rows;
  if (p.w6) return hipErrorInvalidValue;  // x6 mode searches with launch_vq_prefilter + rescore
  if (kname) *kname = "vq_dist_argmin_f32<128,128>";
  return launch_f32<128, 128, 2, 2, true>(q, 1, 1, s);
}

}  // namespace dcx
