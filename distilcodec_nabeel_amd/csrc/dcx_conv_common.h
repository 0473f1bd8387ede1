// Device code shared by the conv kernel files (dcx_conv.hip, dcx_conv_x6w8.hip, dcx_conv_x6.hip,
// dcx_conv_h3.hip): vector types, LDS row layouts, activations, tile maps, the LDS epilogue,
// the LDS-DMA helpers and the diagnostic builds' counters.  The files
// are separate translation units without relocatable device code, so every __device__ variable
// here is a per-file static copy.
#pragma once
#include <algorithm>
#include <type_traits>

#include "dcx_kernels.h"
#include "dcx_planes.h"

namespace dcx {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int BK = 16;    // K chunk per pipeline stage (both modes)
constexpr int LDSK = 20;  // f32 mode: padded LDS row (floats); 20*i mod 64 distinct per b128 group
// x6 mode LDS rows hold [half 2][plane 3][8] bf16 = 96 B of one row / column.  Two layouts, both
// conflict-free for ds_read_b128 of one piece by 16 lanes on 16 consecutive rows (any tap offset):
//  * padded (8-wave kernels): 112-byte rows, 28 r mod 64 distinct;
//  * swizzled (4-wave kernels, which must stay under 80 KB for two workgroups per CU): 96-byte
//    rows, and rows with bit 3 set store their two K halves swapped, so rows r and r+8 differ in
//    the parity of their 16-byte bank group (6 r + piece mod 16).  Measured 1-2 % slower than the
//    padded rows on the 8-wave kernels (the per-row XOR), hence only where LDS requires it.
template <bool SWZ>
struct XRow {
  static constexpr int kStride = SWZ ? 48 : 56;  // ushort
  __device__ static __forceinline__ int half(int row, int h) { return SWZ ? h ^ ((row >> 3) & 1) : h; }
  __device__ static __forceinline__ int off(int row, int piece) {  // piece = half * 3 + plane
    const int h = piece >= 3;
    return row * kStride + (half(row, h) * 3 + piece - 3 * h) * 8;
  }
};

// v * sigmoid(v) from v_exp_f32 and v_rcp_f32 (each ~1 ulp): 5 instructions instead of the
// library expf and an IEEE divide; silu(-inf side) -> -0, silu(+large) -> v.
__device__ __forceinline__ float silu_f(float v) { return v * __builtin_amdgcn_rcpf(1.0f + __expf(-v)); }
__device__ __forceinline__ float gelu_f(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }
// GELU of the bf16 mode, whose result is rounded to bf16 (2^-8 relative) right after: erf from
// the Chebyshev-fitted erfc of Numerical Recipes (erfcc, relative error < 1.2e-7 everywhere), one
// v_rcp_f32, one v_exp_f32 and 9 FMAs, branch-free.  ocml's erff branches on |x| (both paths run in
// mixed waves) and cost 9 of the 64 ms the bf16 1x1 convs take per C3 step (timing probe).  The x6
// mode uses it too (epilogue_lds and splitk_epi4 pick it for every planes-mode conv, p.w6): its
// absolute error against the fp64 GELU is 4.5e-7, below torch's fp32 erff GELU's 1.2e-6, so the
// fp32-level tolerances hold (tests/test_gpu_conv.py, 109 dB end to end).  Only the IEEE fp32-MFMA
// mode keeps the library erff.
__device__ __forceinline__ float gelu_bf16_f(float v) {
#ifdef DCX_GELU_ERF  // A/B builds: the library erff in the bf16 mode too
  return gelu_f(v);
#endif
  const float z = fabsf(v) * 0.70710678118654752440f;
  const float t = __builtin_amdgcn_rcpf(fmaf(0.5f, z, 1.0f));
  float q = 0.17087277f;
  q = fmaf(q, t, -0.82215223f);
  q = fmaf(q, t, 1.48851587f);
  q = fmaf(q, t, -1.13520398f);
  q = fmaf(q, t, 0.27886807f);
  q = fmaf(q, t, -0.18628806f);
  q = fmaf(q, t, 0.09678418f);
  q = fmaf(q, t, 0.37409196f);
  q = fmaf(q, t, 1.00002368f);
  const float c = t * __expf(fmaf(t, q, fmaf(-z, z, -1.26551223f)));  // erfc(|v| / sqrt 2)
  // erf(v / sqrt 2) rounded to fp32, then the reference's 0.5 v (1 + erf) with its cancellation
  // for large negative v (torch's GELU formula)
  const float e = v >= 0.0f ? 1.0f - c : c - 1.0f;
  return 0.5f * v * (1.0f + e);
}

// gelu_bf16_f on two values at once: the same operations in the same order (so the same bits), with
// the multiplies and FMAs as packed fp32 (v_pk_mul_f32 / v_pk_fma_f32, two lanes' worth per
// instruction); only v_rcp_f32 / v_exp_f32 and the sign select stay per value.  The bf16 1x1 convs'
// pwconv1 epilogue is bound by this VALU work (65 k GELUs per 256 x 256 tile).
__device__ __forceinline__ f32x2 gelu_bf16_f2(f32x2 v) {
#ifdef DCX_GELU_SCALAR  // A/B builds
  return f32x2{gelu_bf16_f(v[0]), gelu_bf16_f(v[1])};
#endif
  const f32x2 z = __builtin_elementwise_abs(v) * 0.70710678118654752440f;
  const f32x2 d = __builtin_elementwise_fma(f32x2{0.5f, 0.5f}, z, f32x2{1.0f, 1.0f});
  const f32x2 t = {__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
  auto fm = [&](f32x2 q, float c) { return __builtin_elementwise_fma(q, t, f32x2{c, c}); };
  f32x2 q = {0.17087277f, 0.17087277f};
  q = fm(q, -0.82215223f);
  q = fm(q, 1.48851587f);
  q = fm(q, -1.13520398f);
  q = fm(q, 0.27886807f);
  q = fm(q, -0.18628806f);
  q = fm(q, 0.09678418f);
  q = fm(q, 0.37409196f);
  q = fm(q, 1.00002368f);
  const f32x2 arg = __builtin_elementwise_fma(t, q, __builtin_elementwise_fma(-z, z, f32x2{-1.26551223f, -1.26551223f}));
  const f32x2 c = t * f32x2{__expf(arg[0]), __expf(arg[1])};
  const f32x2 e = {v[0] >= 0.0f ? 1.0f - c[0] : c[0] - 1.0f, v[1] >= 0.0f ? 1.0f - c[1] : c[1] - 1.0f};
  return 0.5f * v * (1.0f + e);
}

// XCD-aware bijective block remap (cdna_hip_programming.md §5 "XCD swizzle must be bijective"):
// blocks b and b+8 share an XCD, so consecutive logical tiles (same row panel, all column
// tiles) are dealt to the same XCD and share its L2.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

// 1-D conv grids: tiles of (phase, clip, row tile, column tile), column tile fastest, XCD-remapped as
// one range, so the blocks of an XCD share input panels and weights across clips too.  (With a
// (tiles, batch, phases) grid, blockIdx.x & 7 is not the block's XCD unless tiles % 8 == 0.)
__device__ __forceinline__ void flat_tile(int tpc, int batch, int& wg, int& b, int& ph) {
  const int t = xcd_remap(blockIdx.x, gridDim.x);
  const int per_ph = tpc * batch;
  ph = t / per_ph;
  const int r = t - ph * per_ph;
  b = r / tpc;
  wg = r - b * tpc;
}

// Split-K (ConvParams::ksplit > 1): the launch's clips are virtual, b = slice * clips + clip; slice
// `sl` owns the input-channel chunks [c0, c0 + nchunks) (whole units of kunit chunks, as even as
// the units allow) and writes its partial sums as clip b of the output (the caller's partial buffer).
__device__ __forceinline__ void ksplit_slice(const ConvParams& p, int b, int& clip, int& c0, int& nchunks) {
  clip = b;
  c0 = 0;
  nchunks = p.Cin / BK;
  if (p.ksplit > 1) {
    const int clips = p.batch / p.ksplit, sl = b / clips;
    clip = b - sl * clips;
    const int nunits = nchunks / p.kunit, base = nunits / p.ksplit, extra = nunits % p.ksplit;
    c0 = (sl * base + min(sl, extra)) * p.kunit;
    nchunks = (base + (sl < extra ? 1 : 0)) * p.kunit;
  }
}

// Zero page read in place of out-of-range input rows (conv zero padding): selecting the address
// instead of the loaded value keeps every staging load unconditional, so hipcc neither branches
// around it nor waits vmcnt(0) after it (cdna_hip_programming.md §5, trap 4(c)).
// (One copy per kernel file.  `used` keeps the compiler from folding loads of a file-local variable
// that nothing writes into constants, which would turn the address select back into a value select.)
static __device__ __attribute__((used, aligned(16))) float g_zero_row[32] = {0.f};

// Diagnostic builds only.  The counters are written by kernels of several files, each of which has
// its own copy; DCX_DIAG_FILE(tag), once per file, defines diag_<tag>(), through which the exported
// dcx_diag_* functions (dcx_conv.hip) add the copies up (the tile stamps: concatenate them).
//  * DCX_CLOCK_DIAG, g_clock_diag: per-workgroup shader-clock and 100 MHz real-time ticks over the
//    main loop, summed (in-kernel clock = sum(memtime) / sum(realtime) * 100 MHz), and steps.
//  * DCX_SEG_DIAG, g_seg_diag: per-segment shader-clock sums of a ping-pong main loop, for wave 0
//    (group 0, [0..5]) and wave 4 (group 1, [6..11]): MFMA issue, barrier wait, fragment-read issue,
//    stores (with their vmcnt wait), loads + loop control, barrier wait; [12] steps.  g_seg_diag8
//    (conv_gemm_x3dw): the same six sums for every wave of the workgroup, [wave * 6 + i], [48] steps.
//  * DCX_TILE_DIAG, g_tile_diag: per-workgroup 100 MHz real-time stamps of a tile (entry, main loop
//    start, main loop end, exit) and the hardware ids of its CU (HW_ID, XCC_ID), in completion order.
#if defined(DCX_CLOCK_DIAG) || defined(DCX_SEG_DIAG) || defined(DCX_TILE_DIAG)
#define DCX_DIAG 1
constexpr int kTileDiagMax = 16384;
[[maybe_unused]] static __device__ unsigned long long g_clock_diag[3], g_seg_diag[13], g_seg_diag8[49];
[[maybe_unused]] static __device__ unsigned long long g_tile_diag[kTileDiagMax * 6];
[[maybe_unused]] static __device__ unsigned int g_tile_cnt;
enum DiagSet : int { DIAG_CLOCK, DIAG_SEG, DIAG_SEG8, DIAG_TILES };
// This file's copy of `set`: its n counters added to out[0..n) (returns 0), or (DIAG_TILES) up to n
// tile stamps of 6 words stored at out (returns how many); -1 on a HIP error.
static int diag_read(int set, unsigned long long* out, int n, int reset) {
  if (set == DIAG_TILES) {
    unsigned int cnt = 0;
    if (hipMemcpyFromSymbol(&cnt, HIP_SYMBOL(g_tile_cnt), sizeof cnt) != hipSuccess) return -1;
    cnt = std::min(cnt, (unsigned)std::max(0, std::min(n, kTileDiagMax)));
    if (cnt && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_tile_diag), sizeof(unsigned long long) * 6 * cnt) != hipSuccess) return -1;
    const unsigned int z = 0;
    if (reset && hipMemcpyToSymbol(HIP_SYMBOL(g_tile_cnt), &z, sizeof z) != hipSuccess) return -1;
    return (int)cnt;
  }
  const void* sym = set == DIAG_CLOCK ? (const void*)g_clock_diag : set == DIAG_SEG ? (const void*)g_seg_diag : (const void*)g_seg_diag8;
  unsigned long long v[49] = {};
  if (n > 49 || hipMemcpyFromSymbol(v, sym, sizeof(unsigned long long) * n) != hipSuccess) return -1;
  for (int i = 0; i < n; ++i) out[i] += v[i];
  const unsigned long long z[49] = {};
  if (reset && hipMemcpyToSymbol(sym, z, sizeof(unsigned long long) * n) != hipSuccess) return -1;
  return 0;
}
#define DCX_DIAG_FILE(tag) \
  int diag_##tag(int set, unsigned long long* out, int n, int reset) { return diag_read(set, out, n, reset); }
#else
#define DCX_DIAG_FILE(tag)
#endif
#ifdef DCX_SEG_DIAG
#define DCX_SEGT(v) const unsigned long long v = __builtin_amdgcn_s_memtime()
#else
#define DCX_SEGT(v)
#endif
#ifdef DCX_TILE_DIAG
#define DCX_TILET(v) const unsigned long long v = __builtin_amdgcn_s_memrealtime()
#else
#define DCX_TILET(v)
#endif

// ---------------------------------------------------------------------------------------------
// Conv epilogue through LDS: the accumulator tile is written to LDS (in row passes that fit the
// kernel's LDS), then each thread finishes 4 consecutive output channels of a row with 16-byte
// loads of bias / gamma / residual / mean accumulator and 16-byte fp32 stores (8-byte plane
// stores).  This keeps the per-element code out of the 64-way unrolled accumulator loop.
// ---------------------------------------------------------------------------------------------
// acc: f32x16[WR/32][WC/32] (32x32 MFMA blocks) or f32x4[WR/16][WC/16] (16x16 blocks).
// The epilogue's per-clip range values, read before a tile's main loop so that their memory round
// trips overlap its prologue instead of stalling the epilogue (round 6): the h2 output's shift from its
// bound program (stored to y_ash, non-finite bounds flagged) and the clip's running max |v| (acur).
struct EpiPre {
  int osh;
  float acur;
  bool track;
};
template <int RROW>
__device__ __forceinline__ EpiPre epi_range_pre(const ConvParams& p, const ConvParams& pr, int b) {
  EpiPre e{0, 0.f, false};
  const bool h2o = (p.y6 && p.y_layout == LAYOUT_H2) || (p.y6s && p.ys_layout != LAYOUT_PLANES);
  const bool h2row = (RROW & 2) && h2o && pr.yb.rowwise;
  if (h2o && !h2row) {
    const float bnd = range_bound(pr.yb, b);
    e.osh = __builtin_amdgcn_readfirstlane(h2_shift(bnd));
    if (threadIdx.x == 0) {
      if (pr.y_ash) pr.y_ash[b] = e.osh;
      if (pr.rflag && !(bnd <= 3.0e38f)) atomicOr(pr.rflag, RANGE_NONFINITE);
    }
  }
  const bool track = pr.y_amax != nullptr;
  e.track = track;
  e.acur = track && !h2row ? __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(
                                                           __builtin_bit_cast(int, range_cur(pr.y_amax, b))))
                           : 0.f;
  return e;
}

// ---------------------------------------------------------------------------------------------
// Compile-time epilogue forms (the h3 kernels).  epilogue_lds decides everything per row at run time:
// epi, mean_mode, which of y / y2 / y6 / y6s exist and their layouts, round_bf16, range tracking.  In
// the unrolled rows that is ~1100 branches, and because the number of stores of a row then depends on
// the path taken, hipcc can place only vmcnt(0) before a later row's loaded values: every such wait
// also drains the stores of the rows before it.  An EpiForm fixes those fields, and epilogue_form is
// the same arithmetic, operation by operation, for a fixed form.  EpiGeneric keeps epilogue_lds.
// y6h / y6sh: y6 / y6s exist and are LAYOUT_H2 (no form writes planes or compact images); rowwise:
// the h2 output's bound is per row (one-tap convs).  round_bf16 is 0 in every form.
// ---------------------------------------------------------------------------------------------
struct EpiGeneric {
  static constexpr bool fixed = false;
};
template <int EPI, int MEAN, bool Y, bool Y2, bool Y6H, bool Y6SH, bool TRACK, bool ROWWISE = false>
struct EpiForm {
  static constexpr bool fixed = true;
  static constexpr int epi = EPI, mean = MEAN;
  static constexpr bool y = Y, y2 = Y2, y6h = Y6H, y6sh = Y6SH, track = TRACK, rowwise = ROWWISE;
};
// (host) whether p is exactly the form F: the launchers pick an instantiation with it
template <typename F>
inline bool epi_form_is(const ConvParams& p) {
  const bool h2o = F::y6h || F::y6sh;
  return p.epi == F::epi && p.mean_mode == F::mean && !p.round_bf16 && (p.y != nullptr) == F::y &&
         (p.y2 != nullptr) == F::y2 && (p.y6 != nullptr) == F::y6h && (p.y6s != nullptr) == F::y6sh &&
         (!p.y6 || p.y_layout == LAYOUT_H2) && (!p.y6s || p.ys_layout == LAYOUT_H2) && (p.y_amax != nullptr) == F::track &&
         (h2o ? (p.yb.rowwise != 0) == F::rowwise : true) && (F::epi != EPI_GELU || p.w6 != nullptr) &&
         (F::mean == MEAN_NONE || p.macc != nullptr);
}

// epilogue_lds for a fixed form F (its template arguments, and the meaning of every name, are
// epilogue_lds's).  Besides the branches, the order of the memory operations differs:
//  * a batch's rows are all finished into registers (LDS read, bias, residual / gamma / mean add)
//    before its first store, so the batch's loaded values are consumed before any store is issued;
//  * the next batch's residual / mean rows are loaded before the current batch's stores, so their
//    wait is vmcnt(stores after them), not 0;
//  * a pass whose rows all lie inside Lq (workgroup-uniform) runs without the per-row end test: a
//    skipped row would again make the store count depend on the path.
// Aliasing (the ResBlock state and the mean accumulator are updated in place): a thread stores only
// elements it has already loaded, and the rows it loads early are rows it has not stored yet.
template <int BM, int BN, int WM, int WN, int LDS_FLOATS, int NT, int RROW, bool RAG, typename F, typename AccT>
__device__ __forceinline__ void epilogue_form(const ConvParams& p, const ConvParams& pr, AccT& acc, int q0, int co0, int b,
                                              int ph, float* smem, const EpiPre& pre) {
  constexpr int WR = BM / WM, WC = BN / WN;
  static_assert(sizeof(acc[0][0]) == 16 && sizeof(acc) == WR * WC * 4 / 64, "16 x 16 accumulator blocks");
  constexpr int LDSW = BN + 4;
  constexpr int RPP = (BM * LDSW <= LDS_FLOATS) ? BM
                      : (BM / 2 * LDSW <= LDS_FLOATS) ? BM / 2
                      : (BM / 4 * LDSW <= LDS_FLOATS) ? BM / 4 : WR;
  static_assert(RPP % WR == 0 && RPP * LDSW <= LDS_FLOATS, "epilogue pass does not fit LDS");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const long long ob = (long long)b * p.y_bstride;
  constexpr bool RIN = RROW & 1, ROUT = RROW & 2;
  constexpr bool h2o = F::y6h || F::y6sh, h2row = ROUT && h2o && F::rowwise;
  constexpr bool need_r = F::epi == EPI_GAMMA_RES || F::epi == EPI_RES;
  constexpr bool need_m = F::mean == MEAN_MID || F::mean == MEAN_LAST;
  // only the last member of a mean chain has outputs of its own
  static_assert(!((F::mean == MEAN_FIRST || F::mean == MEAN_MID) && (F::y || F::y2 || h2o || F::track)), "mean form");
  unsigned short* const y6 = F::y6h ? p.y6 + ob * 2 : nullptr;
  unsigned short* const y6s = F::y6sh ? p.y6s + ob * 2 : nullptr;
  const float osc = __builtin_bit_cast(
      float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, __builtin_ldexpf(1.0f, h2o && !h2row ? pre.osh : 0))));
  float vmax = 0.f;
  const int lq_live = RAG ? clip_rows(pr.clip_len, pr.len_mul, b, p.Lq) : p.Lq;
  // Line-major lanes (dcx_epi_lines.h): a thread owns 4 consecutive channels of a row and twice the
  // rows that epilogue_lds's 8-channel groups give it, so every 16-byte-per-lane load and store of a
  // wave moves whole contiguous 128-byte lines, and the LDS staging reads are one f32x4 per row, 64
  // lanes x 16 B contiguous (a 16-lane group reads 256 contiguous bytes: 16 distinct bank quads).
  // Two forms keep epilogue_lds's 8-channel groups (NH = 2 pieces per row, 16 B apart, read from LDS
  // in the order hsw): the one-tap forms (RROW != 0), whose per-row range words and scales are per
  // thread and row and double with the rows (conv_gemm_x3dw<256,256> 26.7 -> 27.3 ms per C2 step with
  // 4-channel groups), and the ragged 256-column forms with a residual and outputs of their own
  // (EpiC2, last of mean), which gained 8 / 36 / 32 bytes of scratch with them
  // (profiles/epi_lines_resources.md).
  constexpr bool LINES = RROW == 0 && !(RAG && BN == 256 && need_r && (F::mean == MEAN_NONE || F::mean == MEAN_LAST));
  constexpr int G = LINES ? kEpiG : 8, NH = G / 4;
  static_assert(NT % (BN / G) == 0 && LDSW == epi_ldsw(BN), "each thread keeps one channel group");
  const int cg = (tid % (BN / G)) * G, trow = tid / (BN / G), co = co0 + cg;
  const int hsw = (lane >> 3) & 1;  // NH = 2: LDS read order of the two halves (epilogue_lds)
  f32x4 bias4[NH], gamma4[NH];
#pragma unroll
  for (int h = 0; h < NH; ++h) {
    bias4[h] = p.bias ? *reinterpret_cast<const f32x4*>(p.bias + co + 4 * h) : f32x4{0.f, 0.f, 0.f, 0.f};
    gamma4[h] = F::epi == EPI_GAMMA_RES ? *reinterpret_cast<const f32x4*>(p.gamma + co + 4 * h) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  constexpr int RSTEP = NT / (BN / G), ROWS_T = RPP / RSTEP;
  static_assert(RPP % RSTEP == 0 && (!LINES || RSTEP == epi_rstep(NT, BN)), "epilogue rows per thread");
  constexpr auto div_cap = [](int n, int cap) {
    int d = n < cap ? n : cap;
    while (n % d) --d;
    return d;
  };
  // batches of 8 16-byte pieces per thread, 4 where residual / mean rows are loaded (4 VGPRs per piece
  // and tensor): two batches' rows are in registers at a time here, and with twice as many the
  // 256 x 256 residual forms spilled 52-176 bytes, reloaded inside the row code.  (EpiPw1's per-row
  // range words, rin / rbnd, are one VGPR each: it keeps 4 rows.)
  constexpr int IB = div_cap(ROWS_T, need_r || need_m ? 4 / NH : 8 / NH);
  auto row_bound = [&](int q) { return fmaf(pr.yb.g[0], fmaxf(pr.yb.m[0][(long long)b * p.Lq + q], pr.yb.f[0]), pr.yb.c); };

  auto pass = [&](int r0, auto fullt) {
    constexpr bool FULL = decltype(fullt)::value;  // every row of the pass lies inside Lq
    f32x4 r[IB][NH], m[IB][NH];
    float rin[RIN ? IB : 1], rbnd[h2row ? IB : 1];
    auto load = [&](int rb) {  // rows past the end clamped, as in epilogue_lds
#pragma unroll
      for (int k = 0; k < IB; ++k) {
        const int qq = q0 + r0 + trow + (rb + k) * RSTEP;
        const int q = FULL ? qq : min(qq, p.Lq - 1);
        const long long o = ob + ((long long)q * p.out_mul + ph) * p.ldy + co;
#pragma unroll
        for (int h = 0; h < NH; ++h) {
          if constexpr (need_r) r[k][h] = *reinterpret_cast<const f32x4*>(p.res + o + 4 * h);
          if constexpr (need_m) m[k][h] = *reinterpret_cast<const f32x4*>(p.macc + o + 4 * h);
        }
        if constexpr (RIN) rin[k] = pr.x_ash_row ? __builtin_ldexpf(1.0f, -pr.x_ash_row[(long long)b * p.Lin + q]) : 1.0f;
        if constexpr (h2row) rbnd[k] = row_bound(q);
      }
    };
    load(0);
    __syncthreads();  // acc rows [r0, r0 + RPP) of the tile -> LDS (lane holds column l & 15, rows 4 (l >> 4) + e)
    if (wm * WR >= r0 && wm * WR < r0 + RPP) {
#pragma unroll
      for (int i = 0; i < WR / 16; ++i)
#pragma unroll
        for (int j = 0; j < WC / 16; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int row = wm * WR + i * 16 + 4 * (lane >> 4) + e - r0;
            smem[row * LDSW + wn * WC + j * 16 + (lane & 15)] = acc[i][j][e];
          }
    }
    __syncthreads();
#pragma unroll
    for (int rb = 0; rb < ROWS_T; rb += IB) {
      f32x4 x[IB][NH];
      float rsc[IB];
      // phase 1: every row of the batch finished into registers
#pragma unroll
      for (int k = 0; k < IB; ++k) {
        const int rl = trow + (rb + k) * RSTEP;
        const int q = q0 + r0 + rl;
        const bool dead = RAG && q >= lq_live;  // beyond the clip's length (its own zero padding)
        const float rin_ = RIN ? rin[RIN ? k : 0] : 1.0f;
        if constexpr (LINES) {  // one piece per row: the 64 lanes read 1 KiB (two runs of 512 B) of the staged rows
          x[k][0] = *reinterpret_cast<const f32x4*>(smem + epi_lds_float(rl, tid, BN)) * rin_ + bias4[0];
        } else {
          const f32x4 u = *reinterpret_cast<const f32x4*>(smem + rl * LDSW + cg + 4 * hsw);
          const f32x4 v = *reinterpret_cast<const f32x4*>(smem + rl * LDSW + cg + 4 * (1 - hsw));
          x[k][0] = (hsw ? v : u) * rin_ + bias4[0];
          x[k][NH - 1] = (hsw ? u : v) * rin_ + bias4[NH - 1];
        }
#pragma unroll
        for (int h = 0; h < NH; ++h) {
          if constexpr (F::epi == EPI_GELU) {
#pragma unroll
            for (int e = 0; e < 4; e += 2) {
              const f32x2 g = gelu_bf16_f2(f32x2{x[k][h][e], x[k][h][e + 1]});
              x[k][h][e] = g[0];
              x[k][h][e + 1] = g[1];
            }
          } else if constexpr (F::epi == EPI_GAMMA_RES) {
            x[k][h] = r[k][h] + gamma4[h] * x[k][h];
          } else if constexpr (F::epi == EPI_RES) {
            x[k][h] = r[k][h] + x[k][h];
          } else {
            static_assert(F::epi == EPI_BIAS, "epilogue form");
          }
          if (dead) x[k][h] = f32x4{0.f, 0.f, 0.f, 0.f};
          if constexpr (F::mean == MEAN_MID) x[k][h] = dead ? x[k][h] : m[k][h] + x[k][h];
          if constexpr (F::mean == MEAN_LAST) x[k][h] = dead ? x[k][h] : (m[k][h] + x[k][h]) / 3.0f;
        }
        rsc[k] = osc;
        if constexpr (h2row) rsc[k] = rbnd[k];  // the row's bound; its scale is taken in phase 2
      }
      // the next batch's loads ahead of this batch's stores
      if (rb + IB < ROWS_T) load(rb + IB);
      // phase 2: SiLU, split and stores, row by row
#pragma unroll
      for (int k = 0; k < IB; ++k) {
        const int q = q0 + r0 + trow + (rb + k) * RSTEP;
        if (!FULL && q >= p.Lq) continue;
        const long long orow = (long long)q * p.out_mul + ph;
        const long long o = ob + orow * p.ldy + co;
        if constexpr (F::mean == MEAN_FIRST || F::mean == MEAN_MID) {
#pragma unroll
          for (int h = 0; h < NH; ++h) *reinterpret_cast<f32x4*>(p.macc + o + 4 * h) = x[k][h];
          continue;
        }
        float sc = rsc[k];  // the h2 output's scale for this row
        if constexpr (h2row) {
          const float bnd = rsc[k];
          const int sh = h2_shift(bnd);
          sc = __builtin_ldexpf(1.0f, sh);
          if (cg == 0 && pr.y_ash) pr.y_ash[(long long)b * p.Lq + q] = sh;
          if (pr.rflag && !(bnd <= 3.0e38f)) atomicOr(pr.rflag, RANGE_NONFINITE);
        }
        if constexpr (F::track) {
          const float ts = h2row ? sc : 1.0f;
#pragma unroll
          for (int h = 0; h < NH; ++h)
#pragma unroll
            for (int e = 0; e < 4; ++e) vmax = fmaxf(vmax, fabsf(x[k][h][e]) * ts);
        }
        if constexpr (F::y) {
#pragma unroll
          for (int h = 0; h < NH; ++h) *reinterpret_cast<f32x4*>(p.y + o + 4 * h) = x[k][h];
        }
        if constexpr (LINES) {  // (the lanes of an h2 pair own the same row, so both are here or neither)
          if constexpr (F::y6h) store_h2_pair<false>(y6, orow, p.Cout, co, x[k][0], sc);
          if constexpr (F::y2 || F::y6sh) {
            f32x4 sv;
#pragma unroll
            for (int e = 0; e < 4; ++e) sv[e] = silu_f(x[k][0][e]);
            if constexpr (F::y2) *reinterpret_cast<f32x4*>(p.y2 + o) = sv;
            if constexpr (F::y6sh) store_h2_pair<false>(y6s, orow, p.Cout, co, sv, sc);
          }
        } else {
          float xv[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) xv[e] = x[k][e >> 2][e & 3];
          if constexpr (F::y6h) store_h2_8<false>(y6, orow, p.Cout, co, xv, sc);
          if constexpr (F::y2 || F::y6sh) {
            float sv[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) sv[e] = silu_f(xv[e]);
            if constexpr (F::y2) {
              *reinterpret_cast<f32x4*>(p.y2 + o) = f32x4{sv[0], sv[1], sv[2], sv[3]};
              *reinterpret_cast<f32x4*>(p.y2 + o + 4) = f32x4{sv[4], sv[5], sv[6], sv[7]};
            }
            if constexpr (F::y6sh) store_h2_8<false>(y6s, orow, p.Cout, co, sv, sc);
          }
        }
      }
    }
  };
#pragma unroll 1
  for (int r0 = 0; r0 < BM; r0 += RPP) {
    if (q0 + r0 + RPP <= p.Lq) pass(r0, std::true_type{});
    else pass(r0, std::false_type{});
  }
  if constexpr (F::track)  // (rowwise: vmax holds scaled values, and pr.y_amax is not recorded)
    range_report_wg(vmax, h2row ? nullptr : pr.y_amax, b, h2row ? 65504.0f : h2o ? 65504.0f / osc : __builtin_inff(),
                    pr.rflag, pre.acur, smem, NT);
}

// RROW: which per-row range forms a kernel may meet (round 6).  Bit 0: an h2 input scaled per row
// (x_ash_row: the h3 one-tap kernels), loaded with the batch's rows; bit 1: a rowwise bound of an h2
// output (yb.rowwise: one-tap kernels).  Tap convs pass 0, which keeps these registers out of their
// epilogues (with them, round 6's first form spilled ~290 SGPRs into VGPR lanes in
// conv_gemm_x3dw_group: +5 % on the dominant kernel).  pr: where the range fields are read (the
// kernel argument itself in grouped launches, whose private copy then leaves them out).
// RAG: whether the epilogue looks at ConvParams::clip_len (ragged batches) at all.  The h3 kernels,
// most of a step, are instantiated both ways and launched by whether the call has lengths, so the
// padded path runs the code it ran before the lengths existed (with the null-pointer select alone the
// C2 step paid 0.6-1.2 %, DESIGN.md §5 "Ragged decode"); every other kernel keeps the select.
// F: EpiGeneric, or an EpiForm the caller has matched on the host (epi_form_is): epilogue_form.
template <int BM, int BN, int WM, int WN, int LDS_FLOATS, int NT, int RROW = 2, bool RAG = true, typename F = EpiGeneric,
          typename AccT>
__device__ __forceinline__ void epilogue_lds(const ConvParams& p, const ConvParams& pr, AccT& acc, int q0, int co0,
                                             int b, int ph, float* smem, const EpiPre* pre = nullptr) {
#ifndef DCX_EPI4  // (the A/B builds of 4-channel groups keep the generic epilogue everywhere)
  if constexpr (F::fixed) {
    epilogue_form<BM, BN, WM, WN, LDS_FLOATS, NT, RROW, RAG, F>(p, pr, acc, q0, co0, b, ph, smem, *pre);
    return;
  }
#endif
  constexpr int WR = BM / WM, WC = BN / WN;
  constexpr int TM = WR / 32, TN = WC / 32;
  constexpr bool M16 = sizeof(acc[0][0]) == 16;
  static_assert(sizeof(acc) == WR * WC * 4 / 64, "accumulator tile");
  constexpr int LDSW = BN + 4;
  constexpr int RPP = (BM * LDSW <= LDS_FLOATS) ? BM
                      : (BM / 2 * LDSW <= LDS_FLOATS) ? BM / 2
                      : (BM / 4 * LDSW <= LDS_FLOATS) ? BM / 4 : WR;
  static_assert(RPP % WR == 0 && RPP * LDSW <= LDS_FLOATS, "epilogue pass does not fit LDS");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int lrow = lane & 31, rhalf = 4 * (lane >> 5);
  const long long ob = (long long)b * p.y_bstride;
  unsigned short* y6 = p.y6 ? p.y6 + ob * layout_u16(p.y_layout) : nullptr;
  unsigned short* y6s = p.y6s ? p.y6s + ob * (p.ys_layout != LAYOUT_PLANES ? 2 : 3) : nullptr;
  // h2 output range (dcx_kernels.h h2_shift): the clip's scale from its bound program, the same in
  // every workgroup of the clip, or (pr.yb.rowwise, one-tap convs) each row's from its own bound
  // (wave-uniform values moved to scalar registers: the accumulators still occupy most VGPRs here)
  const bool h2o = (y6 && p.y_layout == LAYOUT_H2) || (y6s && p.ys_layout != LAYOUT_PLANES);
  constexpr bool RIN = RROW & 1, ROUT = RROW & 2;
  const bool h2row = ROUT && h2o && pr.yb.rowwise;
  int osh = 0;
  if (pre) {
    osh = pre->osh;
  } else if (h2o && !h2row) {
    const float bnd = range_bound(pr.yb, b);
    osh = __builtin_amdgcn_readfirstlane(h2_shift(bnd));
    if (tid == 0) {
      if (pr.y_ash) pr.y_ash[b] = osh;
      if (pr.rflag && !(bnd <= 3.0e38f)) atomicOr(pr.rflag, RANGE_NONFINITE);
    }
  }
  const float osc =
      __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, __builtin_ldexpf(1.0f, osh))));
#ifdef DCX_DIAG_NORANGE  // timing build: no range tracking in the epilogues (no maxima, no flags)
  const bool track = false;
#else
  // the clip's max |v| where a consumer's bound needs it; an h2 output checks its values against its
  // scale's limit only there (free: the max is taken anyway).  Elsewhere a finite value cannot pass
  // its bound (rigorous, from measured maxima), and a non-finite bound is flagged by the bound's own
  // evaluation (round 6: the per-element check cost ~1 VALU per element in every h2 epilogue)
  const bool track = pre ? pre->track : pr.y_amax != nullptr;
#endif
  const float acur = pre ? pre->acur : track && !h2row ? range_cur(pr.y_amax, b) : 0.f;  // the clip's running max (range_report)
  float vmax = 0.f;  // largest |v| this thread finishes (range_report)
  // ragged batch: the clip's rows that hold data; the rows from there to p.Lq are written as zeros
  const int lq_live = RAG ? clip_rows(pr.clip_len, pr.len_mul, b, p.Lq) : p.Lq;
  // Each thread finishes G consecutive output channels of a row (G = 8: 16-byte plane / compact
  // stores; the epilogue's store issue, not its bytes, sets its pace), the same channels for every
  // row, so bias and gamma are loaded once per tile.
#ifdef DCX_EPI4
  constexpr int G = 4;  // A/B builds: the round-2 form (8-byte plane stores)
#else
  constexpr int G = 8;
#endif
  constexpr int NH = G / 4;  // f32x4 halves per thread and row
  static_assert(NT % (BN / G) == 0, "each thread keeps one channel group");
  const int cg = (tid % (BN / G)) * G, trow = tid / (BN / G), co = co0 + cg;
  // LDS read order of the two halves: lanes with bit 3 set read the upper half first, which makes
  // both ds_read_b128 of a row conflict-free in every 16-lane group (MI355X_MICROARCH.md §LDS)
  const int hsw = G == 8 ? (lane >> 3) & 1 : 0;
  f32x4 bias4[NH], gamma4[NH];
#pragma unroll
  for (int h = 0; h < NH; ++h) {
    bias4[h] = p.bias ? *reinterpret_cast<const f32x4*>(p.bias + co + 4 * h) : f32x4{0.f, 0.f, 0.f, 0.f};
    gamma4[h] = p.epi == EPI_GAMMA_RES ? *reinterpret_cast<const f32x4*>(p.gamma + co + 4 * h) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
#ifdef DCX_DIAG_NOEPI
  if (q0 >= 0) return;  // timing-only build: main loop without the epilogue
#endif
#ifdef DCX_DIAG_DUP
  if (p.diag_skip == 2) return;  // the timing copy of a launch: main loop only
#endif
  // acc rows [r0, r0 + RPP) of the tile -> LDS
  auto stage_acc = [&](int r0) {
    __syncthreads();
    if (wm * WR >= r0 && wm * WR < r0 + RPP) {
      if constexpr (M16) {  // 16x16 block: lane holds column l & 15, rows 4 (l >> 4) + e
#pragma unroll
        for (int i = 0; i < WR / 16; ++i)
#pragma unroll
          for (int j = 0; j < WC / 16; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int row = wm * WR + i * 16 + 4 * (lane >> 4) + e - r0;
              smem[row * LDSW + wn * WC + j * 16 + (lane & 15)] = acc[i][j][e];
            }
      } else {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int row = wm * WR + i * 32 + (r & 3) + 8 * (r >> 2) + rhalf - r0;
              smem[row * LDSW + wn * WC + j * 32 + lrow] = acc[i][j][r];
            }
      }
    }
    __syncthreads();
  };
  // The residual / mean-accumulator rows of a batch are all loaded (unconditionally, past-the-end
  // rows clamped) before any of its stores, and the first batch of a pass before the pass's LDS
  // staging: with stores in flight hipcc can only wait with vmcnt(0), and conditional loads in a
  // rolled loop made it wait before every single load (one memory round trip per row).  The stores
  // may alias the loads (the in-place ResBlock state); each thread stores only elements it has
  // already loaded.
  constexpr int RSTEP = NT / (BN / G), ROWS_T = RPP / RSTEP;
  static_assert(RPP % RSTEP == 0, "epilogue rows per thread");
  const bool need_r = p.epi == EPI_GAMMA_RES || p.epi == EPI_RES;
  const bool need_m = p.mean_mode == MEAN_MID || p.mean_mode == MEAN_LAST;
  auto batch = [&](int r0, int rb, bool stage, auto ibt) {
    constexpr int IB = decltype(ibt)::value;
    f32x4 r[IB][NH], m[IB][NH];
    auto lofs = [&](int k) {
      const int q = min(q0 + r0 + trow + (rb + k) * RSTEP, p.Lq - 1);
      return ob + ((long long)q * p.out_mul + ph) * p.ldy + co;
    };
    if (need_r) {
#pragma unroll
      for (int k = 0; k < IB; ++k)
#pragma unroll
        for (int h = 0; h < NH; ++h) r[k][h] = *reinterpret_cast<const f32x4*>(p.res + lofs(k) + 4 * h);
    }
    if (need_m) {
#pragma unroll
      for (int k = 0; k < IB; ++k)
#pragma unroll
        for (int h = 0; h < NH; ++h) m[k][h] = *reinterpret_cast<const f32x4*>(p.macc + lofs(k) + 4 * h);
    }
    // per-row range data of a one-tap h3 conv (the input row's shift, the output row's bound), loaded
    // with the batch's other rows: inside the row loop each was a memory round trip
    // (a rowwise program has one term: prog_conv_rows)
    auto row_bound = [&](int q) { return fmaf(pr.yb.g[0], fmaxf(pr.yb.m[0][(long long)b * p.Lq + q], pr.yb.f[0]), pr.yb.c); };
    float rin[RIN ? IB : 1], rbnd[RIN ? IB : 1];
    if constexpr (RIN) {
#pragma unroll
      for (int k = 0; k < IB; ++k) {
        const int q = min(q0 + r0 + trow + (rb + k) * RSTEP, p.Lq - 1);
        rin[k] = pr.x_ash_row ? __builtin_ldexpf(1.0f, -pr.x_ash_row[(long long)b * p.Lin + q]) : 1.0f;
        rbnd[k] = h2row ? row_bound(q) : 0.f;
      }
    }
    if (stage) stage_acc(r0);
#pragma unroll
    for (int k = 0; k < IB; ++k) {
      const int rl = trow + (rb + k) * RSTEP;
      const int q = q0 + r0 + rl;
      if (q >= p.Lq) continue;
      const long long orow = (long long)q * p.out_mul + ph;
      const long long o = ob + orow * p.ldy + co;
      f32x4 x[NH];
      // a one-tap h3 conv's input scaled per row: undo the row's power of two (exact) before the bias
      const float rin_ = RIN ? rin[RIN ? k : 0] : 1.0f;
      if constexpr (NH == 2) {
        const f32x4 u = *reinterpret_cast<const f32x4*>(smem + rl * LDSW + cg + 4 * hsw);
        const f32x4 v = *reinterpret_cast<const f32x4*>(smem + rl * LDSW + cg + 4 * (1 - hsw));
        x[0] = (hsw ? v : u) * rin_ + bias4[0];
        x[1] = (hsw ? u : v) * rin_ + bias4[1];
      } else {
        x[0] = *reinterpret_cast<const f32x4*>(smem + rl * LDSW + cg) * rin_ + bias4[0];
      }
#pragma unroll
      for (int h = 0; h < NH; ++h) {
        if (p.round_bf16) x[h] = round_bf16x4(x[h]);
        switch (p.epi) {
          case EPI_GELU:
            // planes modes (x6, bf16): the branch-free GELU (abs error 4.5e-7 against fp64, below
            // torch's fp32 erff GELU's 1.2e-6); the IEEE fp32 mode keeps erff
            if (p.w6) {
#ifndef DCX_EPI_NOGELU  // timing build: the bf16 GELU left out
#pragma unroll
              for (int e = 0; e < 4; e += 2) {
                const f32x2 g = gelu_bf16_f2(f32x2{x[h][e], x[h][e + 1]});
                x[h][e] = g[0];
                x[h][e + 1] = g[1];
              }
#endif
              // a compact-only output rounds to bf16 in its store (the same RNE bits)
              if (p.round_bf16 && (p.y || y6s || p.y2 || p.y_layout != LAYOUT_BF16)) x[h] = round_bf16x4(x[h]);
            } else {
#pragma unroll
              for (int e = 0; e < 4; ++e) x[h][e] = gelu_f(x[h][e]);
            }
            break;
          case EPI_GAMMA_RES: x[h] = r[k][h] + gamma4[h] * x[h]; break;
          case EPI_RES:  // bf16 mode: ResBlock1's `xt + x` of two bf16 tensors is bf16
            x[h] = r[k][h] + x[h];
            if (p.round_bf16) x[h] = round_bf16x4(x[h]);
            break;
          case EPI_LOGCLAMP:
#pragma unroll
            for (int e = 0; e < 4; ++e) x[h][e] = logf(fmaxf(x[h][e], 1e-5f));
            break;
          default: break;
        }
        if (RAG && q >= lq_live) x[h] = f32x4{0.f, 0.f, 0.f, 0.f};  // beyond the clip's length (its own zero padding)
      }
#ifdef DCX_EPI_NOSTORE  // timing build: every output computed, (practically) none stored
      if (x[0][0] != -0x1.234p-100f) continue;
#endif
#ifdef DCX_DIAG_DUP  // the timing copy of a launch: every output computed, (practically) none stored
      if (p.diag_skip == 1 && x[0][0] != -0x1.234p-100f) continue;
#endif
      if (p.mean_mode == MEAN_FIRST) {
#pragma unroll
        for (int h = 0; h < NH; ++h) *reinterpret_cast<f32x4*>(p.macc + o + 4 * h) = x[h];
        continue;
      } else if (p.mean_mode == MEAN_MID) {
#pragma unroll
        for (int h = 0; h < NH; ++h) *reinterpret_cast<f32x4*>(p.macc + o + 4 * h) = RAG && q >= lq_live ? x[h] : m[k][h] + x[h];
        continue;
      } else if (p.mean_mode == MEAN_LAST) {
#pragma unroll
        for (int h = 0; h < NH; ++h) {  // bf16 mode: stack(...).mean(0) of bf16 tensors is bf16
          x[h] = RAG && q >= lq_live ? x[h] : (m[k][h] + x[h]) / 3.0f;
          if (p.round_bf16) x[h] = round_bf16x4(x[h]);
        }
      }
      float rsc = osc;  // the h2 output's scale for this row
      if (h2row) {
        const long long grow = (long long)b * p.Lq + q;
        const float bnd = RIN ? rbnd[RIN ? k : 0] : row_bound(q);
        const int sh = h2_shift(bnd);
        rsc = __builtin_ldexpf(1.0f, sh);
        if (cg == 0 && pr.y_ash) pr.y_ash[grow] = sh;
        if (pr.rflag && !(bnd <= 3.0e38f)) atomicOr(pr.rflag, RANGE_NONFINITE);
      }
      if (track) {  // per-row scales: the scaled values against 65504 (range_report)
        const float ts = h2row ? rsc : 1.0f;
#pragma unroll
        for (int h = 0; h < NH; ++h)
#pragma unroll
          for (int e = 0; e < 4; ++e) vmax = fmaxf(vmax, fabsf(x[h][e]) * ts);
      }
      if (p.y) {
#pragma unroll
        for (int h = 0; h < NH; ++h) *reinterpret_cast<f32x4*>(p.y + o + 4 * h) = x[h];
      }
      if constexpr (G == 8) {
        float xv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) xv[e] = x[e >> 2][e & 3];
        if (y6) {
          if (p.y_layout == LAYOUT_BF16) store_bf16x8(y6, orow, p.Cout, co, xv);
          // unreachable (run_conv rejects layout 2); kept: removing it moved registers / scratch in other kernels
          else if ((int)p.y_layout == 2) store_hm8(y6, orow, p.Cout, co, xv);
          else if (p.y_layout == LAYOUT_H2) store_h2_8<false>(y6, orow, p.Cout, co, xv, rsc);
          else store_planes8(y6, orow, p.Cout, co, xv);
        }
        if (p.y2 || y6s) {
          float sv[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) sv[e] = p.round_bf16 ? bf16_val(bf16_bits(silu_f(xv[e]))) : silu_f(xv[e]);
          if (p.y2) {
            *reinterpret_cast<f32x4*>(p.y2 + o) = f32x4{sv[0], sv[1], sv[2], sv[3]};
            *reinterpret_cast<f32x4*>(p.y2 + o + 4) = f32x4{sv[4], sv[5], sv[6], sv[7]};
          }
          if (y6s) {
            if (p.ys_layout != LAYOUT_PLANES) store_h2_8<false>(y6s, orow, p.Cout, co, sv, rsc);
            else store_planes8(y6s, orow, p.Cout, co, sv);
          }
        }
      } else {
        if (y6) {
          if (p.y_layout == LAYOUT_BF16) store_bf16x4(y6, orow, p.Cout, co, x[0][0], x[0][1], x[0][2], x[0][3]);
          // unreachable (run_conv rejects layout 2); kept: removing it moved registers / scratch in other kernels
          else if ((int)p.y_layout == 2) store_hm4(y6, orow, p.Cout, co, x[0][0], x[0][1], x[0][2], x[0][3]);
          else if (p.y_layout == LAYOUT_H2) store_h2_4<false>(y6, orow, p.Cout, co, x[0][0], x[0][1], x[0][2], x[0][3], rsc);
          else store_planes4(y6, orow, p.Cout, co, x[0][0], x[0][1], x[0][2], x[0][3]);
        }
        if (p.y2 || y6s) {
          f32x4 sv;
#pragma unroll
          for (int e = 0; e < 4; ++e) sv[e] = p.round_bf16 ? bf16_val(bf16_bits(silu_f(x[0][e]))) : silu_f(x[0][e]);
          if (p.y2) *reinterpret_cast<f32x4*>(p.y2 + o) = sv;
          if (y6s) {
            if (p.ys_layout != LAYOUT_PLANES) store_h2_4<false>(y6s, orow, p.Cout, co, sv[0], sv[1], sv[2], sv[3], rsc);
            else store_planes4(y6s, orow, p.Cout, co, sv[0], sv[1], sv[2], sv[3]);
          }
        }
      }
    }
  };
  // batches of 8 rows (4 when both the residual and the mean accumulator are loaded), halved for
  // 8-channel groups (the same registers)
  // (the largest batch within the cap that divides the rows per thread: 6 rows -> 3 + 3)
  constexpr int IBF0 = 8 / NH, IBM0 = 4 / NH;
  constexpr auto div_cap = [](int n, int cap) {
    int d = n < cap ? n : cap;
    while (n % d) --d;
    return d;
  };
  constexpr int IBF = div_cap(ROWS_T, IBF0), IBM = div_cap(ROWS_T, IBM0);
  static_assert(ROWS_T % IBF == 0 && ROWS_T % IBM == 0, "epilogue batches");
#pragma unroll 1
  for (int r0 = 0; r0 < BM; r0 += RPP) {
    if (need_m) {
#pragma unroll
      for (int rb = 0; rb < ROWS_T; rb += IBM) batch(r0, rb, rb == 0, std::integral_constant<int, IBM>{});
    } else {
#pragma unroll
      for (int rb = 0; rb < ROWS_T; rb += IBF) batch(r0, rb, rb == 0, std::integral_constant<int, IBF>{});
    }
  }
  // (rowwise: vmax holds scaled values, and pr.y_amax is not recorded)
  if (track)  // workgroup-uniform; the staging area is free after the last pass
    range_report_wg(vmax, h2row ? nullptr : pr.y_amax, b, h2row ? 65504.0f : h2o ? 65504.0f / osc : __builtin_inff(),
                    pr.rflag, acur, smem, NT);
}

// Ragged batches (ConvParams::clip_len): whether the tile of clip b that starts at output row q0 lies
// wholly beyond the clip's length.  Workgroup-uniform.  A kernel that asks before it issues any DMA
// and before its first barrier may then leave through epilogue_dead instead of its main loop.
__device__ __forceinline__ bool tile_dead(const ConvParams& p, const ConvParams& pr, int b, int q0) {
  return pr.clip_len != nullptr && q0 >= clip_rows(pr.clip_len, pr.len_mul, b, p.Lq);
}
// The epilogue of such a tile, without accumulators: what epilogue_lds writes for rows beyond the
// clip's length (zeros in every output and layout; MEAN_LAST's mean of zeros), the clip's h2 shift as
// epi_range_pre stores it (the clip may have no live tile at all), nothing into y_amax.  No LDS, no
// barrier.  Tap convs only (no per-row ranges).
template <int BM, int BN, int NT>
__device__ __forceinline__ void epilogue_dead(const ConvParams& p, const ConvParams& pr, int q0, int co0, int b, int ph) {
  const long long ob = (long long)b * p.y_bstride;
  unsigned short* y6 = p.y6 ? p.y6 + ob * layout_u16(p.y_layout) : nullptr;
  unsigned short* y6s = p.y6s ? p.y6s + ob * (p.ys_layout != LAYOUT_PLANES ? 2 : 3) : nullptr;
  const bool h2o = (y6 && p.y_layout == LAYOUT_H2) || (y6s && p.ys_layout != LAYOUT_PLANES);
  if (h2o && threadIdx.x == 0) {
    const float bnd = range_bound(pr.yb, b);
    if (pr.y_ash) pr.y_ash[b] = h2_shift(bnd);
    if (pr.rflag && !(bnd <= 3.0e38f)) atomicOr(pr.rflag, RANGE_NONFINITE);
  }
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  const float z8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  constexpr int CG = BN / 8;
  for (int i = threadIdx.x; i < BM * CG; i += NT) {
    const int q = q0 + i / CG, co = co0 + (i % CG) * 8;
    if (q >= p.Lq) break;
    const long long orow = (long long)q * p.out_mul + ph;
    const long long o = ob + orow * p.ldy + co;
    if (p.mean_mode == MEAN_FIRST || p.mean_mode == MEAN_MID) {
      *reinterpret_cast<f32x4*>(p.macc + o) = z4;
      *reinterpret_cast<f32x4*>(p.macc + o + 4) = z4;
      continue;
    }
    if (p.y) {
      *reinterpret_cast<f32x4*>(p.y + o) = z4;
      *reinterpret_cast<f32x4*>(p.y + o + 4) = z4;
    }
    if (y6) {
      if (p.y_layout == LAYOUT_BF16) store_bf16x8(y6, orow, p.Cout, co, z8);
      else if (p.y_layout == LAYOUT_H2) store_h2_8<false>(y6, orow, p.Cout, co, z8, 1.0f);
      else store_planes8(y6, orow, p.Cout, co, z8);
    }
    if (p.y2) {
      *reinterpret_cast<f32x4*>(p.y2 + o) = z4;
      *reinterpret_cast<f32x4*>(p.y2 + o + 4) = z4;
    }
    if (y6s) {
      if (p.ys_layout != LAYOUT_PLANES) store_h2_8<false>(y6s, orow, p.Cout, co, z8, 1.0f);
      else store_planes8(y6s, orow, p.Cout, co, z8);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// LDS-DMA staging (buffer_load_dwordx4 ... lds) of the ping-pong kernels, conv_gemm_x6dm onwards
// ---------------------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) void* lds_ptr_t;

__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t r, unsigned short* lds, int voff, int soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_ptr_t)lds, 16, voff, soff, 0, 0);
}
// barrier that keeps the compiler's memory ops on their side and does not drain the DMA queue
__device__ __forceinline__ void seg_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
__device__ __forceinline__ void wait_dma(int n) {  // n = DMA pieces this wave issued since the ones to retire
#define DCX_W(k) \
  case k: asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); break;
  switch (n) {
    DCX_W(1) DCX_W(2) DCX_W(3) DCX_W(4) DCX_W(5) DCX_W(6) DCX_W(7) DCX_W(8) DCX_W(9) DCX_W(10) DCX_W(11)
    DCX_W(12) DCX_W(13) DCX_W(14) DCX_W(15) DCX_W(16) DCX_W(17) DCX_W(18) DCX_W(19) DCX_W(20) DCX_W(21) DCX_W(22)
    DCX_W(23)
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
#undef DCX_W
}

}  // namespace dcx
