// Internal interface between the host orchestration (dcx_api.cpp) and the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dcx_stream_plan.h"

namespace dcx {

// Epilogue of the implicit-GEMM convolution (applied per output element v = acc + bias).
enum Epi : int {
  EPI_BIAS = 0,       // v
  EPI_GELU = 1,       // gelu_erf(v)                     ConvNeXt pwconv1 + nn.GELU()
  EPI_GAMMA_RES = 2,  // res + gamma * v                 ConvNeXt pwconv2, layer scale, residual
  EPI_RES = 3,        // res + v                         ResBlock1 `x = xt + x`
  EPI_LOGCLAMP = 4,   // log(max(v, 1e-5))               LogMelSpectrogram.compress
};

// ParallelBlock mean of the 3 ResBlock1 outputs (convnext_utils.py:137-138), folded into the
// epilogue of each ResBlock's last conv: first writes, mid adds, last adds and divides by 3.
enum Mean : int { MEAN_NONE = 0, MEAN_FIRST = 1, MEAN_MID = 2, MEAN_LAST = 3 };

constexpr int kMaxPhases = 8;

// Layout of the 16-bit image of an activation tensor [rows][C] (dcx_planes.h has the stores).  It decides
// the kernel family that may read the buffer, the bytes per element, and whether range shifts travel with it:
//  * LAYOUT_PLANES: three bf16 planes per 8 channels, [rows][C/8][plane 3][8], 6 bytes per element; hi +
//    mid + lo reproduces the fp32 value to 2^-27.  Read by the x6 kernels (hi only: the bf16-mode ones).
//  * LAYOUT_BF16 ("compact"): [rows][C] bf16, the hi plane alone, 2 bytes per element.  Read by
//    conv_gemm_bf16dm / bf16dp (bf16 mode only) and by vq_prefilter_b1 (x_pjt_in, either mode).
//  * LAYOUT_H2: fp16 h = fp16(y), l = fp16(y - h) per 32 channels, [rows][C/32][8][8], 4 bytes per element,
//    y = x * 2^shift, the shift per clip or row (h2_shift).  Read by the h3 kernels (x6 mode only).
// The values are the ones the kernels compare against (2 was the retired "hm" layout).
enum Layout : int { LAYOUT_PLANES = 0, LAYOUT_BF16 = 1, LAYOUT_H2 = 3 };
// 16-bit words per element (>= 2: the epilogues keep layout 2's unreachable arm, profiles/layout_enum_ab.md)
__host__ __device__ constexpr int layout_u16(Layout l) { return l == LAYOUT_BF16 ? 1 : (int)l >= 2 ? 2 : 3; }

// ---- h3 activation range (round 6) ------------------------------------------------------------
// An h2 pair (h = fp16(y), l = fp16(y - h)) carries 22 significant bits only while |y| lies in
// [2^-3, 2^16): below, l goes subnormal (an absolute floor of 2^-25), above, fp16 saturates.  Every
// h2 tensor is therefore stored as y = x * 2^a, with a = h2_shift(bound) chosen per clip from an
// upper bound of |x| known BEFORE the tensor is produced (scaled bound in [2^14, 2^15): a 2x margin
// under 65504), and its consumer multiplies its accumulators by 2^-(a + w3_shift) (exact).  Two
// granularities:
//  * per ROW for the one-tap (1x1) consumers, whose output row depends on one input row: a kernel
//    that sees a whole row before splitting it (LayerNorm, launch_h2_rows) takes the row's exact max;
//    the ConvNeXt MLP hidden takes G max|LayerNorm row| + max|bias| (RangeProg::rowwise);
//  * per CLIP for the tap convs (the generator): G max|input| + max|bias| (+ max|residual|) with
//    max|input| MEASURED per clip by the input's producer (ConvParams::y_amax), so the looseness of
//    one layer never compounds; a caller's tensor by its exact clip max (launch_h2_ranged).
// G is the largest absolute row sum of the weights (host).  All bounds are rigorous; with the bound
// B the per-element error is at most 2^-22 |x| + 2^-39 B.
constexpr int kH2Top = 15;
constexpr int kH2ShiftMax = 64;
__host__ __device__ inline int h2_shift(float bound) {
  if (!(bound <= 3.0e38f)) return 0;  // NaN / inf bound: unscaled (the producer raises the range flag)
  if (bound < 1e-30f) return kH2ShiftMax;
  int e = 0;
  (void)frexpf(bound, &e);  // bound = f 2^e, f in [0.5, 1): bound * 2^(15 - e) < 2^15
  const int a = kH2Top - e;
  return a < -kH2ShiftMax ? -kH2ShiftMax : a > kH2ShiftMax ? kH2ShiftMax : a;
}
// Range flag bits (dcx_range_flags): an h2 output's bound was not finite / a value exceeded it.
enum RangeFlag : int { RANGE_NONFINITE = 1, RANGE_OVER = 2 };
// Bound program of an h2 output, evaluated on the device before the tensor is written, per clip b
// (or per row, rowwise: b = the launch's global row b * Lq + q):
// c + sum_{i < n} g[i] * max(m[i] ? m[i][b] : 0, f[i]).  m: measured maxima; f: floors.
constexpr int kRangeTerms = 6;
struct RangeProg {
  const float* m[kRangeTerms];
  float g[kRangeTerms], f[kRangeTerms];
  float c;
  int n;
  int rowwise;  // m indexed by row; the shift written per row (y_ash[row])
};
// (device) the program's bound for clip b; unrolled so the kernel-argument arrays are indexed
// statically (a dynamic index would copy them to scratch)
__device__ __forceinline__ float range_bound(const RangeProg& r, long long b) {
  float v = r.c;
#pragma unroll
  for (int i = 0; i < kRangeTerms; ++i)
    if (i < r.n) v += r.g[i] * fmaxf(r.m[i] ? r.m[i][b] : 0.f, r.f[i]);
  return v;
}
// (device) the current value of a running maximum slot (agent-scope atomic load: never a value newer
// than the slot's, possibly an older one, which only costs an atomic that was not needed)
__device__ __forceinline__ float range_cur(const float* amax, long long b) {
  return amax ? __hip_atomic_load(amax + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
}
// (device) range_report for a whole workgroup of nt threads (all of them call it): the waves' maxima
// meet in LDS (barriers that leave the wave's global stores in flight) (red: nt / 64 floats the caller may overwrite, after its last LDS use) and one thread
// reports, so a launch's first round of tiles makes one atomic per workgroup, not one per wave (the
// atomics of all clips hit one L2 line)
__device__ __forceinline__ void range_report_wg(float vmax, float* amax, int b, float lim, int* rflag, float cur,
                                                float* red, int nt) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, off, 64));
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = vmax;
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  float m = 0.f;
  if (threadIdx.x == 0) {
    m = red[0];
    for (int w = 1; w < nt / 64; ++w) m = fmaxf(m, red[w]);
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // red read before any wave goes on to overwrite the LDS (persistent kernels)
  if (threadIdx.x == 0) {
    if (amax && m > cur) atomicMax(reinterpret_cast<unsigned*>(amax + b), __float_as_uint(m));
    if (rflag && m > lim) atomicOr(rflag, RANGE_OVER);
  }
}
// (device) a wave's largest |value| (vmax >= 0 per lane) into amax[b] (atomicMax on the fp32 bits,
// which order like the values for non-negative floats), and RANGE_OVER when it exceeds lim (the
// largest |value| the h2 output's scale admits; +inf when there is none).  At most one atomic per
// wave, and none when vmax does not exceed cur (range_cur of the slot, read earlier): the slots of
// all clips share one cache line, so every wave's atomic serialised in one L2 channel, and each
// later vmcnt wait of the wave (they count in issue order) waited behind it (round 6: C2 171 -> 181 ms
// before this test).
__device__ __forceinline__ void range_report(float vmax, float* amax, int b, float lim, int* rflag, float cur = -1.f) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, off, 64));
  if ((threadIdx.x & 63) == 0) {
    if (amax && vmax > cur) atomicMax(reinterpret_cast<unsigned*>(amax + b), __float_as_uint(vmax));
    if (rflag && vmax > lim) atomicOr(rflag, RANGE_OVER);
  }
}

// A/B and test switches.  dcx_create reads them from the environment ONCE into its handle
// (knobs_from_env, dcx_api.cpp) and dcx_set_knob changes them per handle; no launcher reads the
// environment, so a captured hipGraph and the eager calls after it run the same kernels.  Every
// default below is the shipped path.
struct Knobs {
  int rp_rows = 0;          // DCX_RP_R: pair-kernel tile height (an instantiated size; 0 = the launcher's choice)
  int rp_old = 0;           // DCX_RP_OLD=1: the step-schedule pair kernel (conv_res_pair) at C = 32 too
  int rp_g64 = 0;           // DCX_RP_G64=1: the barrier-free 8-wave pair kernel at C = 64
  int gelu_lut = -1;        // DCX_GELU_LUT: conv_gemm_bf16dp's table limit (-1 = the whole table, 0 = evaluated)
  int bf16_persist = 1;     // DCX_BF16_PERSIST=0: the staged bf16dm for pwconv1 instead of bf16dp
  int bf16_reg_epi = 1;     // DCX_BF16_REG_EPI=0: the LDS-staged epilogue for pwconv1 too
  int dwconv_tiled = 0;     // DCX_DWCONV_TILED=1: the round-2 tiled dwconv_ln (same bits)
  int split_min_steps = 0;  // DCX_SPLIT_MIN_STEPS: split-K only convs with at least this many K steps
  int split_group_off = 0;  // DCX_SPLIT_GROUP_OFF=1: per-conv split launches instead of grouped ones
  int h3 = 1;               // DCX_H3=0: the wide generator stages' ResBlock convs in x6 arithmetic (A/B, tests)
  int h3_bn = 0;            // DCX_H3_BN=128 / 256: the 256 x 128 / 128 x 256 h3 tiles instead of 256 x 256 (A/B)
  int h3_split = 1;         // DCX_H3_SPLIT=0: conv_gemm_x3dw's DMA issued by group 0 alone (A/B)
  int h3_pairs = 1;         // DCX_H3_PAIRS=0: the C = 32 / 64 ResBlock pairs in x6 arithmetic (A/B, tests)
  int h3_1x1 = 1;           // DCX_H3_1X1=0: the ConvNeXt blocks' 1x1 convs in x6 arithmetic (A/B, tests)
  int rp_ring = 1;          // DCX_RP_RING=0: conv_res_pair_h3's weights loaded per wave instead of the LDS ring (A/B)
  int epi_generic = 0;      // DCX_EPI_GENERIC=1: the h3 convs' run-time epilogue instead of their compile-time forms (same bits; A/B, tests)
  int conv_group = 1;       // DCX_CONV_GROUP=0: a stage's independent convs launched one by one instead of grouped (same bits; tests)
  int enc_streams = 2;      // DCX_ENC_STREAMS: half-batches on two streams, 0 off, 1 the encoder, 2 up to the generator, 3 the whole path (same bits)
};

// out[b][q*out_mul + phase][co] = epi( sum_{m<taps} sum_{ci<Cin} x[b][q + in_base[phase] + m*in_step][ci]
//                                       * w[phase][co][m*Cin + ci] + bias[co] )
// Rows of x outside [0, Lin) read as zero (zero padding).  Channels-last everywhere.
// x6 / y6 / y6s: 16-bit images of fp32 tensors [rows][C], in x_layout / y_layout / ys_layout.
struct ConvParams {
  const float* x;
  const unsigned short* x6;     // x6 mode input image (planes: row stride 3*ldx elements)
  const float* w;               // fp32 weights [phase][Cout][taps*Cin]
  const unsigned short* w6;     // if set: x6 mode, bf16 split weights [phase][tap][Cin/16][Cout][2][3][8]
  const float* bias;   // may be null
  const float* gamma;  // EPI_GAMMA_RES
  const float* res;    // EPI_GAMMA_RES / EPI_RES, layout of y
  float* y;            // v (may be null)
  float* y2;           // silu(v) (may be null)
  float* macc;         // mean accumulator, layout of y (MEAN_* != NONE)
  unsigned short* y6;  // image of v (may be null; needs ldy == Cout)
  unsigned short* y6s; // image of silu(v) (may be null)
  long long x_bstride;      // elements between clips in x
  long long y_bstride;      // elements between clips in y / y2 / res / macc
  long long w_phase_stride; // elements between phases in w
  int Lin, Lq, Cin, Cout, ldx, ldy;
  int taps, in_step, out_mul;
  int in_base[kMaxPhases];
  int epi, mean_mode;
  // argmin epilogue (VQ search)
  const float* x2;      // [rows] squared norms of x rows
  const float* e2;      // [Cout] squared norms of the codebook rows
  float* part_val;      // [rows][ntiles]
  int* part_idx;        // [rows][ntiles]
  float* part_val2;     // [rows][ntiles] second-smallest value (VQ prefilter)
  // planes-mode arithmetic: 6 = x6 (fp32-accurate), 1 = bf16 (hi plane only, one product);
  // round_bf16: round the GEMM result (after bias, and after GELU) to bf16 like torch.autocast
  int nprod, round_bf16;
  // persistent x6 kernels: tiles are enumerated over (phase, clip, row tile, column tile)
  int batch, phases;
  // fp32-input (AF32) kernels: apply silu to the input while staging (the producer then writes
  // only the fp32 tensor, not its silu as well)
  int silu_in;
  // layouts of x6 and y6 (LAYOUT_BF16 output: ldy == Cout)
  Layout x_layout, y_layout;
  // bf16-mode 1x1 weights as [phase][Cin/32][Cout][32] bf16 (hi only; conv_gemm_bf16dm), or null;
  // for vq_prefilter_b1: the codebook in the same layout (compact_pack, dcx_api.cpp).
  const unsigned short* wc;
  // split-K (conv_gemm_x6pp / x6lm only): ksplit > 1 slices over input-channel chunks, each a
  // whole number of kunit chunks; batch = clips * ksplit, and slice s of clip c is output clip
  // s * clips + c (partial sums, plain fp32: launch_splitk_epilogue finishes them)
  int ksplit, kunit;
  // diagnostic builds (-DDCX_DIAG_DUP) only: 1 = compute the epilogue but store nothing, 2 = no
  // epilogue at all (a timing copy launched before the real launch, on the real inputs)
  int diag_skip;
  // conv_gemm_bf16dp with GELU: > 0 = GELU from its LDS table of the bf16 GELU (same bits), a wave
  // with a table offset >= gelu_lut storing the evaluated epilogue instead; 0 = evaluated (set by
  // launch_conv from kn)
  int gelu_lut;
  // the handle's switches (host only; null = the defaults)
  const Knobs* kn;
  // host only: the kernel family must not follow the row count Lq, so launch_conv keeps the 256 x 128
  // tiles where big_tiles_pay would take the 64K-output ones (a ragged batch's one-tap DFT and stem:
  // a clip's bits must not depend on how many rows share its launch)
  int fixed_tiles;
  // h3 arithmetic (conv_gemm_x3dq, x_layout == LAYOUT_H2): weights fp16 h / l of w * 2^w3_shift, steps
  // [phase][tap][Cin/32] of Cout * 128 bytes, each in the order of dcx_w3_layout.h (w3_offset)
  const unsigned short* w3;
  int w3_shift;
  // layout of y6s: planes, or h2 (the input of a following h3 conv); never compact
  Layout ys_layout;
  // h3 activation range (round 6, see h2_shift): the h2 input holds x * 2^x_ash[clip] (x_ash null:
  // x_ash_c for every clip); an h2 output (y6 or y6s in LAYOUT_H2) is written as
  // v * 2^h2_shift(yb(clip)) and that shift stored to y_ash[clip] (may be null); y_amax (may be null)
  // receives the per-clip max |v| of the epilogue's final value v (atomicMax on the fp32 bits);
  // rflag (may be null) the RangeFlag bits
  const int* x_ash;
  int x_ash_c;
  const int* x_ash_row;  // one-tap convs: a per-row shift of the input row b * Lin + q (epilogue_lds)
  int* y_ash;
  float* y_amax;
  RangeProg yb;
  int* rflag;
  // ragged batch (dcx_generate_ragged): clip b holds clip_len[b] frames (device memory, clamped to the
  // launch's padded length) of len_mul output rows q each (a ConvT: per phase).  The epilogue writes
  // rows q >= clip_len[b] * len_mul as zeros in every output and keeps them out of y_amax, so every
  // consumer reads the zero padding the clip sees alone; the main loop of a tile wholly beyond the
  // length is skipped where the kernel can.  Null: every clip has Lq rows (same bits
  // as before the field existed).  Read in place from the kernel argument, like the range fields.
  const int* clip_len;
  int len_mul;
};

// (device) the rows of clip b that hold data: all `full` of them, or the clip's own length in rows
// (ConvParams::clip_len), clamped to [0, full].  Wave-uniform.
__device__ __forceinline__ int clip_rows(const int* clip_len, int len_mul, int b, int full) {
  if (!clip_len) return full;
  const long long r = (long long)max(clip_len[b], 0) * len_mul;
  return __builtin_amdgcn_readfirstlane((int)(r < full ? r : full));
}

// Independent convs issued as one launch (launch_conv_group); problem k owns logical tiles
// [start[k], start[k + 1]), tiles_per_clip[k] per clip.
constexpr int kMaxGroup = 3;
struct ConvGroup {
  ConvParams p[kMaxGroup];
  int start[kMaxGroup + 1];
  int tiles_per_clip[kMaxGroup];
};

// The reduces of a grouped split-K launch (launch_splitk_epilogue_group): member k's partials
// part[k] (splits[k] slices, stride[k] floats apart) finished with p[k]'s epilogue by the blocks
// [start[k], start[k + 1]), total4[k] 4-channel groups.
struct SplitEpiGroup {
  ConvParams p[kMaxGroup];
  const float* part[kMaxGroup];
  int splits[kMaxGroup];
  long long stride[kMaxGroup], total4[kMaxGroup];
  int start[kMaxGroup + 1];
  // chain (> 0: the member count): the members are a ParallelBlock's last convs with the mean folded
  // into their epilogues (MEAN_FIRST, MID.., LAST on one accumulator); one thread finishes an element
  // of every member in member order, so the mean is accumulated in ResBlock order as the per-conv
  // reduces do
  int chain;
};

// One pair (c1 dilated, c2 undilated) of each ResBlock1 of a small-channel ParallelBlock (C = 32 / 64,
// x6 arithmetic), fused: silu(c1) stays in LDS (dcx_resblock.hip).  Member m reads state src[m]
// ([clip][L][C] fp32) and writes src[m] + c2(silu(c1(silu(src[m])))) to dst[m] (dst != src: the
// tap halo makes in-place updates race), or, with mean_out set, silu of the mean over the members
// (ParralelBlock, ResBlock order) to mean_out.  Weights: the x6 planes packing of ConvParams::w6.
struct ResPairParams {
  const float* src[kMaxGroup];
  float* dst[kMaxGroup];
  const unsigned short* w1[kMaxGroup];
  const unsigned short* w2[kMaxGroup];
  const float* b1[kMaxGroup];
  const float* b2[kMaxGroup];
  int taps[kMaxGroup], dil[kMaxGroup];  // c1 taps (odd, (taps - 1) / 2 <= 8) and dilation (reach <= 32)
  int nmem;
  float* mean_out;
  long long bstride;  // elements between clips
  int L, batch, C;
  // h3 (conv_res_pair_h3): w1 / w2 are the ConvParams::w3 weights, scaled by 2^w3_shift{1,2}[m]
  int h3;
  int w3_shift1[kMaxGroup], w3_shift2[kMaxGroup];
  // h3 activation range (round 6): member m's S image is silu(src) * 2^h2_shift(src_amax[m][clip]),
  // its T image silu(c1 + b1) * 2^h2_shift(g1[m] src_amax[m][clip] + bm1[m]) (g1: the c1 weights'
  // largest absolute row sum, bm1: max |b1|); dst_amax[m] (may be null) receives the per-clip max
  // |dst| (atomicMax) for the next pair's S image.  src_amax null: 0 (x6 kernels ignore all of it).
  const float* src_amax[kMaxGroup];
  float* dst_amax[kMaxGroup];
  float g1[kMaxGroup], bm1[kMaxGroup];
  int* rflag;
  const Knobs* kn;  // host only; null = the defaults
  // ragged batch (ConvParams::clip_len; conv_res_pair_h3 only, launch_res_pair refuses the others):
  // clip b holds clip_len[b] * len_mul of its L rows.  The T image is zero from there on, dst and
  // mean_out are written as zeros there and stay out of dst_amax.  Null: L rows per clip.
  const int* clip_len;
  int len_mul;
};

// Launchers (all stream-ordered, no allocation).  Return hipError_t of the launch.
hipError_t launch_conv(const ConvParams& p, int batch, int phases, hipStream_t s, const char** kname);
// n <= kMaxGroup independent single-phase convs with one column tiling as one launch of the
// LDS-DMA 16x16x32 kernel; hipErrorNotSupported when they do not all qualify (the caller then
// launches them one by one, which gives the same bits).
hipError_t launch_conv_group(const ConvParams* ps, int n, int batch, hipStream_t s, const char** kname);
hipError_t launch_res_pair(const ResPairParams& p, hipStream_t s, const char** kname);
// Launches of the conv_gemm_x3dw kernels (single and grouped) so far in this process, by epilogue form
// (dcx_conv_h3.hip: the nine forms in their order there, then the run-time epilogue), optionally reset.
constexpr int kEpiFormCounters = 10;
void epi_form_launches(long long* out, bool reset);
// Split-K latency mode: the reduce kernel that sums `splits` fp32 partial outputs of a
// ConvParams::ksplit launch (laid out like p.y, `stride` floats apart, in order) and applies p's
// whole epilogue (bias, epi, mean, every output and layout).
hipError_t launch_splitk_epilogue(const ConvParams& p, const float* partials, int splits, long long stride, int batch,
                                  int phases, hipStream_t s);
// Split-K latency mode, grouped (round 4): n <= kMaxGroup single-phase halo convs (ResBlock convs:
// Cout % 128, taps >= 3), member k with its own ps[k].ksplit (1 = unsplit: the member's epilogue runs
// in the conv) and virtual clips batch * ksplit, as one conv_gemm_x6pp launch; then one launch of
// the reduces of the split members.  hipErrorNotSupported when the members do not qualify.
hipError_t launch_conv_split_group(const ConvParams* ps, int n, int batch, hipStream_t s, const char** kname);
hipError_t launch_splitk_epilogue_group(const ConvParams* ps, const float* const* partials, const int* splits,
                                        const long long* strides, int n, int batch, bool chain, hipStream_t s);
hipError_t launch_vq_argmin(const ConvParams& p, int rows, hipStream_t s, const char** kname);
int vq_argmin_ntiles(int ncodes);
// per-row partial count of the prefilter launch_vq_prefilter runs with x_pjt_in in x_layout (planes / compact)
int vq_prefilter_ntiles(int ncodes, int dim, Layout x_layout);
// VQ search, x6 / bf16 mode: prefilter (approximate squared distances, per-tile top 2) ...
// p.x_layout == LAYOUT_BF16 with p.wc the [CD/32][NC][32] bf16 hi codebook: vq_prefilter_b1 (one product,
// both modes; vq_b1_takes).  LAYOUT_PLANES (p.w6 the planes codebook): vq_prefilter_dm
// or, where its shape limits fail, vq_prefilter_x3 (three products); x_bf16: the rows of x are bf16
// values (mid and lo planes zero), which drops the mid*hi product.
hipError_t launch_vq_prefilter(const ConvParams& p, int rows, bool x_bf16, hipStream_t s, const char** kname);
bool vq_b1_takes(int ncodes, int dim);
// ... then per row: certify the prefilter's winner with a rigorous error bound, or rescore every
// candidate inside the bound in fp64.  stats (optional): [0] rows rescored, [1] codes rescored.
constexpr float kVqPrefilterBound = 2.5e-4f;
// Coefficient cx of |x| in the half-width of the prefilter's error for x_pjt_in in layout x_layout
// (vq_rescore: bound = 2 (cx |x| + max|e| |x_r|) + 8 2^-24 (|x|^2 + max|e|^2)); dmax = max |e - bf16(e)|.
double vq_prefilter_cx(Layout x_layout, int ncodes, int dim, float emax, float dmax);
// vq_rescore arguments.  part_*: the prefilter's [rows][ntiles] partials; x: x_pjt_in fp32
// [rows][dim]; x2 / x2d: |x|^2 per row (row_sqnorm, fp32 / fp64); xr2 (optional): |x - bf16(x)|^2,
// required for vq_prefilter_b1's bound; e2d: |e|^2 per code in fp64; cx / emax / e2max: the bound
// (vq_prefilter_cx).  Workspace: pairs [cap] candidate list (cap a multiple of 8), cdist / ccode
// [cap / 8] per-chunk results, row_list [rows], npairs (zeroed by row_sqnorm before the prefilter).  stats (optional): [0] rows rescored, [1] codes rescored.
struct VqRescoreArgs {
  const float *part_val, *part_val2;
  const int* part_idx;
  long long rows;
  int ntiles, tile_codes, dim;
  const float *x, *x2, *xr2;
  const double* x2d;
  const float* codebook;
  const double* e2d;
  double cx;
  float emax, e2max;
  int32_t* codes;
  int* stats;
  int2* pairs;
  double* cdist;
  int* ccode;
  long long cap;
  int2* row_list;
  unsigned long long* npairs;
};
// the rescore's three launches, in this order (vq_certify lists, vq_pair_eval evaluates, vq_pair_reduce picks)
hipError_t launch_vq_certify(const VqRescoreArgs& a, hipStream_t s);
hipError_t launch_vq_pair_eval(const VqRescoreArgs& a, hipStream_t s);
hipError_t launch_vq_pair_reduce(const VqRescoreArgs& a, hipStream_t s);
hipError_t launch_vq_reduce(const float* part_val, const int* part_idx, int rows, int ntiles, int32_t* codes,
                            hipStream_t s);
// x2 (fp32) and optionally x2d (fp64) |x|^2, xr2 |x - bf16(x)|^2 per row; zero_me (optional) set to 0
hipError_t launch_row_sqnorm(const float* x, long long rows, int C, float* out, double* x2d, float* xr2,
                             unsigned long long* zero_me, hipStream_t s);
// lay: the layout of y6; channels_first_form: 0 F.layer_norm, 1 the
// reference's channels_first LayerNorm, 2 the latter on a bf16 input under CUDA autocast.
// An h2 output is scaled per row by 2^h2_shift(the row's max |output|), that shift stored
// to ash_row[row] (required) and the max to amax_row[row] (may be null)
hipError_t launch_ln_rows(const float* x, float* y, unsigned short* y6, Layout lay, const float* w, const float* b,
                          long long rows, int C, float eps, int channels_first_form, hipStream_t s,
                          int* ash_row = nullptr, float* amax_row = nullptr);
// bf16: the reference's CUDA autocast (DCX_GEMM_BF16): input, taps and bias rounded to bf16, the
// depthwise conv's result rounded to bf16, then the fp32 F.layer_norm
hipError_t launch_dwconv_ln(const float* x, float* y, unsigned short* y6, Layout lay, const float* dww, const float* dwb,
                            const float* lnw, const float* lnb, int batch, int L, int C, int bf16, const Knobs* kn,
                            hipStream_t s, int* ash_row = nullptr, float* amax_row = nullptr);
// fp32 [rows][C] -> h2, each row scaled by 2^h2_shift(its max |x|), the shift to ash_row[row] (the
// input of a one-tap h3 conv handed in by the caller or written in fp32 by its producer)
hipError_t launch_h2_rows(const float* x, unsigned short* y6, long long rows, int C, int* ash_row, hipStream_t s);
// h3 activation range of a tensor handed in by the caller (round 6): amax[b] = max |x| over clip b's
// rows (batch clips of L rows, C channels; amax zeroed here first), then y6 = h2 of f(x) * 2^a with
// a = h2_shift(max(amax[b], floor)) stored to ash[b]; f = silu when silu != 0 (its |f(x)| <= |x|).
// yf (may be null) receives f(x) in fp32.
// clip_len (may be null; device, frames of len_mul rows): rows at or beyond clip b's length are not
// read; they count as zeros in the max and are written as zeros
hipError_t launch_h2_ranged(const float* x, float* yf, unsigned short* y6, int batch, long long L, int C, int silu,
                            float floor, float* amax, int* ash, int* rflag, hipStream_t s,
                            const int* clip_len = nullptr, int len_mul = 1);
// n 32-bit words zeroed by a kernel (capture-safe ordering; hipMemsetAsync is not used on the path)
hipError_t launch_zero_words(void* p, long long n, hipStream_t s);
// amax[b] = max |x| over clip b (batch clips of L rows, C channels), amax zeroed here first
hipError_t launch_clip_amax(const float* x, int batch, long long L, int C, float* amax, hipStream_t s,
                            const int* clip_len = nullptr, int len_mul = 1);
// the CU count of the current device (cached per device, thread-safe)
int device_cus();
// whether conv_gemm_bf16dm takes a one-tap conv of this shape (then its input may be compact)
bool bf16dm_takes(int cin, int cout, int lq, int ldx, int phases);
// Ragged (packed) batch, dcx_ragged.hip: clip b owns samples [cu_samples[b], cu_samples[b + 1]) of the
// packed audio (no pad stored) and rows [cu_frames[b], cu_frames[b + 1]) of every [sum T][C] tensor.
// The dwconv_ln work items never straddle a clip: cu_t16 / cu_t4 count each clip's 16- and 4-row tiles,
// cu_run its runs of rw rows (rw chosen from the total row count as launch_dwconv_ln chooses it).
// The five prefix arrays ([batch + 1] ints each) are device pointers into the uploaded plan table; the
// totals are the host's copy of their last entries.
// The slot form (n_dev non-null; dcx_tokenize_slots): the padded layout instead, `batch` equal slots of
// slot_samples samples and slot_frames rows, slot b holding n_dev[b] samples (DEVICE memory, clamped by
// the kernels to [0, slot_samples]) and the rows a clip of that many samples has alone: none below
// fr_min samples, else (n + fr_extra - fr_nfft) / fr_hop + 1 (dcx_num_frames(n + 1)).  The prefix arrays
// are then null, the work items are enumerated over every slot's whole row count (rows, n_t16, n_t4,
// n_run: batch times a slot's), and the rows beyond a slot's length are written as zeros.
struct RaggedSeg {
  const int *cu_samples, *cu_frames, *cu_t16, *cu_t4, *cu_run;
  int batch, rw;
  int rows, n_t16, n_t4, n_run;
  const int* n_dev;
  int slot_samples, slot_frames, fr_extra, fr_nfft, fr_hop, fr_min;
};
// rows [r0, r0 + frames) of slot b of codes [batch][frames][R] set to -1 and of pin [batch][frames][dim]
// (may be null) to zero, r0 the slot's length as the slot form of RaggedSeg defines it
hipError_t launch_slots_mask(const RaggedSeg& g, int32_t* codes, int R, float* pin, int dim, hipStream_t s);
// rows per register-ring run of a dwconv_ln launch of `rows` rows (launch_dwconv_ln's rule)
inline int dwconv_run_rows(long long rows) {
  return rows >= 2048LL * 32 ? 32 : rows >= 2048LL * 16 ? 16 : rows >= 2048LL * 8 ? 8 : 4;
}
// STFT input of a ragged batch: whole frames [sum T][n_fft] (fp32 and / or planes) of each clip's
// signal with the reference's leading zero sample and `pad` reflected samples on both sides
hipError_t launch_ragged_frames(const float* audio, const RaggedSeg& g, float* frames, unsigned short* frames6,
                                int n_fft, int hop, int pad, hipStream_t s);
// y[row][j] = x[row + j - taps / 2] for rows of the same clip, zeros beyond the clip's edges; a row of
// x is row_bytes bytes (a multiple of 16) in any layout whose tap-major concatenation is the layout
// of [rows][taps * C] (fp32, planes)
hipError_t launch_ragged_unfold(const void* x, void* y, const RaggedSeg& g, int row_bytes, int taps, hipStream_t s);
// launch_dwconv_ln on a ragged batch: taps outside the row's own clip are dropped
hipError_t launch_dwconv_ln_ragged(const float* x, float* y, unsigned short* y6, Layout lay, const float* dww,
                                   const float* dwb, const float* lnw, const float* lnb, const RaggedSeg& g, int C,
                                   int bf16, const Knobs* kn, hipStream_t s, int* ash_row = nullptr,
                                   float* amax_row = nullptr);
hipError_t launch_frame_pad(const float* audio, float* frames, unsigned short* frames6, int batch, long long n, int rows,
                            int hop, int pad_left, hipStream_t s);
// lay: the layout of y6, planes or h2 (unscaled)
hipError_t launch_silu_act(const float* x, float* yf, unsigned short* y6, long long rows, int C, hipStream_t s,
                           Layout lay = LAYOUT_PLANES);
hipError_t launch_spec_mag(const float* spec, float* mag, unsigned short* mag6, float* loglin, long long rows, int nbins,
                           int ld_out, hipStream_t s);
hipError_t launch_split_planes(const float* x, unsigned short* y6, long long rows, int C, Layout lay, hipStream_t s);
// clip_len (may be null; device): the rows are clips of `frames` rows, and a row at or beyond its
// clip's length is written as zeros without reading (or counting) its index
hipError_t launch_gather_rows(const float* table, int ntable, const int32_t* idx, long long rows, int width,
                              float* out, int32_t* n_invalid, int masked_row, hipStream_t s,
                              const int* clip_len = nullptr, long long frames = 0);
// ---- residual VQ (dcx_rvq.hip) ----
constexpr int kMaxCodebooks = 8;  // DCX_MAX_CODEBOOKS
// One layer's step of the chain on [rows][dim] fp32 rows (vq_residual_step): ck [rows] the layer's
// codes, codes_out (optional) the [rows][R] codes tensor at this layer's column, fup (optional) = e
// (fup_first) or += e, dst = src - e (null: the last layer; may be src) with its image op6 in
// op_layout (planes / compact bf16) and the row quantities of launch_row_sqnorm (x2, x2d, xr2,
// zero_me), each optional.
struct VqResidualArgs {
  const float* src;
  const float* codebook;
  const int32_t* ck;
  int32_t* codes_out;
  float* dst;
  unsigned short* op6;
  Layout op_layout;
  float *x2, *xr2;
  double* x2d;
  unsigned long long* zero_me;
  float* fup;
  int fup_first;
  long long rows;
  int dim, ncodes, R;
};
hipError_t launch_vq_residual_step(const VqResidualArgs& a, hipStream_t s);
// out[row] = sum over the R layers of table[k][idx[row][k]] in fp32, in layer order; an index -1 adds
// nothing, the wrap / invalid-count / clip_len rules are launch_gather_rows'.  out (fp32) and / or out6
// in out_layout (planes / compact bf16).
struct GatherSumArgs {
  const float* table[kMaxCodebooks];
  const int32_t* idx;
  float* out;
  unsigned short* out6;
  Layout out_layout;
  int32_t* n_invalid;
  const int* clip_len;
  long long frames;
  long long rows;
  int dim, ncodes, R;
};
hipError_t launch_gather_sum_rows(const GatherSumArgs& a, hipStream_t s);
// rows [r0, r1) of every clip of x [batch][L][C] set to zero, r0 = clip_len[b] * len_mul (ragged batches)
hipError_t launch_zero_tail_rows(float* x, int batch, long long L, int C, const int* clip_len, int len_mul,
                                 hipStream_t s);
// clip_len (may be null; device, frames of len_mul samples): input rows at or beyond the clip's length
// read as zeros and the samples there are written as zeros (a block wholly beyond it computes nothing)
hipError_t launch_conv_post_tanh(const float* x, const float* w, float bias, float* out, int batch, int L, int C,
                                 int k, int bf16, hipStream_t s, const int* clip_len = nullptr, int len_mul = 1);
// ---- token streams (dcx_stream.hip; DESIGN.md §3 "Token streams") ----
// The caller's state buffer of `sessions` slots, push size P, halo h, W = P + 2 h window frames, R codes
// per frame: eleven [sessions] int arrays (the counters of dcx_stream_plan.h; the counters a step
// leaves, committed by the emit kernel once every launch before it was accepted; the step's outputs),
// the code ring [sessions][W][R] (frame f at row f % W), the step's window [sessions][W][R] and its
// waveform [sessions][W * hop], each part on a 256-byte boundary.
struct StreamState {
  int *T, *E, *closed;           // the slots' counters
  int *T_next, *E_next, *closed_next;
  int *len, *skip, *take, *t_old, *n;  // the step's outputs
  int32_t *ring, *window;
  float* wav;
  int sessions, push, halo, W, R, hop;
};
constexpr int kStreamCounters = 11;
constexpr int kStreamMaxSessions = 65535, kStreamMaxFrames = 1 << 16;  // grid.y; push and halo each
// the views of a state buffer at `base` (may be null: sizing) and its size in bytes
inline size_t stream_state_layout(void* base, int sessions, int push, int halo, int R, int hop, StreamState& st) {
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t B = (size_t)sessions, W = (size_t)push + 2 * (size_t)halo;
  char* p = (char*)base;
  size_t off = 0;
  int** ctr[kStreamCounters] = {&st.T, &st.E, &st.closed, &st.T_next, &st.E_next, &st.closed_next,
                                &st.len, &st.skip, &st.take, &st.t_old, &st.n};
  for (int i = 0; i < kStreamCounters; ++i) *ctr[i] = (int*)(p + off + i * B * sizeof(int));
  off = up(off + kStreamCounters * B * sizeof(int));
  st.ring = (int32_t*)(p + off);
  off = up(off + B * W * R * sizeof(int32_t));
  st.window = (int32_t*)(p + off);
  off = up(off + B * W * R * sizeof(int32_t));
  st.wav = (float*)(p + off);
  off = up(off + B * W * hop * sizeof(float));
  st.sessions = sessions; st.push = push; st.halo = halo; st.W = (int)W; st.R = R; st.hop = hop;
  return off;
}
// every slot empty (the counters zeroed; the ring is only read where a step wrote it)
hipError_t launch_stream_reset(const StreamState& st, hipStream_t s);
// one thread per slot: stream_plan_step on the slot's counters with n_new[b] / flags[b] (device), the
// step's outputs and the counters it leaves written to the state
hipError_t launch_stream_plan(const StreamState& st, const int* n_new, const int* flags, hipStream_t s);
// window[b][j] = code frame T - len + j for j < len (zeros beyond), from the ring or, for the frames this
// step appends, from new_codes [sessions][push][R], which are stored into the ring too; n_invalid (may be
// null) counts the appended codes outside the codebook by launch_gather_rows' rule
hipError_t launch_stream_window(const StreamState& st, const int32_t* new_codes, int ncodes, int32_t* n_invalid,
                                hipStream_t s);
// out[b] = the window waveform's frames [skip, skip + take), then zeros up to (push + halo) * hop samples;
// n_out[b] = take; the slot's counters take the values the plan kernel left
hipError_t launch_stream_emit(const StreamState& st, float* out, int* n_out, hipStream_t s);
// ---- audio streams (dcx_stream.hip; DESIGN.md §3 "Audio streams") ----
// The caller's state buffer of `sessions` slots, push size P (raw samples), halo h (frames): twelve
// [sessions] int arrays (the counters of dcx_stream_plan.h's AudioSlot, the counters a step leaves, the
// step's outputs), the sample ring [sessions][Ws] (raw sample r at r % Ws), the step's window
// [sessions][Ws], its codes [sessions][Wf][R] and, when asked for (CD > 0), its x_pjt_in
// [sessions][Wf][CD], each part on a 256-byte boundary.  Ws = audio_window_samples, Wf = Ws / hop its
// frames, K = audio_take_max the rows of the step's outputs.
struct AudioStreamState {
  int *M, *C, *closed;
  int *M_next, *C_next, *closed_next;
  int *len, *start, *skip, *take, *m_old, *n;  // the step's outputs
  float *ring, *window;
  int32_t* codes;
  float* pin;
  int sessions, push, halo, Ws, Wf, K, R, CD;
  AudioGeom geo;
};
constexpr int kAudioStreamCounters = 12;
constexpr int kAudioStreamMaxPush = 1 << 24;  // samples
inline size_t audio_stream_state_layout(void* base, int sessions, int push, int halo, int R, int CD, const AudioGeom& geo,
                                        AudioStreamState& st) {
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t B = (size_t)sessions, Ws = (size_t)audio_window_samples(geo, halo, push), Wf = Ws / geo.hop;
  char* p = (char*)base;
  size_t off = 0;
  int** ctr[kAudioStreamCounters] = {&st.M, &st.C, &st.closed, &st.M_next, &st.C_next, &st.closed_next,
                                     &st.len, &st.start, &st.skip, &st.take, &st.m_old, &st.n};
  for (int i = 0; i < kAudioStreamCounters; ++i) *ctr[i] = (int*)(p + off + i * B * sizeof(int));
  off = up(off + kAudioStreamCounters * B * sizeof(int));
  st.ring = (float*)(p + off);
  off = up(off + B * Ws * sizeof(float));
  st.window = (float*)(p + off);
  off = up(off + B * Ws * sizeof(float));
  st.codes = (int32_t*)(p + off);
  off = up(off + B * Wf * R * sizeof(int32_t));
  st.pin = CD > 0 ? (float*)(p + off) : nullptr;
  if (CD > 0) off = up(off + B * Wf * CD * sizeof(float));
  st.sessions = sessions; st.push = push; st.halo = halo; st.Ws = (int)Ws; st.Wf = (int)Wf;
  st.K = (int)audio_take_max(geo, halo, push); st.R = R; st.CD = CD; st.geo = geo;
  return off;
}
// every slot empty (the counters zeroed; the ring is only read where a step wrote it)
hipError_t launch_audio_stream_reset(const AudioStreamState& st, hipStream_t s);
// one thread per slot: audio_plan_step on the slot's counters with n_new[b] / flags[b] (device)
hipError_t launch_audio_stream_plan(const AudioStreamState& st, const int* n_new, const int* flags, hipStream_t s);
// the step's n samples of new_samples [sessions][push] appended to the ring, and window[b][j] = raw sample
// start + j for j < len (zeros beyond), from the ring or from the samples this step appends
hipError_t launch_audio_stream_window(const AudioStreamState& st, const float* new_samples, hipStream_t s);
// codes_out[b] = the window's code rows [skip, skip + take), then -1 up to K rows; pin_out (may be null)
// the same rows of the window's x_pjt_in, then zeros; n_out[b] = take; the slot's counters take the
// values the plan kernel left
hipError_t launch_audio_stream_emit(const AudioStreamState& st, int32_t* codes_out, int* n_out, float* pin_out,
                                    hipStream_t s);

hipError_t launch_transpose(const float* in, float* out, int batch, long long rows, long long cols, hipStream_t s);
hipError_t launch_resample_poly(const float* x, int batch, long long n_in, long long xs, const double* h, int hlen,
                                int up, int down, long long pre, float* y, long long n_out, long long ys,
                                hipStream_t s);

}  // namespace dcx
