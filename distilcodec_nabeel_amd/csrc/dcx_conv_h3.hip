// The h3 conv kernels (fp16 "h2" operands, three products): conv_gemm_x3dq / x3dm and the wide-tile
// conv_gemm_x3dw, their grouped forms, tile choice and launchers.  Fragment maps: dcx_conv.hip.
#include <atomic>

#include "dcx_conv_common.h"
#include "dcx_conv_launch.h"
#include "dcx_conv_pingpong.h"
#include "dcx_a3_layout.h"
#include "dcx_w3_layout.h"

namespace dcx {

DCX_DIAG_FILE(h3)

// ---------------------------------------------------------------------------------------------
// conv_gemm_x3dq: the fp16 "h3" arithmetic (round 5) on conv_gemm_x6dq's LDS-DMA ping-pong schedule.
//
// An fp32 value is held as two fp16 values, h = fp16(x) and l = fp16(x - h) (dcx_planes.h "h2"
// layout, 22 significant bits), the weights likewise after scaling by 2^w3_shift (the largest |w|
// just below 2^15, so l stays normal for all weights within 2^-18 of it); the accumulators are
// scaled back by 2^-w3_shift before the epilogue.  A product keeps three terms, hh' + hl' + lh'
// (ll' is 2^-22 relative), against x6's six, at the same K32 rate per MFMA
// (v_mfma_f32_16x16x32_f16; the K16 f16 MFMA issues at half rate on gfx950, tools/probe).
// A step is one 32-channel chunk of one tap; per 16 x 16 block three MFMAs, A{h} . B{l'},
// A{l} . B{h'} and A{h} . B{h'}, the lanes of K group kg = lane >> 4 holding channel group kg
// (8 channels) of every operand, so a lane reads h and l of its rows and h' and l' of its columns
// once per step.
// Tiles BM x BN = 128 x 256 (BN = 256) or 256 x 128, 8 waves of 64 x 64 (group 0 the upper half of
// the rows); every fragment of a step (8 A + 8 B ds_read_b128) is read in the memory segment and
// an MFMA segment is 48 MFMAs.  LDS images, piece-major and row-linear: A [piece 8][BM + 64][16 B]
// (two buffers, by chunk parity), B [piece 8][BN][16 B] (3-slot ring), piece = plane * 4 + channel
// group; one 1 KiB DMA instruction fills 64 rows of one piece.  Rows of one piece are 16 B apart,
// so a ds_read_b128 lane group (16 distinct rows mod 16) is conflict-free at any tap offset.
// The A buffer of chunk c + 2 is issued taps - 2 segments after chunk c's last read: taps >= 3.
// ---------------------------------------------------------------------------------------------
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// The epilogue forms (dcx_conv_common.h EpiForm) the host code produces on these kernels in x6 mode;
// anything else (bf16 rounding, planes or compact outputs, DCX_EPI_GENERIC=1) runs EpiGeneric.
//                       epi            mean        y      y2     y6h    y6sh   track  rowwise
using EpiC1 = EpiForm<EPI_BIAS, MEAN_NONE, false, false, false, true, true>;        // conv_pre, a pair's c1: silu in h2
using EpiUp = EpiForm<EPI_BIAS, MEAN_NONE, true, false, false, true, true>;         // ConvT: fp32 and silu in h2
using EpiC2 = EpiForm<EPI_RES, MEAN_NONE, true, false, false, true, true>;          // a pair's c2: state and silu in h2
using EpiMeanF = EpiForm<EPI_RES, MEAN_FIRST, false, false, false, false, false>;   // ParallelBlock mean, first ResBlock
using EpiMeanM = EpiForm<EPI_RES, MEAN_MID, false, false, false, false, false>;     // ... the middle ones
using EpiMeanLH = EpiForm<EPI_RES, MEAN_LAST, false, false, false, true, true>;     // ... last: silu(mean) in h2
using EpiMeanLF = EpiForm<EPI_RES, MEAN_LAST, false, true, false, false, true>;     // ... last: silu(mean) in fp32
using EpiPw1 = EpiForm<EPI_GELU, MEAN_NONE, false, false, true, false, false, true>;  // ConvNeXt pwconv1: h2, row ranges
using EpiPw2 = EpiForm<EPI_GAMMA_RES, MEAN_NONE, true, false, false, false, false>;   // ConvNeXt pwconv2: fp32 stream

// Launch counts of the conv_gemm_x3dw kernels by epilogue form, process-wide (epi_form_launches: the
// kernel names do not tell the forms apart, so the tests read these): [0 .. 8] the forms in the order
// above, [kEpiFormCounters - 1] EpiGeneric.
static std::atomic<long long> g_form_launches[kEpiFormCounters];
template <typename F>
constexpr int epi_form_id() {
  return std::is_same_v<F, EpiC1> ? 0 : std::is_same_v<F, EpiUp> ? 1 : std::is_same_v<F, EpiC2> ? 2
       : std::is_same_v<F, EpiMeanF> ? 3 : std::is_same_v<F, EpiMeanM> ? 4 : std::is_same_v<F, EpiMeanLH> ? 5
       : std::is_same_v<F, EpiMeanLF> ? 6 : std::is_same_v<F, EpiPw1> ? 7 : std::is_same_v<F, EpiPw2> ? 8
                                                                                                     : kEpiFormCounters - 1;
}
void epi_form_launches(long long* out, bool reset) {
  for (int i = 0; i < kEpiFormCounters; ++i) out[i] = reset ? g_form_launches[i].exchange(0) : g_form_launches[i].load();
}
// f(F{}) for the first of Fs that p is (epi_form_is), else, and under Knobs::epi_generic, f(EpiGeneric{})
template <typename... Fs, typename Fn>
static hipError_t with_epi_form(const ConvParams& p, bool generic, Fn&& f) {
  hipError_t e = hipSuccess;
  bool done = false;
  if (!generic)
    ((done = done || (epi_form_is<Fs>(p) ? (++g_form_launches[epi_form_id<Fs>()], e = f(Fs{}), true) : false)), ...);
  if (!done) ++g_form_launches[kEpiFormCounters - 1];
  return done ? e : f(EpiGeneric{});
}
// A grouped launch runs one form: the members' (the host groups a stage's c1 convs, or its c2 convs,
// which differ in weights and buffers only); members of different forms run EpiGeneric.
static bool group_generic(const ConvGroup& g) {
  if (knobs(g.p[0]).epi_generic) return true;
  for (int k = 1; k < kMaxGroup; ++k)
    if (g.start[k + 1] > g.start[k] && !(epi_form_is<EpiC1>(g.p[k]) == epi_form_is<EpiC1>(g.p[0]) &&
                                         epi_form_is<EpiC2>(g.p[k]) == epi_form_is<EpiC2>(g.p[0])))
      return true;
  return false;
}

// Ragged batches: a tile wholly beyond its clip's length writes its zeros and the caller leaves
// (workgroup-uniform; nothing has been issued and no barrier met yet, and of the tile's geometry
// only its origin is computed before the test).
template <int BM, int BN>
__device__ __forceinline__ bool ragged_tile_done(const ConvParams& p, const ConvParams& pr, int wg, int b, int ph) {
  int q0, co0;
  tile_origin<BM, BN>(p, wg, q0, co0);
  if (!tile_dead(p, pr, b, q0)) return false;
  epilogue_dead<BM, BN, 512>(p, pr, q0, co0, b, ph);
  return true;
}

// HALO = 64: convs with a tap halo (taps >= 3), input chunks double-buffered by chunk parity;
// HALO = 0 (conv_gemm_x3dm): one-tap convs, every step opens a chunk, so the input tiles ride the
// weight ring's 3 slots, over a descriptor of the tile's rows only (32-bit offsets at any length).
// RAG: the ragged-batch instantiation (ConvParams::clip_len honoured; tap convs only)
template <int BN, int HALO, bool RAG = false>
__device__ __forceinline__ void x3dq_tile(const ConvParams& p, const ConvParams& pr, const int wg, const int b, const int ph) {
  constexpr int BM = 32768 / BN, WN = BN / 64, WM = 8 / WN;
  constexpr int NA = HALO ? 2 : 3;
  constexpr int WR = BM / WM, WC = BN / WN, TM = WR / 16, TN = WC / 16;
  constexpr int AR = BM + HALO;                 // rows of an input image
  constexpr int A_G = AR / 16, B_G = BN / 16;   // 1 KiB DMA instructions per group (A per chunk, B per step)
  constexpr int A_PW = A_G / 4, B_PW = B_G / 4;
  constexpr int ABUF = AR * 128, BBUF = BN * 128;  // bytes
  constexpr int LDS_B = NA * ABUF + 3 * BBUF;
  static_assert(WR == 64 && WC == 64 && A_G % 4 == 0 && B_G % 4 == 0 && AR % 64 == 0, "tile shape");
  static_assert(LDS_B <= 160 * 1024, "LDS");
  __shared__ __attribute__((aligned(16))) unsigned short lds[LDS_B / 2];

  if constexpr (RAG)
    if (ragged_tile_done<BM, BN>(p, pr, wg, b, ph)) return;
  const TileGeo g = tile_geo<BM, BN, WN>(p, wg, ph, p.Cin / 32);
  const int lane = g.lane, group = g.group, gw = g.gw, wm = g.wm, wn = g.wn, q0 = g.q0, co0 = g.co0;
  const int nchunks = g.nchunks, taps = g.taps, nsteps = g.nsteps, lo_rel = g.lo_rel, row0 = g.row0;
  const int arow = p.ldx * 4;  // bytes per h2 row
  const __amdgpu_buffer_rsrc_t rx = x_desc<4, HALO>(p, b, row0, BM);
  const int rbase = HALO ? row0 : 0;  // row of image row 0 relative to the descriptor
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(p.w3 + w3_step(taps, p.Cin, p.Cout, ph, 0, 0)), 0, taps * nchunks * p.Cout * 128, 0x00020000);

  // DMA: group instruction k fills 64 rows of piece (k * 64) / rows; the wave's i-th is k = i * 4 + gw.
  // Source of piece pc in an h2 row's chunk: channel group pc & 3 at 32 B, plane pc >> 2 at 16 B;
  // of the weights: dcx_w3_layout.h (the wide flavour, each 64-column block in image order).
  int a_off[A_PW], b_off[B_PW];
#pragma unroll
  for (int i = 0; i < A_PW; ++i) {
    const int u = (group * A_G + i * 4 + gw) * 64;
    const int pc = u / AR, row = u - pc * AR + lane;
    a_off[i] = (rbase + row) * arow + (pc & 3) * 32 + (pc >> 2) * 16;  // negative rows: out of range
  }
#pragma unroll
  for (int i = 0; i < B_PW; ++i) {
    b_off[i] = w3_wide_lane(co0, lane) + w3_wide_piece(BN, group * B_G + i * 4 + gw);  // 1 KiB contiguous
  }
  unsigned short* const a_dst = lds + (group * A_G + gw) * 512;
  unsigned short* const b_dst = lds + NA * ABUF / 2 + (group * B_G + gw) * 512;
  [[maybe_unused]] bool in_loop = false;  // -DDCX_X3_NODMA (diagnostic): no DMA after the prologue (wrong results)
  auto dma_step = [&](int c, int m, int slot) {
#ifdef DCX_X3_NODMA
    if (in_loop) return 0;
#endif
    int n = B_PW;
    if (m == 0) {
#pragma unroll
      for (int i = 0; i < A_PW; ++i)
        dma16(rx, a_dst + (HALO ? (c & 1) : slot) * (ABUF / 2) + i * 2048, a_off[i] + c * 128, 0);
      n += A_PW;
    }
    const int soff = w3_step_bytes(nchunks, p.Cout, m, c);
#pragma unroll
    for (int i = 0; i < B_PW; ++i) dma16(rw, b_dst + slot * (BBUF / 2) + i * 2048, b_off[i], soff);
    return n;
  };

  const int l15 = lane & 15, kg = lane >> 4;
  // piece offsets (bytes): h and l of the lane's channel group
  const int pah = kg * AR * 16, pal = (4 + kg) * AR * 16;
  const int pbh = kg * BN * 16, pbl = (4 + kg) * BN * 16;
  const char* const ldsb = reinterpret_cast<const char*>(lds);
  const int bcol = NA * ABUF + (wn * WC + l15) * 16;
  s16x8 aq[TM][2], bq[TN][2];  // [h, l]
  auto readF = [&](int c, int m, int slot) {
    const char* a = ldsb + (HALO ? (c & 1) : slot) * ABUF + (wm * WR + m * p.in_step - lo_rel + l15) * 16;
    const char* bb = ldsb + bcol + slot * BBUF;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      bq[j][0] = *reinterpret_cast<const s16x8*>(bb + j * 256 + pbh);
      bq[j][1] = *reinterpret_cast<const s16x8*>(bb + j * 256 + pbl);
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      aq[i][0] = *reinterpret_cast<const s16x8*>(a + i * 256 + pah);
      aq[i][1] = *reinterpret_cast<const s16x8*>(a + i * 256 + pal);
    }
  };
  f32x4 acc[TM][TN];
  zero_acc(acc);
  // the cross terms first (hl', lh'), then hh'; 16 independent accumulators between dependent MFMAs
  // (priority 1 while issuing MFMAs: without it the C2 step took 212.0 against 192.8 ms, r05k)
  auto mfma = [&]() {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int sa = k == 1 ? 1 : 0, sb = k == 0 ? 1 : 0;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, aq[i][sa]),
                                                             __builtin_bit_cast(f16x8, bq[j][sb]), acc[i][j], 0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);
  };

  const StepPos l3 = pingpong3_prologue(nsteps, taps, dma_step);
  // the epilogue's range values and the input's unscale, in flight with the prologue's DMA
  const EpiPre epre = epi_range_pre<HALO == 0 ? 3 : 0>(p, pr, b);
  const float unscale = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int,
      __builtin_ldexpf(1.0f, -(p.w3_shift + (pr.x_ash ? pr.x_ash[b] : pr.x_ash_c))))));
  pingpong3_drain();
  in_loop = true;
  // DMA first in the memory segments (see pingpong3_loop)
  pingpong3_loop<true>(group, nsteps, taps, l3, dma_step, readF, mfma);
  // undo the weight and the input's range scaling (powers of two: exact)
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] *= unscale;
  epilogue_lds<BM, BN, WM, WN, LDS_B / 4, 512, HALO == 0 ? 3 : 0, RAG>(p, pr, acc, q0, co0, b, ph, reinterpret_cast<float*>(lds), &epre);
}

template <int BN, int HALO, bool RAG = false>
__global__ void __launch_bounds__(512, 2) conv_gemm_x3dq(const ConvParams p) {
  int wg, b, ph;
  flat_tile(((p.Lq + 32768 / BN - 1) / (32768 / BN)) * (p.Cout / BN), p.batch, wg, b, ph);
  x3dq_tile<BN, HALO, RAG>(p, p, wg, b, ph);
}

// grouped launch of up to 3 h3 convs (members as group_member deals them)
template <int BN, bool RAG = false>
__global__ void __launch_bounds__(512, 2) conv_gemm_x3dq_group(const ConvGroup g) {
  ConvParams p;
  int local, b;
  const ConvParams& pr = group_member(g, p, local, b);
  x3dq_tile<BN, 64, RAG>(p, pr, local, b, 0);
}

// ---------------------------------------------------------------------------------------------
// conv_gemm_x3dw: h3 arithmetic on 256 x 256 tiles (64 x 128 wave tiles, 96 MFMAs per segment).
//
// Segment stamps of x3dq / x3dm (tools/seg_diag_h3.py) put their memory segment, and within it the
// DMA issue, at or above the MFMA segment: a CU takes in about 16 B per cycle by LDS-DMA, and a
// 256 x 128 tile needs (A / taps + B) bytes per 48 MFMAs per wave.  A 256 x 256 tile moves the same
// A and twice the columns per step, and a 64 x 128 wave tile issues twice the MFMAs per fragment
// read.  It fits the LDS with a 2-slot step ring (B 32 KiB per slot; A 40 KiB per chunk, double-
// buffered by chunk parity, or, one-tap, 32 KiB riding the B slot): 144 / 128 KiB.
// Schedule (segment 2s = MFMA0(s) | MEM1(s), 2s + 1 = MEM0(s) | MFMA1(s); step t in slot t % 2):
//   * group 1 reads step s in MEM1(s); group 0 reads step s + 1 in MEM0(s);
//   * group 0 alone issues the DMA: step s + 2 in MEM0(s) (step s's slot, whose last reader was
//     MEM1(s)), and waits for it (vmcnt(0)) at the end of MFMA0(s + 1), before the barrier that
//     opens MEM0(s + 1), its first reader: one segment of MFMAs covers the DMA latency.
//   * A chunk c (halo) is issued with step c * taps into buffer c & 1, whose last reader (chunk
//     c - 2's last step, MEM1((c - 1) * taps - 1)) is at least two segments earlier for taps >= 2.
// Per-lane DMA offsets are one VGPR per operand (row base) plus a wave-uniform add per piece.
// ---------------------------------------------------------------------------------------------
// SPLIT (Knobs::h3_split): the weight pieces of step s + 2 are issued half by group 0 in MEM0(s)
// and half by group 1 in MEM1(s) (one tap: group 0 the input pieces, group 1 all weight pieces), so
// the CU fetches during both segments.  Group 1 may overwrite step s's slot only once all four of its
// waves have read their step-s fragments: each wave, once its reads have returned, bumps an LDS
// counter, and waits for it to reach 4 (s + 2) before issuing: group 0's waves bump it once too,
// after their step-0 reads (made before the loop, in segment 0, the segment in which group 1 refills
// step 0's slot with step 2 -- without them in the count that refill raced those reads and the last
// clip's output differed between runs, tools/determinism_check.py).  Group 1 retires its pieces at
// the end of MEM1(s + 1), before the barrier that opens MEM0(s + 1), their first reader.
// BN = 256: 256 x 256 tiles of 64 x 128 wave tiles (Cout % 256 == 0); BN = 128: 384 x 128 tiles of
// 48 x 128 wave tiles (the C = 128 stage: 72 MFMAs per segment against x3dq's 48).
template <int HALO, bool SPLIT, int BN = 256, bool RAG = false, bool GROUPED = false, typename F = EpiGeneric>
__device__ __forceinline__ void x3dw_tile(const ConvParams& p, const ConvParams& pr, const int wg, const int b, const int ph) {
  constexpr int BM = BN == 256 ? 256 : 384, WN = BN / 128, WM = 8 / WN;
  constexpr int WR = BM / WM, WC = 128, TM = WR / 16, TN = WC / 16;
  constexpr int AR = BM + HALO;                 // rows of an input image
  constexpr int A_N = AR / 8, B_N = BN / 8;     // 1 KiB DMA instructions per A chunk / B step
  constexpr int A_PW = A_N / 4;                 // A pieces per group-0 wave
  constexpr int ABUF = AR * 128, BBUF = BN * 128;  // bytes
  constexpr int NA = 2;                         // A buffers (halo: chunk parity; one tap: step slot)
  constexpr int LDS_B = NA * ABUF + 2 * BBUF;
  static_assert(A_N % 4 == 0 && B_N % 4 == 0 && AR % 64 == 0, "tile shape");
  static_assert(LDS_B + 16 <= 160 * 1024, "LDS");
  __shared__ __attribute__((aligned(16))) unsigned short lds[LDS_B / 2 + 8];  // + group 1's read counter
  unsigned int* const rd_cnt = reinterpret_cast<unsigned int*>(lds + LDS_B / 2);
  DCX_TILET(tile_t0);

  // (its own geometry preamble, not tile_geo: with the shared one the epilogues of the 256 x 256 forms
  // spilled 4-8 bytes more, the ragged or the padded ones depending on where the dead-tile test stood)
  const int tid = threadIdx.x, lane = tid & 63;
  [[maybe_unused]] const int wave = tid >> 6;
  const int group = __builtin_amdgcn_readfirstlane(tid >> 8);
  const int gw = __builtin_amdgcn_readfirstlane((tid >> 6) & 3);
  const int wm = wave / WN, wn = wave % WN;
  const int ntiles = p.Cout / BN;
  const int mt = wg / ntiles, nt = wg - mt * ntiles;
  const int q0 = mt * BM, co0 = nt * BN;
  // ragged batches: a tile wholly beyond its clip's length writes its zeros and leaves (workgroup-
  // uniform; nothing has been issued and no barrier met yet)
  if (RAG && tile_dead(p, pr, b, q0)) {
    epilogue_dead<BM, BN, 512>(p, pr, q0, co0, b, ph);
    return;
  }
  const int nchunks = p.Cin / 32;
  const int taps = p.taps;
  const int nsteps = nchunks * taps;
  const int lo_rel = p.in_step < 0 ? (taps - 1) * p.in_step : 0;
  const int row0 = q0 + p.in_base[ph] + lo_rel;
  const int arow = p.ldx * 4;  // bytes per h2 row
  const __amdgpu_buffer_rsrc_t rx = x_desc<4, HALO>(p, b, row0, BM);
  const int rbase = HALO ? row0 : 0;  // row of image row 0 relative to the descriptor
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(p.w3 + w3_step(taps, p.Cin, p.Cout, ph, 0, 0)), 0, taps * nchunks * p.Cout * 128, 0x00020000);

  // The A image: rows of 128 B with XOR-permuted pieces, fetched 8 rows per instruction
  // (dcx_a3_layout.h).  One instantiation keeps x3dq's piece-major image, [piece 8][AR][16 B], 64 rows
  // of one piece per instruction: conv_gemm_x3dw's unsplit, unragged halo form at BN = 256 (launched
  // under DCX_H3_SPLIT=0 only), whose epilogue spills 8 bytes more with the row image's DMA offsets
  // in place (12 -> 20, profiles/a3_image_resources.md), whatever their spelling.  The grouped kernel
  // calls this function with the same HALO / SPLIT / BN / RAG and takes the row image (GROUPED).
  constexpr bool ROWS = !(HALO && !SPLIT && BN == 256 && !RAG && !GROUPED);
  // DMA (group 0 alone): A instruction k fills image rows [8 k, 8 k + 8) with their chunks, 128 B per 8
  // lanes; B instruction k fills 64 columns of piece (k * 64) / BN; the wave's i-th is k = i * 4 + gw.
  // Lane part of the source offset in one VGPR, the rest wave-uniform; both go into the vector offset
  // (the scalar one stays 0): a negative row's lane part must wrap together with the uniform part
  // before the descriptor's range check, or the row would not read zeros.  (Group 1
  // issuing half of the weight pieces from inside its MFMA segment, so that the DMA of a step is in
  // flight in both segments, measured slower: C2 194.2-194.7 against 185.3-185.4 ms, r05n; the
  // issue stalls behind group 0's and holds up the MFMAs.)
  const int a_lane = ROWS ? a3_src_lane(rbase, arow, lane) : (rbase + lane) * arow;  // negative rows: huge unsigned, out of range (zeros)
  const int b_lane = w3_wide_lane(co0, lane);  // dcx_w3_layout.h: every weight piece is 1 KiB contiguous
  [[maybe_unused]] bool in_loop = false;  // -DDCX_X3_NODMA (diagnostic): no DMA after the prologue (wrong results)
  auto dmaA1 = [&](int c, int slot, int i) {  // the wave's i-th A piece of chunk c
#ifdef DCX_X3_NODMA
    if (in_loop) return;
#endif
    const int k = i * 4 + gw;
    const int abuf = HALO ? (c & 1) : slot;
    if constexpr (ROWS) {
      dma16(rx, lds + abuf * (ABUF / 2) + k * 512, a_lane + a3_src_inst(arow, k, c), 0);
    } else {
      const int u = k * 64, pc = u / AR, row = u - pc * AR;
      dma16(rx, lds + abuf * (ABUF / 2) + k * 512, a_lane + row * arow + (pc & 3) * 32 + (pc >> 2) * 16 + c * 128, 0);
    }
  };
  // B instructions [0, B_G0) are group 0's, [B_G0, B_N) group 1's (SPLIT)
#ifndef DCX_X3W_BG0_DIV  // A/B builds: group 0's share of the weight pieces, 1 / DIV (halo convs)
#define DCX_X3W_BG0_DIV 2
#endif
  constexpr int B_G0 = !SPLIT ? B_N : HALO ? B_N / DCX_X3W_BG0_DIV : 0;
  constexpr int B_W0 = B_G0 / 4, B_W1 = (B_N - B_G0) / 4;  // B pieces per wave of group 0 / 1
  auto dmaB1 = [&](int c, int m, int slot, int i) {  // the wave's i-th B piece of step (c, m)
#ifdef DCX_X3_NODMA
    if (in_loop) return;
#endif
    const int k = (group ? B_G0 : 0) + i * 4 + gw;
    dma16(rw, lds + NA * ABUF / 2 + slot * (BBUF / 2) + k * 512, b_lane, w3_step_bytes(nchunks, p.Cout, m, c) + w3_wide_piece(BN, k));
  };
  auto dma_step = [&](int c, int m, int slot) {  // group 0's pieces of a step (its input chunk first)
    if (m == 0) {
#pragma unroll
      for (int i = 0; i < A_PW; ++i) dmaA1(c, slot, i);
    }
#pragma unroll
    for (int i = 0; i < B_W0; ++i) dmaB1(c, m, slot, i);
  };
  auto dma_step1 = [&](int c, int m, int slot) {  // group 1's (SPLIT)
#pragma unroll
    for (int i = 0; i < B_W1; ++i) dmaB1(c, m, slot, i);
  };

  // fragment addresses: one lane base per operand (h piece of the lane's channel group kg); the
  // l piece of B, row / column blocks and the B slot are immediate offsets.  The A image
  // (dcx_a3_layout.h) is not linear in the row, so a tap conv's base is recomputed per step from the
  // lane's row; its l piece is the h address ^ 64.
  const int l15 = lane & 15, kg = lane >> 4;
  const char* const ldsb = reinterpret_cast<const char*>(lds);
  const int a_row = wm * WR + l15;  // image row of the lane's first fragment at tap offset 0
  static_assert(WR % kA3BlockRows == 0 && a3_image(16, 0) == 2048, "row blocks as immediates");
  const char* const b_rd = ldsb + NA * ABUF + kg * BN * 16 + (wn * WC + l15) * 16;
  s16x8 aq[TM][2], bq[TN][2];  // [h, l]
  auto readF = [&](int c, int m, int slot) {
    const int a_r = a_row + (HALO ? m * p.in_step - lo_rel : 0);
    const int ah = (HALO ? (c & 1) : slot) * ABUF + (ROWS ? a3_image(a_r, kg) : kg * AR * 16 + a_r * 16);
    const char* a = ldsb + ah;
    const char* al = ldsb + (ROWS ? ah ^ kA3PlaneXor : ah + 4 * AR * 16);
    const char* bb = b_rd + slot * BBUF;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      bq[j][0] = *reinterpret_cast<const s16x8*>(bb + j * 256);
      bq[j][1] = *reinterpret_cast<const s16x8*>(bb + j * 256 + 4 * BN * 16);
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      aq[i][0] = *reinterpret_cast<const s16x8*>(a + i * (ROWS ? 2048 : 256));
      aq[i][1] = *reinterpret_cast<const s16x8*>(al + i * (ROWS ? 2048 : 256));
    }
  };
  f32x4 acc[TM][TN];
  zero_acc(acc);
  auto mfma = [&]() {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int sa = k == 1 ? 1 : 0, sb = k == 0 ? 1 : 0;
#pragma unroll
      for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, aq[i][sa]),
                                                             __builtin_bit_cast(f16x8, bq[j][sb]), acc[i][j], 0, 0, 0);
      }
    }
    __builtin_amdgcn_s_setprio(0);
  };

  // prologue: steps 0 and 1, drained
  int cl = 0, ml = 0;  // the next step this group issues
  if (SPLIT && tid == 0) *rd_cnt = 0u;
  for (int t = 0; t < 2 && t < nsteps; ++t) {
    if (group == 0) dma_step(cl, ml, t);
    else if (SPLIT) dma_step1(cl, ml, t);
    step_adv(cl, ml, taps);
  }
  // the epilogue's range values and the input's unscale, in flight with the prologue's DMA
  const EpiPre epre = epi_range_pre<HALO == 0 ? 3 : 0>(p, pr, b);
  const float unscale = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int,
      __builtin_ldexpf(1.0f, -(p.w3_shift + (pr.x_ash ? pr.x_ash[b] : pr.x_ash_c))))));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  seg_barrier();
  DCX_TILET(tile_t1);
  in_loop = true;
#ifdef DCX_SEG_DIAG
  unsigned long long sd[6] = {};
#endif
  int cr = 0, mr = 0;
  if (group == 0) {
    readF(0, 0, 0);
    if (SPLIT) {  // step 0's slot is refilled by group 1 in segment 0: count these reads too
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (lane == 0) __hip_atomic_fetch_add(rd_cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    step_adv(cr, mr, taps);
    for (int s = 0; s < nsteps; ++s) {
      DCX_SEGT(ta);
      mfma();  // MFMA(s)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // step s + 1 (issued in MEM0(s - 1)) landed
      DCX_SEGT(tb);
      seg_barrier();
      DCX_SEGT(tc);
      // MEM0(s): issue step s + 2 into step s's slot, fragments of step s + 1 (reads first: same
      // times, r05q)
      if (s + 2 < nsteps) {
        dma_step(cl, ml, s & 1);
        step_adv(cl, ml, taps);
      }
      DCX_SEGT(tr);
      if (s + 1 < nsteps) readF(cr, mr, (s + 1) & 1);
      DCX_SEGT(tq);
      DCX_SEGT(td);
      seg_barrier();
      DCX_SEGT(te);
#ifdef DCX_SEG_DIAG
      sd[0] += tb - ta; sd[1] += tc - tb; sd[2] += td - tc; sd[3] += te - td; sd[4] += tr - tc; sd[5] += tq - tr;
#endif
      step_adv(cr, mr, taps);
    }
  } else {
    for (int s = 0; s < nsteps; ++s) {
      DCX_SEGT(ta);
      readF(cr, mr, s & 1);  // MEM1(s): fragments of step s
      if (SPLIT) {
        int n = 0;
        if (s + 2 < nsteps) {  // this group's pieces of step s + 2, into step s's slot once read
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          if (lane == 0) __hip_atomic_fetch_add(rd_cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          const unsigned int want = 4u * (unsigned)(s + 2);  // + group 0's four step-0 reads
          while (__hip_atomic_load(rd_cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < want) {
          }
          dma_step1(cl, ml, s & 1);
          step_adv(cl, ml, taps);
          n = B_W1;
        }
        wait_dma(n);  // step s + 1's pieces (issued in MEM1(s - 1)) landed
      }
      DCX_SEGT(tb);
      seg_barrier();
      DCX_SEGT(tc);
      mfma();  // MFMA(s)
      DCX_SEGT(td);
      seg_barrier();
      DCX_SEGT(te);
#ifdef DCX_SEG_DIAG
      sd[2] += tb - ta; sd[3] += tc - tb; sd[0] += td - tc; sd[1] += te - td; sd[5] += tb - ta;
#endif
      step_adv(cr, mr, taps);
    }
  }
#ifdef DCX_SEG_DIAG
  if ((threadIdx.x & 255) == 0) {
#pragma unroll
    for (int i = 0; i < 6; ++i) atomicAdd(&g_seg_diag[group * 6 + i], sd[i]);
    if (group == 0) atomicAdd(&g_seg_diag[12], (unsigned long long)nsteps);
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 6; ++i) atomicAdd(&g_seg_diag8[wave * 6 + i], sd[i]);
    if (wave == 0) atomicAdd(&g_seg_diag8[48], (unsigned long long)nsteps);
  }
#endif
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  DCX_TILET(tile_t2);
  // undo the weight and the input's range scaling (powers of two: exact)
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] *= unscale;
  epilogue_lds<BM, BN, WM, WN, LDS_B / 4, 512, HALO == 0 ? 3 : 0, RAG, F>(p, pr, acc, q0, co0, b, ph, reinterpret_cast<float*>(lds), &epre);
  DCX_TILE_END(nsteps);
}

template <int HALO, bool SPLIT, int BN = 256, bool RAG = false, typename F = EpiGeneric>
__global__ void __launch_bounds__(512, 2) conv_gemm_x3dw(const ConvParams p) {
  constexpr int BM = BN == 256 ? 256 : 384;
  int wg, b, ph;
  flat_tile(((p.Lq + BM - 1) / BM) * (p.Cout / BN), p.batch, wg, b, ph);
  x3dw_tile<HALO, SPLIT, BN, RAG, false, F>(p, p, wg, b, ph);
}

template <bool SPLIT, int BN = 256, bool RAG = false, typename F = EpiGeneric>
__global__ void __launch_bounds__(512, 2) conv_gemm_x3dw_group(const ConvGroup g) {
  ConvParams p;
  int local, b;
  const ConvParams& pr = group_member(g, p, local, b);
  x3dw_tile<64, SPLIT, BN, RAG, true, F>(p, pr, local, b, 0);
}

// Whether conv_gemm_x3dq<bn> (taps >= 3 with a halo) or conv_gemm_x3dm<bn> (one tap) takes an h3
// conv (input in LAYOUT_H2).
// wide (conv_gemm_x3dw): taps >= 2 (its input buffer is free two segments before it is refilled)
bool x3dq_ok(const ConvParams& p, int bn, bool wide) {
  const int span = (p.taps - 1) * (p.in_step < 0 ? -p.in_step : p.in_step);
  if (!p.x6 || !p.w3 || p.x_layout != LAYOUT_H2 || p.Cin % 32 || p.Cout % bn || p.ksplit > 1) return false;
  const long long arow = (long long)p.ldx * 4;
  if ((long long)p.taps * p.Cin * p.Cout * 4 >= (1LL << 31)) return false;
  if (p.taps == 1) {  // per-tile descriptor: every phase's rows start at or after the tile's
    for (int i = 0; i < kMaxPhases; ++i)
      if (p.in_base[i] < 0) return false;
    return 256LL * arow < (1LL << 31);
  }
  return p.taps >= (wide ? 2 : 3) && span > 0 && span <= 64 && (long long)(p.Lin + 1024) * arow < (1LL << 31);
}
// Tiles of an h3 conv: 256 x 256 (conv_gemm_x3dw) where Cout % 256 == 0, else 256 x 128.  (256 x 128
// against 128 x 256: half the weight DMA per step, C2 205.1 -> 193.2 ms, r05i.)  Knobs::h3_bn
// (DCX_H3_BN, A/B): 128 = the 256 x 128 tiles everywhere, 256 = the 128 x 256 ones at Cout % 256 == 0.
// Returns the column tile, 512 standing for the 256 x 256 kernel.
// 384 stands for the 384 x 128 conv_gemm_x3dw (Cout % 256 != 0, taps >= 2; DCX_H3_BN=128 keeps the
// 256 x 128 conv_gemm_x3dq there where it can, taps >= 3).
int x3dq_bn(const ConvParams& p) {
  const int k = p.kn ? p.kn->h3_bn : 0;
  if (p.Cout % 256) return (k == 128 && p.taps >= 3) || p.taps < 2 ? 128 : 384;
  // (a two-tap conv, the ConvTs' phases, has no x3dq form: the knob leaves it on the 256 x 256 tiles,
  // where a whole generator call under DCX_H3_BN used to fail its launch)
  if (p.taps == 2) return 512;
  return k == 128 ? 128 : k == 256 ? 256 : 512;
}

template <int BN>
hipError_t launch_x3dq(const ConvParams& p, int batch, int phases, hipStream_t s, const char** kname) {
  constexpr int BM = 32768 / BN;
  if (p.taps == 1) {
    if (p.clip_len) return hipErrorNotSupported;  // the one-tap kernels take no per-clip lengths
    if (kname) *kname = BN == 256 ? "conv_gemm_x3dm<128,256>" : "conv_gemm_x3dm<256,128>";
    return launch_flat<BM, BN>(conv_gemm_x3dq<BN, 0>, p, batch, phases, 512, s);
  }
  // (these tiles run EpiGeneric: the tap convs come here under DCX_H3_BN only, and no conv of the
  // model is a one-tap conv with Cout % 256 != 0)
  if (kname) *kname = BN == 256 ? "conv_gemm_x3dq<128,256,halo>" : "conv_gemm_x3dq<256,128,halo>";
  if (p.clip_len) return launch_flat<BM, BN>(conv_gemm_x3dq<BN, 64, true>, p, batch, phases, 512, s);  // ragged batch
  return launch_flat<BM, BN>(conv_gemm_x3dq<BN, 64>, p, batch, phases, 512, s);
}

template hipError_t launch_x3dq<256>(const ConvParams&, int, int, hipStream_t, const char**);
template hipError_t launch_x3dq<128>(const ConvParams&, int, int, hipStream_t, const char**);

// A tap conv on conv_gemm_x3dw's BM x BN tiles, ragged or not, in its epilogue form.  The forms are
// instantiated for the shipped DMA split only (Knobs::h3_split = 0, an A/B switch, runs EpiGeneric).
template <int BM, int BN, bool RAG>
static hipError_t launch_x3dw_halo(const ConvParams& p, bool sp, int batch, int phases, hipStream_t s) {
  if (!sp) {
    ++g_form_launches[kEpiFormCounters - 1];
    return launch_flat<BM, BN>(conv_gemm_x3dw<64, false, BN, RAG>, p, batch, phases, 512, s);
  }
  return with_epi_form<EpiC1, EpiUp, EpiC2, EpiMeanF, EpiMeanM, EpiMeanLH, EpiMeanLF>(p, knobs(p).epi_generic, [&](auto f) {
    return launch_flat<BM, BN>(conv_gemm_x3dw<64, true, BN, RAG, decltype(f)>, p, batch, phases, 512, s);
  });
}

// bsel (x3dq_bn): 384 = the 384 x 128 tiles (the C = 128 stage), 512 = the 256 x 256 tiles
hipError_t launch_x3dw(const ConvParams& p, int bsel, int batch, int phases, hipStream_t s, const char** kname) {
  const bool sp = knobs(p).h3_split;
  if (p.clip_len && p.taps == 1) return hipErrorNotSupported;  // ragged batch: the length-aware instantiations (tap convs)
  if (bsel == 384) {
    if (kname) *kname = "conv_gemm_x3dw<384,128,halo>";
    return p.clip_len ? launch_x3dw_halo<384, 128, true>(p, sp, batch, phases, s)
                      : launch_x3dw_halo<384, 128, false>(p, sp, batch, phases, s);
  }
  if (p.taps == 1) {
    if (kname) *kname = "conv_gemm_x3dw<256,256>";
    if (!sp) {
      ++g_form_launches[kEpiFormCounters - 1];
      return launch_flat<256, 256>(conv_gemm_x3dw<0, false>, p, batch, phases, 512, s);
    }
    return with_epi_form<EpiPw1, EpiPw2>(p, knobs(p).epi_generic, [&](auto f) {
      return launch_flat<256, 256>(conv_gemm_x3dw<0, true, 256, false, decltype(f)>, p, batch, phases, 512, s);
    });
  }
  if (kname) *kname = "conv_gemm_x3dw<256,256,halo>";
  return p.clip_len ? launch_x3dw_halo<256, 256, true>(p, sp, batch, phases, s)
                    : launch_x3dw_halo<256, 256, false>(p, sp, batch, phases, s);
}

template <int BN, bool RAG>
static void launch_x3dw_group(const ConvGroup& g, bool split, unsigned blocks, hipStream_t s) {
  if (!split) {
    ++g_form_launches[kEpiFormCounters - 1];
    hipLaunchKernelGGL((conv_gemm_x3dw_group<false, BN, RAG>), dim3(blocks), dim3(512), 0, s, g);
    return;
  }
  (void)with_epi_form<EpiC1, EpiC2>(g.p[0], group_generic(g), [&](auto f) {  // (the caller reads hipGetLastError)
    hipLaunchKernelGGL((conv_gemm_x3dw_group<true, BN, RAG, decltype(f)>), dim3(blocks), dim3(512), 0, s, g);
    return hipSuccess;
  });
}

// bsel 384 / 512: conv_gemm_x3dw_group; 256 / 128: conv_gemm_x3dq_group<bsel>
hipError_t launch_h3_group(const ConvGroup& g, int bsel, bool split, unsigned blocks, hipStream_t s, const char** kname) {
  const bool rag = g.p[0].clip_len != nullptr;  // ragged batch (every member of a group has the lengths or none): the length-aware instantiations
  if (bsel == 384) {
    if (kname) *kname = "conv_gemm_x3dw_group<384,128,halo>";
    if (rag) launch_x3dw_group<128, true>(g, split, blocks, s);
    else launch_x3dw_group<128, false>(g, split, blocks, s);
  } else if (bsel == 512) {
    if (kname) *kname = "conv_gemm_x3dw_group<256,256,halo>";
    if (rag) launch_x3dw_group<256, true>(g, split, blocks, s);
    else launch_x3dw_group<256, false>(g, split, blocks, s);
  } else if (bsel == 256) {
    if (kname) *kname = "conv_gemm_x3dq_group<128,256,halo>";
    if (rag) hipLaunchKernelGGL((conv_gemm_x3dq_group<256, true>), dim3(blocks), dim3(512), 0, s, g);
    else hipLaunchKernelGGL((conv_gemm_x3dq_group<256>), dim3(blocks), dim3(512), 0, s, g);
  } else {
    if (kname) *kname = "conv_gemm_x3dq_group<256,128,halo>";
    if (rag) hipLaunchKernelGGL((conv_gemm_x3dq_group<128, true>), dim3(blocks), dim3(512), 0, s, g);
    else hipLaunchKernelGGL((conv_gemm_x3dq_group<128>), dim3(blocks), dim3(512), 0, s, g);
  }
  return hipGetLastError();
}

}  // namespace dcx
