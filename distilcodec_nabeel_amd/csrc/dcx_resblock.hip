// Fused ResBlock1 pairs for the small-channel generator stages (C = 32 and 64).
//
// ResBlock1 (convnext_utils.py:106-113) runs three pairs
//     xt = c2(silu(c1(silu(x))));  x = xt + x
// with c1 dilated (k, d) and c2 undilated (k, 1); ParralelBlock (:137-138) averages three such
// ResBlocks (k = 3 / 7 / 11).  At C = 32 / 64 each conv has K = k * C <= 704, so one conv per launch
// (conv_gemm_x6w4f / x6pf) spent its time staging and splitting its fp32 input and round-tripping
// silu(c1) through HBM rather than in MFMAs (0.30 / 0.47 MFMA busy, 7 SALU + 8 VALU per MFMA).
//
// conv_res_pair runs one pair of all three ResBlocks per launch.  A workgroup owns R output rows of
// one clip and, for each ResBlock in turn:
//   1. S image: silu(state) as x6 planes in LDS, rows [r0 - 8 - 32, r0 + R + 8 + 32) (zero outside
//      the clip = the conv's zero padding), prefetched into registers during the previous c2;
//   2. c1 over the R + 16 rows [r0 - 8, r0 + R + 8) (the c2 halo, (k - 1) / 2 <= 8);
//   3. T image: silu(c1 + b1) planes written over S (zero outside the clip);
//   4. c2 over the R output rows, epilogue state + c2 + b2 to the next state buffer (or, for the
//      last pair, into the ParallelBlock mean, kept in registers across the three ResBlocks in
//      ResBlock order: m = v0; m += v1; m = (m + v2) / 3, then silu(mean) to the next ConvT input).
// The halo makes in-place updates race, so each pair writes a buffer other than the one it reads.
//
// Arithmetic: the x6 products of conv_gemm_x6dq (v_mfma_f32_16x16x32_bf16, the K dimension split
// into (term, channel)), with the weights as the A operand and the activations as B, so each lane's
// accumulator holds 4 consecutive channels of one time row: T-image writes are 8-byte plane stores
// and epilogue loads / stores are 16-byte fp32 accesses.
//   W{h',m'} . X{h,m} = hh' + mm',  W{h',m'} . X{m,h} = mh' + hm',  W{h',l'} . X{l,h} = lh' + hl'.
// Weights stream through a 2-slot LDS ring, one tap (C * C * 6 bytes) per step, prefetched one
// step ahead into registers; the step sequence runs on across convs, ResBlocks and tiles.
// LDS images: piece-major and row-linear, byte ((chunk * 6 + piece) * NS + row) * 16 (piece = half * 3 +
// plane, NS the image rows, a multiple of 16): every ds_read_b128 of 16 consecutive rows of one piece
// is conflict-free at any tap offset, and a tap's row offset is one add per read set (round 5; the
// round-2 layout of 16-row blocks cost ~6 VALU per row block and tap in address arithmetic).  The
// weight slot is the global tap slice [chunk][Cout][96 B] copied as is.
// The phases every pair kernel shares (geometry, the x6 / h3 arithmetics, S / T image, MFMA block,
// weight fragments, tile loop, epilogue, stamps) are in dcx_resblock_common.h; here are the three
// schedules and the launcher.
#include <algorithm>
#include <cstdio>

#include "dcx_resblock_common.h"

namespace dcx {

// output rows per tile: 496 / 176 (C = 32 / 64) by default; the launcher takes fewer rows per tile
// when a launch has too few tiles for the CUs (small batches: the C5 streaming hop), same bits
template <int C>
constexpr int kRpRows = C == 32 ? 496 : 176;
// conv_res_pair_h3: h3 images are 4 B per element instead of 6, so taller tiles fit the LDS
template <int C>
constexpr int kRp3Rows = C == 32 ? 624 : 240;

template <int C, bool MEAN, int RR = kRpRows<C>>
__global__ void __launch_bounds__(512, 1) conv_res_pair(const ResPairParams p) {
  using A = RpX6;
  using G = RpGeom<A, C, RR>;
  constexpr int NCH = G::NCH, WR = G::WR, RB = G::RB1, PS = G::PS, IMG = G::IMG, WTAP = G::WTAP, NIT = G::NIT;
  constexpr int TPS = C == 32 ? 2 : 1;  // taps per step (weight slot)
  constexpr int WSLOT = TPS * WTAP;
  constexpr int WP = WSLOT / 1024, WPW = (WP + 7) / 8;  // DMA pieces per slot, per wave
  constexpr int LDS = IMG + 2 * WSLOT + G::BIASB;
  static_assert(WSLOT % 1024 == 0 && LDS <= 160 * 1024, "LDS");
  __shared__ __attribute__((aligned(16))) char lds[LDS];
  float* const bias_lds = reinterpret_cast<float*>(lds + IMG + 2 * WSLOT);  // [conv][member][C]

  const RpLane ln = RpLane::make<G>();
  const int tid = ln.tid, lane = ln.lane, wave = ln.wave, wr = ln.wr;
  const int L = p.L, nmem = p.nmem;

  // ---- weight ring: LDS-DMA of a step's taps (lane-linear 1 KiB pieces, no staging registers);
  // taps past the conv's last read zeros (outside the buffer descriptor) and are never used ----
  auto issue_w = [&](int m, int conv, int step, int slot) {
    const int k = p.taps[m], j0 = step * TPS;
    const unsigned short* w = (conv ? p.w2[m] : p.w1[m]) + (long long)j0 * (WTAP / 2);
    const __amdgpu_buffer_rsrc_t rw =
        __builtin_amdgcn_make_buffer_rsrc((void*)w, 0, min(TPS, k - j0) * WTAP, 0x00020000);
#pragma unroll
    for (int i = 0; i < WPW; ++i) {
      const int piece = wave + 8 * i;
      if (WP % 8 == 0 || piece < WP)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (rp_lds_t)(lds + IMG + slot * WSLOT + piece * 1024), 16,
                                                 piece * 1024 + lane * 16, 0, 0, 0);
    }
    asm volatile("" ::: "memory");  // later loads stay younger than the pieces (rp_wait counts them)
  };

  f32x4 pf[NIT][2];  // the next S image's rows in flight

  // ---- one step: the step's taps, every chunk, rows of this wave, its 2 column blocks.  hook(i)
  // runs after row block i of the first tap (global loads spread between the MFMAs) ----
  const A::Wo wo = A::wo(lane, ln.wc);
  const A::Xb xl = A::xlane<G::NS>(lds, lane);
  auto mfma_step = [&](RpRow (&acc)[RB], int slot, int ntaps, int row0, int rstep, int nrb, auto hook) {
#pragma unroll
    for (int u = 0; u < TPS; ++u) {
      if (u >= ntaps) break;
      const char* wb = lds + IMG + slot * WSLOT + u * WTAP;
      s16x8 wf[NCH][2][2];
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
          const char* w = wb + (ch * C + cb * 16) * G::WROW;
          wf[ch][cb][0] = *reinterpret_cast<const s16x8*>(w + wo.o0);  // {h', m'}
          wf[ch][cb][1] = *reinterpret_cast<const s16x8*>(w + wo.o1);  // {h', l'}
        }
      const A::Xb x = A::at(xl, (wr * 16 + row0 + u * rstep) * 16);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < RB; ++i) {
        if (i < nrb) {
#pragma unroll
          for (int ch = 0; ch < NCH; ++ch) rp_block<A>(acc[i], wf[ch], x, (WR * 16 * i) * 16 + ch * A::PPC * PS);
        }
        if (u == 0) hook(i);
      }
      __builtin_amdgcn_s_setprio(0);
    }
  };
  auto no_hook = [](int) {};

  // rows of c2 this wave owns
  const int nrb2 = min(RB, (G::NB2 - wr + WR - 1) / WR);
  RpTiles<G::R> tl;
  if (!tl.first(p)) return;  // whole workgroup, before any barrier
  // prologue: biases, first ResBlock's S image and first weight step
  rp_bias_prologue<C>(bias_lds, p, tid);
  issue_w(0, 0, 0, 0);
#pragma unroll
  for (int k = 0; k < NIT; ++k) rp_fill_issue<G, C>(pf[k], p.src[0] + (long long)tl.b * p.bstride, tl.r0, L, tid, k);
  rp_fill_commit<A, G>(lds, pf, tl.r0, L, tid);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  rp_barrier();
  int slot = 0;
  RpRow macc[MEAN ? RB : 1];
  RP_STAMP(RpStamps st;)
  for (;;) {
    tl.look_ahead();
    const int r0 = tl.r0;
    for (int m = 0; m < nmem; ++m) {
      const int k = p.taps[m], hk = (k - 1) >> 1, d = p.dil[m];
      const int nst = (k + TPS - 1) / TPS;  // steps per conv
      const long long cb0 = (long long)tl.b * p.bstride;
      const bool last_m = m + 1 == nmem;
      const bool has_next = !last_m || tl.more;
      RpRow acc[RB];
      RP_T(ta);
      // ---- c1 over rows [r0 - 8, r0 + R + 8) from the S image
#pragma unroll
      for (int i = 0; i < RB; ++i) acc[i].zero();
      for (int j = 0; j < nst; ++j) {
        if (j + 1 < nst) issue_w(m, 0, j + 1, slot ^ 1);
        else issue_w(m, 1, 0, slot ^ 1);
        RP_T(s1);
        mfma_step(acc, slot, min(TPS, k - j * TPS), G::H1 + (j * TPS - hk) * d, d, RB, no_hook);
        RP_T(s2);
        rp_wait(0);
        rp_barrier();
        RP_STAMP({
          RP_T(s3);
          st.dg[8] += s2 - s1;
          st.dg[9] += s3 - s2;
        })
        slot ^= 1;
      }
      RP_T(tb);
      // ---- T image: silu(c1 + b1) planes over the S image (zero outside the clip)
      rp_t_image<A, G, C>(lds, bias_lds + m * C, acc, ln, r0, L);
      rp_barrier();
      RP_T(tc);
      // ---- c2 over rows [r0, r0 + R) from the T image.  Step 0 loads the residual rows, step 1 (or
      // 0) the next S image's rows (this tile's next ResBlock, or the next tile's first), one row
      // block's share between the MFMAs of each, after the step's weight pieces.  The two steps are
      // peeled out of the loop: a load pending across the loop's back edge made hipcc wait for it.
#pragma unroll
      for (int i = 0; i < RB; ++i) acc[i].zero();
      const float* nsrc = !last_m ? p.src[m + 1] + cb0 : p.src[0] + (long long)tl.nb * p.bstride;
      const int nsr0 = !last_m ? r0 : tl.nr0;
      const int jpf = nst > 1 ? 1 : 0;
      RpRow res[RB];
      auto res_hook = [&](int i) { rp_load_res<G, C>(res[i], p.src[m] + cb0, ln, r0, L, i); };
      auto pf_hook = [&](int i) {
        if (!has_next) return;
#pragma unroll
        for (int kk = NIT * i / RB; kk < NIT * (i + 1) / RB; ++kk) rp_fill_issue<G, C>(pf[kk], nsrc, nsr0, L, tid, kk);
      };
      auto both_hook = [&](int i) {
        res_hook(i);
        pf_hook(i);
      };
      auto c2_issue_w = [&](int j) {
        if (j + 1 < nst) issue_w(m, 1, j + 1, slot ^ 1);
        else if (has_next) issue_w(last_m ? 0 : m + 1, 0, 0, slot ^ 1);
      };
      const int npf = has_next ? 2 * NIT : 0;
      c2_issue_w(0);
      if (jpf == 0) {
        mfma_step(acc, slot, min(TPS, k), 8 - hk, 1, nrb2, both_hook);
        rp_wait(2 * RB + npf);
      } else {
        mfma_step(acc, slot, TPS, 8 - hk, 1, nrb2, res_hook);
        rp_wait(2 * RB);
        rp_barrier();
        slot ^= 1;
        c2_issue_w(1);
        mfma_step(acc, slot, min(TPS, k - TPS), 8 + TPS - hk, 1, nrb2, pf_hook);
        rp_wait(npf);
      }
      rp_barrier();
      slot ^= 1;
      for (int j = jpf + 1; j < nst; ++j) {
        c2_issue_w(j);
        mfma_step(acc, slot, min(TPS, k - j * TPS), 8 + j * TPS - hk, 1, nrb2, no_hook);
        rp_wait(0);
        rp_barrier();
        slot ^= 1;
      }
      RP_T(te);
      // ---- epilogue: state + c2 + b2 (rows past the clip end are dropped)
      rp_epilogue<A, G, C, MEAN>(p, bias_lds + (kMaxGroup + m) * C, acc, res, macc, ln, m, cb0, r0, nrb2);
      RP_T(tf);
      if (has_next) {
        rp_fill_commit<A, G>(lds, pf, nsr0, L, tid);
        rp_barrier();
      }
      RP_STAMP({
        RP_T(tg);
        st.member(ta, tb, tc, te, tf, tg, nst);
      })
    }
    if (!tl.more) break;
    tl.advance();
  }
  RP_STAMP(st.flush(C, tid);)
}

// Barrier-free tap loops (round 3): conv_res_pair_g.  conv_res_pair's per-step stamps put a c1 tap
// step at 3690 cycles against 2304 of MFMA issue per SIMD (C = 64).  A timing build that never
// refilled the weight ring was no faster, and a 4-slot ring of half-tap units with the next unit's
// fragments prefetched into registers took 2278 cycles per 1152-cycle unit: every barrier of the
// ring costs ~1100 cycles (the 8 waves restart together behind one LDS queue, and the slowest wave
// sets the end), however short the step.  Here each wave loads its weight fragments from global
// memory (L2; the four waves of a column half read the same bytes, so most hit L1) into registers,
// chunk by chunk, one tap ahead: after the MFMAs of chunk ch of tap j, the registers take chunk ch
// of the next tap in the stream (next conv, member or tile).  The tap loops need no barrier; only the
// image hand-offs do (S -> T after c1, T -> the next S after c2).  Arithmetic, summation order and
// layouts are conv_res_pair's, so the results are the same bits.
template <int C, bool MEAN, int RR = kRpRows<C>>
__global__ void __launch_bounds__(512, 1) conv_res_pair_g(const ResPairParams p) {
  using A = RpX6;
  using G = RpGeom<A, C, RR>;
  constexpr int NCH = G::NCH, WR = G::WR, RB = G::RB1, PS = G::PS, IMG = G::IMG, NIT = G::NIT;
  __shared__ __attribute__((aligned(16))) char lds[IMG + G::BIASB];
  float* const bias_lds = reinterpret_cast<float*>(lds + IMG);  // [conv][member][C]

  const RpLane ln = RpLane::make<G>();
  const int tid = ln.tid, lane = ln.lane, wr = ln.wr;
  const int L = p.L, nmem = p.nmem;

  f32x4 pf[NIT][2];      // the next S image's rows in flight
  s16x8 wf[NCH][2][2];  // the weight fragments of a tap, [chunk][column block][{h',m'} | {h',l'}]
  const A::Wo wo = A::wo(lane, ln.wc);
  const A::Xb xl = A::xlane<G::NS>(lds, lane);

  // ---- one tap, chunk-major: the MFMAs of chunk ch for every row block of the wave, then chunk ch
  // of the next tap into the fragment registers; hook() once every reload of the tap is issued (its
  // loads are then younger than the fragments the next tap waits for) ----
  auto tap = [&](RpRow (&acc)[RB], int rowoff, int nrb, const unsigned short* wnext, auto hook) {
    const A::Xb x = A::at(xl, (wr * 16 + rowoff) * 16);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
      for (int i = 0; i < RB; ++i) {
        if (i < nrb) rp_block<A>(acc[i], wf[ch], x, (WR * 16 * i) * 16 + ch * A::PPC * PS);
      }
      rp_load_wf<A, G, C>(wf[ch], wnext, ch, wo);
      // keep the reloads here: left to itself the scheduler sinks all of them to the end of the tap,
      // and the next tap's first MFMAs then wait a whole L2 round trip
      __builtin_amdgcn_sched_barrier(0);
    }
    __builtin_amdgcn_s_setprio(0);
    hook();
  };
  auto no_hook = [] {};

  const int nrb2 = min(RB, (G::NB2 - wr + WR - 1) / WR);
  RpTiles<G::R> tl;
  if (!tl.first(p)) return;  // whole workgroup, before any barrier
  rp_bias_prologue<C>(bias_lds, p, tid);
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) rp_load_wf<A, G, C>(wf[ch], p.w1[0], ch, wo);
#pragma unroll
  for (int k = 0; k < NIT; ++k) rp_fill_issue<G, C>(pf[k], p.src[0] + (long long)tl.b * p.bstride, tl.r0, L, tid, k);
  rp_fill_commit<A, G>(lds, pf, tl.r0, L, tid);
  rp_barrier();
  RpRow macc[MEAN ? RB : 1];
  RP_STAMP(RpStamps st;)
  for (;;) {
    tl.look_ahead();
    const int r0 = tl.r0;
    for (int m = 0; m < nmem; ++m) {
      const int k = p.taps[m], hk = (k - 1) >> 1, d = p.dil[m];
      const long long cb0 = (long long)tl.b * p.bstride;
      const bool last_m = m + 1 == nmem;
      const bool has_next = !last_m || tl.more;
      RpRow acc[RB];
      RP_T(ta);
      // ---- c1 over rows [r0 - 8, r0 + R + 8) from the S image
#pragma unroll
      for (int i = 0; i < RB; ++i) acc[i].zero();
      for (int j = 0; j < k; ++j) tap(acc, G::H1 + (j - hk) * d, RB, rp_next_tap<G>(p, m, 0, j), no_hook);
      RP_T(tb);
      rp_barrier();  // every wave's S reads are done before T overwrites them
      // ---- T image: silu(c1 + b1) planes over the S image (zero outside the clip)
      rp_t_image<A, G, C>(lds, bias_lds + m * C, acc, ln, r0, L);
      rp_barrier();
      RP_T(tc);
      // ---- c2 over rows [r0, r0 + R) from the T image.  Tap 0 loads the residual rows, taps 1 and 2
      // the next S image's rows (this tile's next ResBlock, or the next tile's first), each after the
      // tap's fragment reloads (k >= 3, so taps 0..2 exist; they are peeled so that the register
      // arrays are indexed by constants)
#pragma unroll
      for (int i = 0; i < RB; ++i) acc[i].zero();
      const float* nsrc = !last_m ? p.src[m + 1] + cb0 : p.src[0] + (long long)tl.nb * p.bstride;
      const int nsr0 = !last_m ? r0 : tl.nr0;
      RpRow res[RB];
      auto res_hook = [&] {
#pragma unroll
        for (int i = 0; i < RB; ++i) rp_load_res<G, C>(res[i], p.src[m] + cb0, ln, r0, L, i);
      };
      auto pf_hook0 = [&] {
        if (has_next) rp_fill_issue_range<G, C, 0, NIT / 2>(pf, nsrc, nsr0, L, tid);
      };
      auto pf_hook1 = [&] {
        if (has_next) rp_fill_issue_range<G, C, NIT / 2, NIT>(pf, nsrc, nsr0, L, tid);
      };
      tap(acc, 8 - hk, nrb2, rp_next_tap<G>(p, m, 1, 0), res_hook);
      tap(acc, 9 - hk, nrb2, rp_next_tap<G>(p, m, 1, 1), pf_hook0);
      tap(acc, 10 - hk, nrb2, rp_next_tap<G>(p, m, 1, 2), pf_hook1);
      for (int j = 3; j < k; ++j) tap(acc, 8 + j - hk, nrb2, rp_next_tap<G>(p, m, 1, j), no_hook);
      RP_T(te);
      // ---- epilogue: state + c2 + b2 (rows past the clip end are dropped)
      rp_epilogue<A, G, C, MEAN>(p, bias_lds + (kMaxGroup + m) * C, acc, res, macc, ln, m, cb0, r0, nrb2);
      RP_T(tf);
      if (has_next) {
        rp_barrier();  // every wave's T reads are done before the next S image overwrites them
        rp_fill_commit<A, G>(lds, pf, nsr0, L, tid);
        rp_barrier();
      }
      RP_STAMP({
        RP_T(tg);
        st.member(ta, tb, tc, te, tf, tg, k);
      })
    }
    if (!tl.more) break;
    tl.advance();
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the last tap's (unused) fragment reloads
  RP_STAMP(st.flush(C, tid);)
}

// conv_res_pair_h3 (round 5): conv_res_pair_g in h3 arithmetic (ResPairParams::h3; the fp16 h / l
// split of conv_gemm_x3dq, three products per fp32 product on v_mfma_f32_16x16x32_f16).  A K32 chunk
// of a tap is three MFMAs per 16 x 16 block, W{h'} . X{l}, W{l'} . X{h}, W{h'} . X{h}, the lanes of K
// group kg = lane >> 4 holding channel group kg of both operands: half the MFMAs of x6, two fragment
// reads per block and chunk instead of six, and images of 4 B per element instead of 6 (byte
// ((chunk * 8 + piece) * NS + row) * 16, piece = plane * 4 + channel group).  Weights: the
// ConvParams::w3 tap slices (dcx_w3_layout.h, the pair flavour; scaled by 2^w3_shift per conv); the
// accumulators are scaled back before the bias.  Schedule, tiles and hand-offs are conv_res_pair_g's.
// RAG: the ragged-batch instantiation (ResPairParams::clip_len honoured), launched only when the call
// has lengths: the kernels sit at the register limit, and with the length code in the one instantiation
// the padded path spilled more (conv_res_pair_h3<32,mean,624,ring>: 64 -> 124 bytes of scratch per lane).
template <int C, bool MEAN, int RR = kRp3Rows<C>, bool RING = false, bool RAG = false>
__global__ void __launch_bounds__(512, 1) conv_res_pair_h3(const ResPairParams p) {
#ifdef __HIP_DEVICE_COMPILE__  // the body is device code only (its host pass dropped the RING stubs)
  using A = RpH3;
  using G = RpGeom<A, C, RR>;
  constexpr int NCH = G::NCH, WR = G::WR, RB = G::RB1, PS = G::PS, IMG = G::IMG, NIT = G::NIT, WTAP = G::WTAP;
  // RING (round 6, Knobs::rp_ring): the weight taps through an LDS ring of NSLOT taps instead of
  // per-wave loads (below)
  constexpr int NSLOT = 4, RINGB = RING ? NSLOT * WTAP : 0, BIASB = G::BIASB;
  constexpr int NP = C * C / 256, PPW = (NP + 7) / 8;  // 1 KiB pieces per tap, per wave
  static_assert(IMG + RINGB + BIASB + 2 * NSLOT * 4 <= 160 * 1024, "LDS");
  __shared__ __attribute__((aligned(16))) char lds[IMG + RINGB + BIASB + (RING ? 2 * NSLOT * 4 : 0)];
  float* const bias_lds = reinterpret_cast<float*>(lds + IMG + RINGB);  // [conv][member][C]
  // ring counters: rd_cnt[slot] += 1 per wave once it holds a tap of the slot in registers, full_cnt[slot]
  // += 1 per wave once its pieces of the slot's tap have landed (monotone: use u of a slot is complete at 8 (u + 1))
  unsigned* const rd_cnt = reinterpret_cast<unsigned*>(lds + IMG + RINGB + BIASB);
  unsigned* const full_cnt = rd_cnt + NSLOT;

  const RpLane ln = RpLane::make<G>();
  const int tid = ln.tid, lane = ln.lane, wave = ln.wave, wc = ln.wc, wr = ln.wr;
  const int L = p.L, nmem = p.nmem;

  f32x4 pf[NIT][2];      // the next S image's rows in flight
  s16x8 wf[NCH][2][2];  // the weight fragments of a tap, [chunk][column block][h' | l'] of the lane's channel group
  const A::Wo wo = A::wo(lane, wc);
  const A::Xb xl = A::xlane<G::NS>(lds, lane);

  // ---- RING: the weight stream through LDS.  Tap t (counted over the whole kernel: c1 then c2 of
  // each member, tile after tile) sits in slot t % NSLOT as NP pieces of 1 KiB, piece (ch, column
  // block, h' | l') laid out as the fragment read of a wave (lane l: channel l & 15 of the block, K
  // group l >> 4), so every ds_read_b128 of a fragment is one linear 1 KiB piece (conflict-free).
  // Each wave issues pieces w, w + 8, ... of a tap by LDS-DMA, two taps ahead; per tap t it
  //   A. counts itself in rd_cnt[t % NSLOT] once its reads of tap t (made during tap t - 1) returned;
  //   B. waits for its own pieces of tap t + 1 (vmcnt, counted past the younger loads) and counts
  //      itself in full_cnt[(t + 1) % NSLOT];
  //   C. issues its pieces of tap t + 2 into that tap's slot once every wave has counted itself in as
  //      having read the slot's previous tap t + 2 - NSLOT;
  //   and after its chunk-0 MFMAs waits for full_cnt of tap t + 1 before reading it from the ring.
  // A wave counts itself in (A, B) before it waits on anything at a tap, so the slowest wave is never
  // blocked: no deadlock, and the waves stay within two taps of each other.  Replaces per-wave loads
  // of each tap's fragments from L2 / L1 (16 KiB per wave-pair at C = 64, 4x the tap; timing build
  // without them: 21.0 -> 13.5 ms for the C = 64 ParallelBlock, r06e).
  int ring_t = 0;                    // the tap being computed
  int ic_m = 0, ic_conv = 0, ic_j = 0;  // the next tap to issue (ring_t + 2 in the loop)
  int dsrc[PPW];                     // per-lane source offsets of this wave's pieces
#pragma unroll
  for (int i = 0; i < PPW; ++i) {
    dsrc[i] = w3_pair_piece(C, min(wave + 8 * i, NP - 1), lane);  // the piece's 1 KiB, contiguous (dcx_w3_layout.h)
  }
  // members' weights and tap counts picked by uniform selects (an index into the kernel-argument
  // arrays became a vector load that hipcc then waited for with vmcnt(0), DMA in flight included)
  auto mpick = [&](auto a0, auto a1, auto a2, int m) { return m == 0 ? a0 : m == 1 ? a1 : a2; };
  auto ring_issue = [&](int slot) {  // this wave's pieces of the issue cursor's tap, then advance it
    const unsigned short* w1 = mpick(p.w1[0], p.w1[1], p.w1[2], ic_m);
    const unsigned short* w2 = mpick(p.w2[0], p.w2[1], p.w2[2], ic_m);
    const unsigned short* wp = (ic_conv ? w2 : w1) + (long long)ic_j * (WTAP / 2);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)wp, 0, WTAP, 0x00020000);
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
      const int pc = wave + 8 * i;
      if (NP % 8 == 0 || pc < NP)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (rp_lds_t)(lds + IMG + slot * WTAP + pc * 1024), 16, dsrc[i], 0, 0, 0);
    }
    if (++ic_j == mpick(p.taps[0], p.taps[1], p.taps[2], ic_m)) {
      ic_j = 0;
      if (ic_conv == 0) ic_conv = 1;
      else {
        ic_conv = 0;
        ic_m = ic_m + 1 < nmem ? ic_m + 1 : 0;
      }
    }
  };
  // the counter read is inline asm: as a C++ LDS load hipcc made it wait for the wave's LDS-DMA in
  // flight (vmcnt(0): the pieces of tap t + 2, just issued), which it cannot tell apart from the slot
  auto spin_ge = [&](const unsigned* c, unsigned want) {
    const unsigned a = (unsigned)(size_t)(const __attribute__((address_space(3))) void*)c;
    for (;;) {
      unsigned v;
      asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(a) : "memory");
      if (__builtin_amdgcn_readfirstlane(v) >= want) break;
      __builtin_amdgcn_s_sleep(1);
    }
  };
  auto count_in = [&](unsigned* c) {  // inline asm for the same reason as spin_ge
    const unsigned a = (unsigned)(size_t)(__attribute__((address_space(3))) void*)c;
    if (lane == 0) asm volatile("ds_add_u32 %0, %1" ::"v"(a), "v"(1u) : "memory");
  };
  const int wrd = lane * 16 + (2 * wc) * 2 * 1024;  // lane part of a fragment read from the ring
  auto read_wf = [&](int slot, int ch) {
    const char* wb = lds + IMG + slot * WTAP + wrd;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      wf[ch][cb][0] = *reinterpret_cast<const s16x8*>(wb + ((ch * (C / 16) + cb) * 2 + 0) * 1024);
      wf[ch][cb][1] = *reinterpret_cast<const s16x8*>(wb + ((ch * (C / 16) + cb) * 2 + 1) * 1024);
    }
  };

  // ---- one tap, chunk-major: the MFMAs of chunk ch for every row block of the wave, then chunk ch
  // of the next tap into the fragment registers; hook() once every reload of the tap is issued (its
  // loads are then younger than the fragments the next tap waits for) ----
  // RING: hook() first (its nyoung global loads are then the only ones younger than the pieces B
  // waits for; nyoung may undercount, never overcount)
  auto tap = [&](RpRow (&acc)[RB], int rowoff, int nrb, const unsigned short* wnext, int nyoung, auto hook) {
    const A::Xb x = A::at(xl, (wr * 16 + rowoff) * 16);
    const int t = ring_t;
    if constexpr (RING) {
      hook();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // A
      count_in(rd_cnt + t % NSLOT);
      rp_wait(nyoung);  // B
      count_in(full_cnt + (t + 1) % NSLOT);
      spin_ge(rd_cnt + (t + 2) % NSLOT, 8u * (unsigned)((t + 2) / NSLOT));  // C
      ring_issue((t + 2) % NSLOT);
      ring_t = t + 1;
    }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
      for (int i = 0; i < RB; ++i) {
        if (i < nrb) rp_block<A>(acc[i], wf[ch], x, (WR * 16 * i) * 16 + ch * A::PPC * PS);
      }
      if constexpr (RING) {
        if (ch == 0) spin_ge(full_cnt + (t + 1) % NSLOT, 8u * (unsigned)((t + 1) / NSLOT + 1));
        read_wf((t + 1) % NSLOT, ch);
      } else {
        rp_load_wf<A, G, C>(wf[ch], wnext, ch, wo);
      }
      // keep the reloads here: left to itself the scheduler sinks all of them to the end of the tap,
      // and the next tap's first MFMAs then wait a whole L2 round trip
      __builtin_amdgcn_sched_barrier(0);
    }
    __builtin_amdgcn_s_setprio(0);
    if constexpr (!RING) hook();
  };
  auto no_hook = [] {};
  auto next_tap = [&](int m, int conv, int j) { return RING ? nullptr : rp_next_tap<G>(p, m, conv, j); };

  // c2 computes every row block (the waves owning fewer than RB of the R output rows compute rows past
  // them, from image rows inside the image, and drop them in the epilogue): a runtime row-block count
  // put a branch between the MFMAs of every row block (round 6: c2 taps ran 1.2-1.6x as long as c1's)
  const int nrb2 = min(RB, (G::NB2 - wr + WR - 1) / WR);
  // range shifts (round 6): member m's S image of clip bb from the measured max |state|, its T image
  // from the bound g1 max|state| + max|b1| of c1's output (|silu(v)| <= |v|)
  auto s_shift = [&](int m, int bb) { return p.src_amax[m] ? h2_shift(p.src_amax[m][bb]) : 0; };
  auto t_shift = [&](int m, int bb) {
    return p.src_amax[m] ? h2_shift(fmaf(p.g1[m], p.src_amax[m][bb], p.bm1[m])) : 0;
  };
  // the shifts of the tile's clip for every member, read once per tile into scalar registers (read
  // where they are used, each load's wait took every load and DMA in flight with it)
  // (RING: the launcher guarantees src_amax for every member, so the loads are unconditional and
  // issued together); shs0n: member 0's S shift of the next tile's clip
  int shs[kMaxGroup], sht[kMaxGroup], shs0n = 0;
  auto tile_shifts = [&](int bb, int nbb) {
    float a[kMaxGroup];
#pragma unroll
    for (int i = 0; i < kMaxGroup; ++i) a[i] = p.src_amax[i < nmem ? i : 0][bb];
    const float an = p.src_amax[0][nbb];
#pragma unroll
    for (int i = 0; i < kMaxGroup; ++i) {
      shs[i] = __builtin_amdgcn_readfirstlane(h2_shift(a[i]));
      sht[i] = __builtin_amdgcn_readfirstlane(h2_shift(fmaf(p.g1[i], a[i], p.bm1[i])));
    }
    shs0n = __builtin_amdgcn_readfirstlane(h2_shift(an));
  };
  RpTiles<G::R> tl;
  if (!tl.first(p)) return;  // whole workgroup, before any barrier
  rp_bias_prologue<C>(bias_lds, p, tid);
  if constexpr (RING) {
    if (tid < 2 * NSLOT) rd_cnt[tid] = 0u;
    rp_barrier();
    ring_issue(0);
    ring_issue(1);
  } else {
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) rp_load_wf<A, G, C>(wf[ch], p.w1[0], ch, wo);
  }
#pragma unroll
  for (int k = 0; k < NIT; ++k) rp_fill_issue<G, C>(pf[k], p.src[0] + (long long)tl.b * p.bstride, tl.r0, L, tid, k);
  rp_fill_commit<A, G>(lds, pf, tl.r0, L, tid, __builtin_ldexpf(1.0f, s_shift(0, tl.b)));
  if constexpr (RING) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    count_in(full_cnt + 0);  // tap 1's pieces are counted in by B of tap 0
  }
  rp_barrier();
  if constexpr (RING) {
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) read_wf(0, ch);
  }
  RpRow macc[MEAN ? RB : 1];
  RP_STAMP(RpStamps st;)
  for (;;) {
    tl.look_ahead();
    const int b = tl.b, r0 = tl.r0;
    if constexpr (RING) tile_shifts(b, tl.nb);
    // ragged batches: the clip's rows that hold data (a scalar load per tile).  Every producer of a
    // state tensor writes zeros from there to L, so the S images need no bound of their own; the T
    // image and the outputs take the clip's.
    const int Lc = RAG ? clip_rows(p.clip_len, p.len_mul, b, L) : L;
    if (RAG && r0 >= Lc) {
      // A tile wholly beyond its clip's length (never without clip_len: r0 < L): its outputs are zeros
      // and no tap is computed.  Workgroup-uniform, entered between tiles: every wave is past the
      // barrier that closed the S-image commit, nothing reads the image, and the weight stream stands
      // at a tile's first tap (fragments of tap 0 in registers, taps 0 and 1 in the ring or on their
      // way), which is where the next tile, live or not, picks it up.  Only the S image in LDS is this
      // tile's: the next tile's replaces it here, as the last member's c2 hooks would have.
      const long long cb0 = (long long)b * p.bstride;
      for (int i = tid; i < G::R * (C / 4); i += 512) {
        const int q = r0 + i / (C / 4), c4 = (i % (C / 4)) * 4;
        if (q >= L) break;
        const long long o = cb0 + (long long)q * C + c4;
        if constexpr (MEAN) {
          *reinterpret_cast<f32x4*>(p.mean_out + o) = f32x4{0.f, 0.f, 0.f, 0.f};
        } else {
          for (int m = 0; m < nmem; ++m) *reinterpret_cast<f32x4*>(mpick(p.dst[0], p.dst[1], p.dst[2], m) + o) = f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
      if (!tl.more) break;
      rp_fill_issue_range<G, C, 0, NIT>(pf, p.src[0] + (long long)tl.nb * p.bstride, tl.nr0, L, tid);
      rp_fill_commit<A, G>(lds, pf, tl.nr0, L, tid, __builtin_ldexpf(1.0f, RING ? shs0n : s_shift(0, tl.nb)));
      rp_barrier();
      tl.advance();
      continue;
    }
    for (int m = 0; m < nmem; ++m) {
      const int k = p.taps[m], hk = (k - 1) >> 1, d = p.dil[m];
      const long long cb0 = (long long)b * p.bstride;
      const bool last_m = m + 1 == nmem;
      const bool has_next = !last_m || tl.more;
      RpRow acc[RB];
      RP_T(ta);
      // ---- c1 over rows [r0 - 8, r0 + R + 8) from the S image
#pragma unroll
      for (int i = 0; i < RB; ++i) acc[i].zero();
      for (int j = 0; j < k; ++j) tap(acc, G::H1 + (j - hk) * d, RB, next_tap(m, 0, j), 0, no_hook);
      RP_T(tb);
      rp_barrier();  // every wave's S reads are done before T overwrites them
      // ---- T image, range-scaled (rigorous bound: no per-element check, epilogue_lds)
      const int sh_t = RING ? mpick(sht[0], sht[1], sht[2], m) : t_shift(m, b);
      const float us1 = __builtin_ldexpf(1.0f, -(p.w3_shift1[m] + (RING ? mpick(shs[0], shs[1], shs[2], m) : s_shift(m, b))));
      rp_t_image<A, G, C>(lds, bias_lds + m * C, acc, ln, r0, Lc, us1, __builtin_ldexpf(1.0f, sh_t));
      rp_barrier();
      RP_T(tc);
      // ---- c2 over rows [r0, r0 + R) from the T image.  Tap 0 loads the residual rows, taps 1 and 2
      // the next S image's rows (this tile's next ResBlock, or the next tile's first), each after the
      // tap's fragment reloads (k >= 3, so taps 0..2 exist; they are peeled so that the register
      // arrays are indexed by constants)
#pragma unroll
      for (int i = 0; i < RB; ++i) acc[i].zero();
      const float* nsrc = !last_m ? p.src[m + 1] + cb0 : p.src[0] + (long long)tl.nb * p.bstride;
      const int nsr0 = !last_m ? r0 : tl.nr0;
      RpRow res[RB];
      float dcur = 0.f;  // this clip's running max |dst| (range_report)
      auto res_hook = [&] {
        if constexpr (!MEAN) dcur = range_cur(p.dst_amax[m], b);  // older than the residual loads
#pragma unroll
        for (int i = 0; i < RB; ++i) rp_load_res<G, C>(res[i], p.src[m] + cb0, ln, r0, L, i);
      };
      // RING at C = 32: the empty asm makes tid opaque, so the items' image rows are computed here and
      // not hoisted out of the tile loop.  Hoisted, conv_res_pair_h3<32,mean,624,ring> spilled them and
      // reloaded them here from scratch, and each reload's vmcnt(0) wait took the weight DMA in flight
      // with it (3 reloads in the c2 taps: 3.24 ms per launch on the C2 bench against 3.02 with the asm;
      // scratch 120 -> 64 bytes per lane).  At C = 64 nothing was spilled and the recomputed item math
      // cost 0.7 % (conv_res_pair_h3<64,ring> 10.12 against 10.05 ms), so it keeps the plain tid.
      auto pf_tid = [&] {
        int t = tid;
        if constexpr (RING && C == 32) asm volatile("" : "+v"(t));
        return t;
      };
      auto pf_hook0 = [&] {
        if (has_next) rp_fill_issue_range<G, C, 0, NIT / 2>(pf, nsrc, nsr0, L, pf_tid());
      };
      auto pf_hook1 = [&] {
        if (has_next) rp_fill_issue_range<G, C, NIT / 2, NIT>(pf, nsrc, nsr0, L, pf_tid());
      };
      tap(acc, 8 - hk, RB, next_tap(m, 1, 0), RB * 2, res_hook);
      tap(acc, 9 - hk, RB, next_tap(m, 1, 1), has_next ? (NIT / 2) * 2 : 0, pf_hook0);
      tap(acc, 10 - hk, RB, next_tap(m, 1, 2), has_next ? (NIT - NIT / 2) * 2 : 0, pf_hook1);
      for (int j = 3; j < k; ++j) tap(acc, 8 + j - hk, RB, next_tap(m, 1, j), 0, no_hook);
      RP_T(te);
      // ---- epilogue; its max |.| per clip for the next pair's S image
      const float us2 = __builtin_ldexpf(1.0f, -(p.w3_shift2[m] + sh_t));
      [[maybe_unused]] const float dmax =
          rp_epilogue<A, G, C, MEAN>(p, bias_lds + (kMaxGroup + m) * C, acc, res, macc, ln, m, cb0, r0, nrb2, us2, RAG ? Lc : 0x7fffffff);
      if constexpr (!MEAN) {
        if (p.dst_amax[m]) range_report(dmax, p.dst_amax[m], b, __builtin_inff(), nullptr, dcur);  // workgroup-uniform
      }
      RP_T(tf);
      if (has_next) {
        rp_barrier();  // every wave's T reads are done before the next S image overwrites them
        rp_fill_commit<A, G>(lds, pf, nsr0, L, tid,
                             __builtin_ldexpf(1.0f, RING ? (last_m ? shs0n : mpick(shs[1], shs[2], shs[2], m))
                                                    : last_m ? s_shift(0, tl.nb) : s_shift(m + 1, b)));
        rp_barrier();
      }
      RP_STAMP({
        RP_T(tg);
        st.member(ta, tb, tc, te, tf, tg, k);
      })
    }
    if (!tl.more) break;
    tl.advance();
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the last tap's (unused) fragment reloads
  RP_STAMP(st.flush(C, tid);)
#endif
}

#ifdef RP_DIAG_STAMPS
extern "C" int dcx_diag_rp(unsigned long long* out32, int reset) {
  if (hipMemcpyFromSymbol(out32, HIP_SYMBOL(g_rp_diag), sizeof(unsigned long long) * 32) != hipSuccess) return -1;
  if (reset) {
    const unsigned long long z[32] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_rp_diag), z, sizeof z) != hipSuccess) return -1;
  }
  return 0;
}
#endif

hipError_t launch_res_pair(const ResPairParams& p, hipStream_t s, const char** kname) {
  if (p.nmem < 1 || p.nmem > kMaxGroup || p.batch < 1 || p.L < 1 || (p.C != 32 && p.C != 64))
    return hipErrorInvalidValue;
  if (p.clip_len && (!p.h3 || p.len_mul < 1)) return hipErrorNotSupported;  // only conv_res_pair_h3 is length-aware
  for (int m = 0; m < p.nmem; ++m) {
    const int hk = (p.taps[m] - 1) / 2;
    if (p.taps[m] < 1 || p.taps[m] % 2 == 0 || hk > 8 || p.dil[m] < 1 || hk * p.dil[m] > 32 || !p.src[m] ||
        !p.w1[m] || !p.w2[m] || !p.b1[m] || !p.b2[m] || (!p.mean_out && !p.dst[m]))
      return hipErrorInvalidValue;
  }
  static const Knobs kDefault{};
  const Knobs& kn = p.kn ? *p.kn : kDefault;
  const int cus = device_cus();
  // C = 32: the barrier-free conv_res_pair_g, C = 64: the step schedule; Knobs (A/B and
  // tests): rp_old runs the step schedule at C = 32 too, rp_g64 the barrier-free kernel at C = 64
  // rows per tile: the default unless a smaller tile finishes the launch sooner, by rounds of tiles
  // over the CUs (one workgroup each) times a tile's rows (c1 rows R + 16, c2 rows R, ~64 rows' worth of fixed
  // cost); Knobs::rp_rows forces one of the instantiated sizes.  Every size gives the same bits.
  static constexpr int kW8_32[3] = {496, 240, 112}, kW8_64[3] = {176, 112, 48};
  static constexpr int kH3_32[3] = {624, 240, 112}, kH3_64[3] = {240, 112, 48};
  const int* sizes = p.h3 ? (p.C == 32 ? kH3_32 : kH3_64) : (p.C == 32 ? kW8_32 : kW8_64);
  int si = 0;
  long long best = -1;
  for (int i = 0; i < 3; ++i) {
    const int r = sizes[i];
    const long long tiles = (long long)((p.L + r - 1) / r) * p.batch;
    const long long cost = (tiles + cus - 1) / cus * (2LL * r + 16 + 64);
    if (best < 0 || cost < best) {
      best = cost;
      si = i;
    }
  }
  for (int i = 0; i < 3; ++i)
    if (kn.rp_rows && sizes[i] == kn.rp_rows) si = i;
  const int R = sizes[si];
  const long long total = (long long)((p.L + R - 1) / R) * p.batch;
  if (total > (1LL << 30)) return hipErrorInvalidValue;
  const unsigned grid = (unsigned)std::min<long long>(total, cus);  // resident workgroups (LDS)
  const bool mean = p.mean_out != nullptr;
  // profile names are string literals (no shared buffer between threads)
#define DCX_RP_GO(KERN, CC, RR, NAME, ...)                                                  \
  do {                                                                                      \
    if (kname) *kname = mean ? #KERN "<" #CC ",mean" NAME ">" : #KERN "<" #CC NAME ">";     \
    if (mean) hipLaunchKernelGGL((KERN<CC, true, RR __VA_ARGS__>), dim3(grid), dim3(512), 0, s, p);   \
    else hipLaunchKernelGGL((KERN<CC, false, RR __VA_ARGS__>), dim3(grid), dim3(512), 0, s, p);       \
  } while (0)
#define DCX_RP_SIZES(KERN, CC, R0, R1, R2, ...)                \
  do {                                                         \
    if (si == 0) DCX_RP_GO(KERN, CC, R0, "" __VA_ARGS__);                  \
    else if (si == 1) DCX_RP_GO(KERN, CC, R1, ",small" __VA_ARGS__);       \
    else DCX_RP_GO(KERN, CC, R2, ",small" __VA_ARGS__);                    \
  } while (0)
  bool ring_ok = kn.rp_ring != 0;  // the ring kernel reads every member's src_amax unconditionally
  for (int m = 0; m < p.nmem; ++m) ring_ok = ring_ok && p.src_amax[m];
  if (p.h3 && p.clip_len) {  // ragged batch: the length-aware instantiations, ring or per-wave loads
    if (ring_ok) {
      if (p.C == 32) DCX_RP_SIZES(conv_res_pair_h3, 32, 624, 240, 112, ",ring", , true, true);
      else DCX_RP_SIZES(conv_res_pair_h3, 64, 240, 112, 48, ",ring", , true, true);
    } else {
      if (p.C == 32) DCX_RP_SIZES(conv_res_pair_h3, 32, 624, 240, 112, "", , false, true);
      else DCX_RP_SIZES(conv_res_pair_h3, 64, 240, 112, 48, "", , false, true);
    }
  } else if (p.h3 && ring_ok) {  // h3 weights, the LDS weight ring (round 6, default)
    if (p.C == 32) DCX_RP_SIZES(conv_res_pair_h3, 32, 624, 240, 112, ",ring", , true);
    else DCX_RP_SIZES(conv_res_pair_h3, 64, 240, 112, 48, ",ring", , true);
  } else if (p.h3) {  // h3 weights: conv_res_pair_h3 (the barrier-free schedule at both widths)
    if (p.C == 32) DCX_RP_SIZES(conv_res_pair_h3, 32, 624, 240, 112);
    else DCX_RP_SIZES(conv_res_pair_h3, 64, 240, 112, 48);
  } else if (p.C == 32 && !kn.rp_old) {
    DCX_RP_SIZES(conv_res_pair_g, 32, 496, 240, 112);
  } else if (p.C == 64 && !kn.rp_old && kn.rp_g64) {
    DCX_RP_SIZES(conv_res_pair_g, 64, 176, 112, 48);
  } else if (p.C == 32) {
    DCX_RP_SIZES(conv_res_pair, 32, 496, 240, 112);
  } else {
    DCX_RP_SIZES(conv_res_pair, 64, 176, 112, 48);
  }
#undef DCX_RP_SIZES
#undef DCX_RP_GO
  return hipGetLastError();
}

}  // namespace dcx
