// Device code shared by the fused ResBlock pair kernels of dcx_resblock.hip (conv_res_pair,
// conv_res_pair_g, conv_res_pair_h3): the tile geometry, the two arithmetics (x6 / h3: image format,
// element conversion, MFMA block, weight fragments), the S-image fill, the T-image write, the tile
// loop's bookkeeping, the residual loads, the epilogue with the ParallelBlock mean, and the
// diagnostic build's stamps.  Every helper is __forceinline__: the kernels sit at the register limit
// and each phase must compile as if written in place.
#pragma once
#include "dcx_kernels.h"
#include "dcx_planes.h"
#include "dcx_w3_layout.h"

namespace dcx {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float rp_silu(float v) { return v * __builtin_amdgcn_rcpf(1.0f + __expf(-v)); }
// barrier that leaves global loads in flight (only LDS traffic is drained)
__device__ __forceinline__ void rp_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
typedef __attribute__((address_space(3))) void* rp_lds_t;
// retire this wave's weight pieces: all but the n youngest vector-memory ops (the prefetch loads
// issued after the pieces) done
__device__ __forceinline__ void rp_wait(int n) {
#define RP_W(k) \
  case k: asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); break;
  switch (n) {
    RP_W(1) RP_W(2) RP_W(3) RP_W(4) RP_W(5) RP_W(6) RP_W(7) RP_W(8) RP_W(9) RP_W(10) RP_W(11) RP_W(12)
    RP_W(13) RP_W(14) RP_W(15) RP_W(16) RP_W(17) RP_W(18) RP_W(19) RP_W(20) RP_W(21) RP_W(22) RP_W(23) RP_W(24)
    RP_W(25) RP_W(26) RP_W(27) RP_W(28) RP_W(29) RP_W(30) RP_W(31) RP_W(32)
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // n > 32 waits for more: always safe
  }
#undef RP_W
}

// ---- the two arithmetics.  An image is piece-major and row-linear: byte ((chunk * PPC + piece) * NS +
// row) * 16, a chunk CW channels of a tap's K; ps below is the bytes per piece, NS * 16 ----

// x6 (conv_res_pair, conv_res_pair_g): three bf16 planes per element, piece = half * 3 + plane of a
// 16-channel chunk; weights [chunk][Cout][96 B], the ConvParams::w6 tap slice.  The lane holds half
// hf = (lane >> 4) & 1 and term t = lane >> 5 of the (term, channel) split of K.
struct RpX6 {
  static constexpr int PPC = 6, CW = 16, WB = 6;  // pieces per chunk, chunk width, weight bytes per element
  __device__ static __forceinline__ int piece(int g8) { return (g8 >> 1) * 6 + (g8 & 1) * 3; }  // of 8-channel group g8
  __device__ static __forceinline__ float scaled(float v, float) { return v; }
  template <class T>
  __device__ static __forceinline__ T pre(T acc, float, T bias) { return acc + bias; }
  // N = 8 or 4 consecutive channels of one image row as planes: one store per plane
  template <int N>
  __device__ static __forceinline__ void put(char* d, int ps, const float (&v)[N]) {
    typedef short vec __attribute__((ext_vector_type(N)));
    vec hv, mv, lv;
#pragma unroll
    for (int e = 0; e < N; ++e) {
      unsigned short h, m, l;
      split3(v[e], h, m, l);
      hv[e] = (short)h;
      mv[e] = (short)m;
      lv[e] = (short)l;
    }
    *reinterpret_cast<vec*>(d) = hv;
    *reinterpret_cast<vec*>(d + ps) = mv;
    *reinterpret_cast<vec*>(d + 2 * ps) = lv;
  }
  // lane offsets of the weight fragments {h', m'} and {h', l'} of column block 2 * wc in a tap slice
  struct Wo { int o0, o1; };
  __device__ static __forceinline__ Wo wo(int lane, int wc) {
    const int l15 = lane & 15, hf = (lane >> 4) & 1, t = lane >> 5;
    const int base = ((2 * wc) * 16 + l15) * 96 + hf * 48;
    return {base + t * 16, base + (t ? 32 : 0)};
  }
  // lane parts of the three activation reads (piece, row within the 16-row block); a tap adds its
  // wave-uniform row offset once, and row block / chunk offsets are instruction immediates
  struct Xb { const char *x0, *x1, *x2; };
  template <int NS>
  __device__ static __forceinline__ Xb xlane(const char* lds, int lane) {
    const int l15 = lane & 15, hf = (lane >> 4) & 1, t = lane >> 5;
    return {lds + ((hf * 3 + t) * NS + l15) * 16, lds + ((hf * 3 + (t ? 0 : 1)) * NS + l15) * 16,
            lds + ((hf * 3 + (t ? 0 : 2)) * NS + l15) * 16};
  }
  __device__ static __forceinline__ Xb at(const Xb& x, int tb) { return {x.x0 + tb, x.x1 + tb, x.x2 + tb}; }
  // the activation fragments of one row block of one chunk, and their three products with the
  // weight fragments wf = [{h',m'} | {h',l'}] of one column block:
  //   W{h',l'} . X{l,h} = lh' + hl',  W{h',m'} . X{m,h} = mh' + hm',  W{h',m'} . X{h,m} = hh' + mm'
  struct Xv { s16x8 x2, x1, x0; };
  __device__ static __forceinline__ Xv read(const Xb& x, int io) {
    return {*reinterpret_cast<const s16x8*>(x.x2 + io), *reinterpret_cast<const s16x8*>(x.x1 + io),
            *reinterpret_cast<const s16x8*>(x.x0 + io)};
  }
  __device__ static __forceinline__ f32x4 mma(f32x4 acc, const s16x8 (&wf)[2], const Xv& v) {
    const bf16x8 w0 = __builtin_bit_cast(bf16x8, wf[0]), w1 = __builtin_bit_cast(bf16x8, wf[1]);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, __builtin_bit_cast(bf16x8, v.x2), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, __builtin_bit_cast(bf16x8, v.x1), acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, __builtin_bit_cast(bf16x8, v.x0), acc, 0, 0, 0);
  }
};

// h3 (conv_res_pair_h3): fp16 h / l per element scaled by a power of two, piece = plane * 4 + channel
// group of a 32-channel chunk; weights: the ConvParams::w3 tap slice in the pair flavour of
// dcx_w3_layout.h, [chunk][16-column block][h' | l'][K group 4][16 columns][16 B].
// The lane holds channel group kg = lane >> 4 of both operands.
struct RpH3 {
  static constexpr int PPC = 8, CW = 32, WB = 4;
  __device__ static __forceinline__ int piece(int g8) { return (g8 >> 2) * 8 + (g8 & 3); }
  __device__ static __forceinline__ float scaled(float v, float sc) { return v * sc; }
  template <class T>
  __device__ static __forceinline__ T pre(T acc, float us, T bias) { return acc * us + bias; }
  template <int N>
  __device__ static __forceinline__ void put(char* d, int ps, const float (&v)[N]) {
    typedef short vec __attribute__((ext_vector_type(N)));
    vec hv, lv;
#pragma unroll
    for (int e = 0; e < N; ++e) {
      unsigned short hh, ll;
      split2h_nc(v[e], hh, ll);
      hv[e] = (short)hh;
      lv[e] = (short)ll;
    }
    *reinterpret_cast<vec*>(d) = hv;
    *reinterpret_cast<vec*>(d + 4 * ps) = lv;
  }
  // h' and l' of the lane's channel group in column block 2 * wc of chunk 0; a column block is 2 KiB
  // and a chunk C * 128 B further, as in x6's slices of WROW bytes per column (rp_load_wf)
  struct Wo { int o0, o1; };
  __device__ static __forceinline__ Wo wo(int lane, int wc) {
    return {w3_pair_lane(2 * wc * 16, lane, 0), w3_pair_lane(2 * wc * 16, lane, 1)};
  }
  // lane parts of the two activation reads (h and l pieces of the lane's channel group, row within
  // the 16-row block); a tap adds its wave-uniform row offset once, row block / chunk offsets are
  // instruction immediates
  struct Xb { const char *xh, *xl; };
  template <int NS>
  __device__ static __forceinline__ Xb xlane(const char* lds, int lane) {
    const int l15 = lane & 15, kg = lane >> 4;
    return {lds + (kg * NS + l15) * 16, lds + ((4 + kg) * NS + l15) * 16};
  }
  __device__ static __forceinline__ Xb at(const Xb& x, int tb) { return {x.xh + tb, x.xl + tb}; }
  // the activation fragments of one row block of one chunk, and their three products with the
  // weight fragments wf = [h' | l'] of one column block: W{h'} . X{l}, W{l'} . X{h}, W{h'} . X{h}
  struct Xv { s16x8 xl, xh; };
  __device__ static __forceinline__ Xv read(const Xb& x, int io) {
    return {*reinterpret_cast<const s16x8*>(x.xl + io), *reinterpret_cast<const s16x8*>(x.xh + io)};
  }
  __device__ static __forceinline__ f32x4 mma(f32x4 acc, const s16x8 (&wf)[2], const Xv& v) {
    const f16x8 w0 = __builtin_bit_cast(f16x8, wf[0]), w1 = __builtin_bit_cast(f16x8, wf[1]);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0, __builtin_bit_cast(f16x8, v.xl), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1, __builtin_bit_cast(f16x8, v.xh), acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(w0, __builtin_bit_cast(f16x8, v.xh), acc, 0, 0, 0);
  }
};

// The accumulators of one 16-row block: its two column blocks, 4 channels of one row per lane.  A
// struct, so that a wave's row blocks are an array of structs: as a plain f32x4[RB][2] hipcc's
// promote-alloca pass turned the short arrays (RB <= 4) into one 16- to 32-float vector before they
// were split into registers, and copied the whole vector around every runtime-bounded row block of c2
// (conv_res_pair_g<64,112>: 392 more v_mov_b64, +22 % instructions).
struct RpRow {
  f32x4 c[2];
  __device__ __forceinline__ void zero() { c[0] = c[1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
};

// the MFMA block: one row block of one chunk, both column blocks
template <class A>
__device__ __forceinline__ void rp_block(RpRow& acc, const s16x8 (&wf)[2][2], const typename A::Xb& x, int io) {
  const typename A::Xv v = A::read(x, io);
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) acc.c[cb] = A::mma(acc.c[cb], wf[cb], v);
}

// ---- geometry of a tile of RR output rows in arithmetic A: 8 waves as WR row groups x WC column
// halves (32 channels), each wave RB1 = RB2 row blocks of 16 rows in c1 and c2 ----
template <class A, int C, int RR>
struct RpGeom {
  static constexpr int R = RR;
  static constexpr int M1 = R + 16;              // c1 rows: [r0 - 8, r0 + R + 8)
  static constexpr int H1 = 32;                  // largest c1 reach (k - 1) / 2 * d
  static constexpr int NS = M1 + 2 * H1;         // S image rows
  static constexpr int NCH = C / A::CW;          // chunks per tap
  static constexpr int WC = C / 32, WR = 8 / WC;
  static constexpr int NB1 = M1 / 16, RB1 = NB1 / WR;
  static constexpr int NB2 = R / 16, RB2 = (NB2 + WR - 1) / WR;
  static constexpr int PS = NS * 16;             // bytes per piece of one chunk
  static constexpr int IMG = NCH * A::PPC * PS;  // S image bytes (T reuses its start)
  static constexpr int WTAP = C * C * A::WB;     // one tap of weights (bytes)
  static constexpr int WROW = A::CW * A::WB;     // one output channel of a chunk of a tap slice (bytes)
  static constexpr int G8 = C / 8;               // 8-channel groups per row
  static constexpr int NIT = (NS * G8 + 511) / 512;  // S-image items (one row, 8 channels) per thread
  static constexpr int BIASB = 2 * kMaxGroup * C * 4;  // [conv][member][C] fp32
  static_assert(NB1 % WR == 0 && RB1 == RB2, "row blocks per wave");
  static_assert(IMG + BIASB <= 160 * 1024, "LDS");
};

// this thread's place in the workgroup
struct RpLane {
  int tid, lane, wave, wc, wr, l15;
  template <class G>
  __device__ static __forceinline__ RpLane make() {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    return {tid, lane, wave, wave % G::WC, wave / G::WC, lane & 15};
  }
  // first of the lane's 4 accumulator channels in column block cb
  __device__ __forceinline__ int c0(int cb) const { return (2 * wc + cb) * 16 + 4 * (lane >> 4); }
};

// ---- tile bookkeeping: a workgroup walks tiles blockIdx.x, + gridDim.x, ... of ntl row tiles per clip ----
template <int R>
struct RpTiles {
  int ntl, total, tile, b, r0;
  int next_tile, nb, nr0;  // the tile after this one (look_ahead)
  bool more;
  __device__ __forceinline__ bool first(const ResPairParams& p) {
    ntl = (p.L + R - 1) / R;
    total = ntl * p.batch;
    tile = blockIdx.x;
    if (tile >= total) return false;
    b = tile / ntl;
    r0 = (tile - b * ntl) * R;
    return true;
  }
  __device__ __forceinline__ void look_ahead() {
    next_tile = tile + gridDim.x;
    more = next_tile < total;
    nb = more ? next_tile / ntl : 0;
    nr0 = more ? (next_tile - nb * ntl) * R : 0;
  }
  __device__ __forceinline__ void advance() {
    tile = next_tile;
    b = nb;
    r0 = nr0;
  }
};

// biases of every member's c1 and c2 into LDS as [conv][member][C]
template <int C>
__device__ __forceinline__ void rp_bias_prologue(float* bias_lds, const ResPairParams& p, int tid) {
  const int nmem = p.nmem;
  if (tid < 2 * nmem * C) {
    const int conv = tid / (nmem * C), m = (tid / C) % nmem, c = tid % C;
    bias_lds[(conv * kMaxGroup + m) * C + c] = (conv ? p.b2[m] : p.b1[m])[c];
  }
}

// ---- S image fill: state rows -> registers (issue) -> silu, image format, LDS (commit).  Item it of
// a tile at r0 is image row s, 8-channel group g8, clip row a ----
template <class G>
struct RpItem {
  int s, g8, a;
  __device__ __forceinline__ RpItem(int it, int r0)
      : s(((it >> 3) / G::G8) * 8 + (it & 7)), g8((it >> 3) % G::G8), a(r0 - 8 - G::H1 + s) {}
};
template <class G, int C>
__device__ __forceinline__ void rp_fill_issue(f32x4 (&pf)[2], const float* src, int r0, int L, int tid, int k) {
  const RpItem<G> q(min(tid + 512 * k, G::NS * G::G8 - 1), r0);  // unconditional (rp_wait counts the loads)
  const f32x4* g = reinterpret_cast<const f32x4*>(src + (long long)min(max(q.a, 0), L - 1) * C + q.g8 * 8);
  pf[0] = g[0];
  pf[1] = g[1];
}
// items [K0, K1) of the thread (a c2 hook's share of the next S image)
template <class G, int C, int K0, int K1>
__device__ __forceinline__ void rp_fill_issue_range(f32x4 (&pf)[G::NIT][2], const float* src, int r0, int L, int tid) {
#pragma unroll
  for (int kk = K0; kk < K1; ++kk) rp_fill_issue<G, C>(pf[kk], src, r0, L, tid, kk);
}
// sc: the image's range scale (h3), 2^h2_shift(max |state| of the clip) (dcx_kernels.h)
template <class A, class G>
__device__ __forceinline__ void rp_fill_commit(char* lds, const f32x4 (&pf)[G::NIT][2], int r0, int L, int tid,
                                               float sc = 1.0f) {
#pragma unroll
  for (int k = 0; k < G::NIT; ++k) {
    const int it = tid + 512 * k;
    if (!(G::NIT * 512 == G::NS * G::G8 || it < G::NS * G::G8)) continue;
    const RpItem<G> q(it, r0);
    const bool ok = q.a >= 0 && q.a < L;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float sv = A::scaled(rp_silu(pf[k][e >> 2][e & 3]), sc);
      v[e] = ok ? sv : 0.f;
    }
    A::template put<8>(lds + A::piece(q.g8) * G::PS + q.s * 16, G::PS, v);
  }
}

// ---- T image: silu(c1 + b1) in the image format over the S image (zero outside the clip).  us: the
// accumulators' scale back (h3), tsc: the T image's range scale (h3) ----
template <class A, class G, int C>
__device__ __forceinline__ void rp_t_image(char* lds, const float* bias1, const RpRow (&acc)[G::RB1],
                                           const RpLane& ln, int r0, int L, float us = 1.0f, float tsc = 1.0f) {
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) {
    const int c0 = ln.c0(cb);
    const f32x4 bias = *reinterpret_cast<const f32x4*>(bias1 + c0);
#pragma unroll
    for (int i = 0; i < G::RB1; ++i) {
      const int ir = (ln.wr + G::WR * i) * 16 + ln.l15, a = r0 - 8 + ir;
      const bool ok = a >= 0 && a < L;
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float sv = rp_silu(A::pre(acc[i].c[cb][e], us, bias[e]));
        v[e] = ok ? A::scaled(sv, tsc) : 0.f;
      }
      A::template put<4>(lds + A::piece(c0 >> 3) * G::PS + ir * 16 + (c0 & 7) * 2, G::PS, v);
    }
  }
}

// ---- per-wave weight fragments of chunk ch of a tap slice, [column block][fragment]: buffer loads
// whose lane offsets are loop-invariant VGPRs, the tap base a scalar resource and the chunk /
// column-block offsets scalar constants, so a reload costs no address arithmetic ----
template <class A, class G, int C>
__device__ __forceinline__ void rp_load_wf(s16x8 (&wf)[2][2], const unsigned short* wtap, int ch,
                                           const typename A::Wo& wo) {
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)wtap, 0, G::WTAP, 0x00020000);
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) {
    const int so = (ch * C + cb * 16) * G::WROW;
    wf[cb][0] = __builtin_bit_cast(s16x8, __builtin_amdgcn_raw_buffer_load_b128(rw, wo.o0, so, 0));
    wf[cb][1] = __builtin_bit_cast(s16x8, __builtin_amdgcn_raw_buffer_load_b128(rw, wo.o1, so, 0));
  }
}
// the tap after tap j of conv `conv` of member m: the stream runs c1, c2 of each member, then
// member 0 again (the next tile; past the last tile harmless loads of weights already used)
template <class G>
__device__ __forceinline__ const unsigned short* rp_next_tap(const ResPairParams& p, int m, int conv, int j) {
  if (j + 1 < p.taps[m]) return (conv ? p.w2[m] : p.w1[m]) + (long long)(j + 1) * (G::WTAP / 2);
  if (conv == 0) return p.w2[m];
  return p.w1[m + 1 < p.nmem ? m + 1 : 0];
}

// ---- c2's residual rows of row block i (rows past the clip end read its last row; dropped later) ----
template <class G, int C>
__device__ __forceinline__ void rp_load_res(RpRow& res, const float* src, const RpLane& ln, int r0, int L, int i) {
  const int q = min(r0 + (ln.wr + G::WR * i) * 16 + ln.l15, L - 1);
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) res.c[cb] = *reinterpret_cast<const f32x4*>(src + (long long)q * C + ln.c0(cb));
}

// ---- epilogue: v = state + c2 + b2 (rows past the clip end are dropped) to dst[m], or with MEAN into
// the ParallelBlock mean, kept in macc across the members in ResBlock order (m = v0; m += v1;
// m = (m + v2) / 3) and written as silu(mean).  Returns max |v| over what this lane stored to dst
// (!MEAN; the h3 kernel's range report).  us: the accumulators' scale back (h3).  Lc: the rows of the
// clip that hold data (ragged batches, ResPairParams::clip_len): rows in [Lc, p.L) are written as
// zeros, the zero padding the clip sees alone, and stay out of the max ----
template <class A, class G, int C, bool MEAN>
__device__ __forceinline__ float rp_epilogue(const ResPairParams& p, const float* bias2, const RpRow (&acc)[G::RB1],
                                             const RpRow (&res)[G::RB1], RpRow (&macc)[MEAN ? G::RB1 : 1],
                                             const RpLane& ln, int m, long long cb0, int r0, int nrb2, float us = 1.0f,
                                             int Lc = 0x7fffffff) {
  const bool last_m = m + 1 == p.nmem;
  float dmax = 0.f;
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) {
    const int c0 = ln.c0(cb);
    const f32x4 bias = *reinterpret_cast<const f32x4*>(bias2 + c0);
#pragma unroll
    for (int i = 0; i < G::RB1; ++i) {
      if (i >= nrb2) break;
      const int q = r0 + (ln.wr + G::WR * i) * 16 + ln.l15;
      const f32x4 vf = res[i].c[cb] + A::pre(acc[i].c[cb], us, bias);
      const f32x4 v = q < Lc ? vf : f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (!MEAN) {
        if (q < p.L) {
          *reinterpret_cast<f32x4*>(p.dst[m] + cb0 + (long long)q * C + c0) = v;
          dmax = fmaxf(dmax, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
        }
      } else if (m == 0) {
        macc[i].c[cb] = v;
      } else if (!last_m) {
        macc[i].c[cb] = macc[i].c[cb] + v;
      } else {
        const f32x4 mv = (macc[i].c[cb] + v) / 3.0f;
        f32x4 sv;
#pragma unroll
        for (int e = 0; e < 4; ++e) sv[e] = rp_silu(mv[e]);
        if (q < p.L) *reinterpret_cast<f32x4*>(p.mean_out + cb0 + (long long)q * C + c0) = sv;
      }
    }
  }
  return dmax;
}

// ---- diagnostic build (-DRP_DIAG_STAMPS, tools/rp_stamps.py): shader-clock sums per phase (wave 0
// of every workgroup): [0] c1 taps / steps, [1] T image, [2] c2, [3] epilogue, [4] next S image,
// [5] member-tiles, [6] c1 steps counted, [7] c2 steps counted, [8] c1 step MFMA phases, [9] c1 step
// barrier waits (conv_res_pair only) ----
#ifdef RP_DIAG_STAMPS
__device__ unsigned long long g_rp_diag[32];  // [C == 64][16]
#define RP_T(v) const unsigned long long v = __builtin_amdgcn_s_memtime()
struct RpStamps {
  unsigned long long dg[16] = {};
  __device__ __forceinline__ void member(unsigned long long ta, unsigned long long tb, unsigned long long tc,
                                         unsigned long long te, unsigned long long tf, unsigned long long tg, int n) {
    dg[0] += tb - ta; dg[1] += tc - tb; dg[2] += te - tc; dg[3] += tf - te; dg[4] += tg - tf;
    dg[5] += 1; dg[6] += n; dg[7] += n;
  }
  __device__ __forceinline__ void flush(int C, int tid) {
    if (tid == 0)
      for (int i = 0; i < 16; ++i) atomicAdd(&g_rp_diag[(C == 64 ? 16 : 0) + i], dg[i]);
  }
};
#define RP_STAMP(...) __VA_ARGS__
#else
#define RP_T(v)
#define RP_STAMP(...)
#endif

}  // namespace dcx
