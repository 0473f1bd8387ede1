// Host check of the h3 weight layout (distilcodec_nabeel_amd/csrc/dcx_w3_layout.h), no GPU:
//   * w3_offset is a bijection onto [0, phases * taps * Cin * Cout * 2);
//   * for every tile origin, DMA instruction and lane, the source offset a kernel computes is the
//     offset of the element its LDS image expects at byte k * 1 KiB + lane * 16 of the weight tile:
//     conv_gemm_x3dq at BN = 128 / 256, conv_gemm_x3dw at BN = 256 / 128 (both SPLIT shares), the pair
//     kernels' ring at C = 64 / 32 and their per-wave fragment loads (DCX_RP_RING=0).
// The kernels' enumeration of their instructions (which wave issues which piece) is restated here from
// dcx_conv_h3.hip / dcx_resblock.hip; the offsets come from the header's functions, which the kernels call.
// Built by `make -C distilcodec_nabeel_amd/csrc w3check`; plain C++, so it also builds with
// -fsanitize=address,undefined (W3CHECK_FLAGS).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dcx_w3_layout.h"

using namespace dcx;

static int g_fail = 0;
#define EXPECT(c, ...)                                     \
  do {                                                     \
    if (!(c)) {                                            \
      if (g_fail++ < 20) {                                 \
        std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); \
        std::printf(__VA_ARGS__);                          \
        std::printf("\n");                                 \
      }                                                    \
    }                                                      \
  } while (0)

struct Shape { int phases, taps, cin, cout; };

static void bijection(const Shape& s) {
  const long long n = 2LL * s.phases * s.taps * s.cin * s.cout;
  std::vector<char> seen((size_t)n, 0);
  for (int r = 0; r < s.phases; ++r)
    for (int m = 0; m < s.taps; ++m)
      for (int ci = 0; ci < s.cin; ++ci)
        for (int co = 0; co < s.cout; ++co)
          for (int pl = 0; pl < 2; ++pl) {
            const long long o = w3_offset(s.taps, s.cin, s.cout, r, m, ci, co, pl);
            EXPECT(o >= 0 && o < n, "offset %lld of %lld", o, n);
            if (o < 0 || o >= n) continue;
            EXPECT(!seen[(size_t)o], "offset %lld twice (r %d m %d ci %d co %d pl %d)", o, r, m, ci, co, pl);
            seen[(size_t)o] = 1;
          }
  long long cnt = 0;
  for (char c : seen) cnt += c;
  EXPECT(cnt == n, "%lld of %lld offsets hit", cnt, n);
}

// one weight DMA instruction of a conv kernel: LDS byte k * 1 KiB + lane * 16 of the [piece 8][BN][16 B]
// image of the tile at co0 must receive element (piece k * 64 / BN, column k * 64 % BN + lane)
static void conv_instr(const Shape& s, int bn, int r, int m, int c, int co0, int k, std::vector<char>& hit) {
  const int nch = s.cin / 32;
  const long long phase_bytes = (long long)s.taps * nch * s.cout * 128;  // the descriptor's size
  if (k < 0 || k >= bn / 8 || hit[k]) {
    EXPECT(false, "instruction %d of %d out of range or issued twice", k, bn / 8);
    return;
  }
  hit[k] = 1;
  const int pc = k * 64 / bn, col0 = k * 64 % bn;
  for (int lane = 0; lane < 64; ++lane) {
    const long long in_phase = (long long)w3_step_bytes(nch, s.cout, m, c) + w3_wide_lane(co0, lane) + w3_wide_piece(bn, k);
    EXPECT(in_phase >= 0 && in_phase + 16 <= phase_bytes, "offset %lld outside the descriptor", in_phase);
    const long long got = 2 * w3_step(s.taps, s.cin, s.cout, r, 0, 0) + in_phase;
    const long long want = 2 * w3_offset(s.taps, s.cin, s.cout, r, m, c * 32 + (pc & 3) * 8, co0 + col0 + lane, pc >> 2);
    EXPECT(got == want, "bn %d r %d m %d c %d co0 %d k %d lane %d: %lld != %lld", bn, r, m, c, co0, k, lane, got, want);
  }
}

static void all_hit(const std::vector<char>& hit) {
  for (size_t k = 0; k < hit.size(); ++k) EXPECT(hit[k], "instruction %d never issued", (int)k);
}

static void conv_kernels(const Shape& s) {
  const int nch = s.cin / 32;
  for (int bn : {128, 256}) {
    if (s.cout % bn) continue;
    for (int r = 0; r < s.phases; ++r)
      for (int m = 0; m < s.taps; ++m)
        for (int c = 0; c < nch; ++c)
          for (int co0 = 0; co0 < s.cout; co0 += bn) {
            // conv_gemm_x3dq<BN>: group g's wave gw issues k = g * B_G + i * 4 + gw, i < B_PW
            {
              const int B_G = bn / 16, B_PW = B_G / 4;
              std::vector<char> hit(bn / 8, 0);
              for (int g = 0; g < 2; ++g)
                for (int gw = 0; gw < 4; ++gw)
                  for (int i = 0; i < B_PW; ++i) conv_instr(s, bn, r, m, c, co0, g * B_G + i * 4 + gw, hit);
              all_hit(hit);
            }
            // conv_gemm_x3dw<BN>: k = (group ? B_G0 : 0) + i * 4 + gw; group 0's share B_G0 of the B_N
            // instructions is all (no SPLIT), half (SPLIT, halo) or none (SPLIT, one tap)
            const int B_N = bn / 8;
            for (int B_G0 : {B_N, B_N / 2, 0}) {
              std::vector<char> hit(B_N, 0);
              for (int g = 0; g < 2; ++g)
                for (int gw = 0; gw < 4; ++gw)
                  for (int i = 0; i < (g ? B_N - B_G0 : B_G0) / 4; ++i)
                    conv_instr(s, bn, r, m, c, co0, (g ? B_G0 : 0) + i * 4 + gw, hit);
              all_hit(hit);
            }
          }
  }
}

// the pair kernels: C = cin = cout, one phase, a descriptor per tap
static void pair_kernels(const Shape& s) {
  const int C = s.cout, nch = C / 32, NP = C * C / 256, WTAP = C * C * 4;
  for (int m = 0; m < s.taps; ++m) {
    const long long tap = 2 * w3_step(s.taps, C, C, 0, m, 0);
    EXPECT(tap == (long long)m * WTAP, "tap base %lld", tap);
    // ring piece pc = (chunk * (C / 16) + column block) * 2 + plane at ring byte pc * 1 KiB, lane l:
    // column l & 15 of the block, K group l >> 4
    for (int pc = 0; pc < NP; ++pc)
      for (int lane = 0; lane < 64; ++lane) {
        const int pl = pc & 1, cbk = (pc >> 1) % (C / 16), ch = (pc >> 1) / (C / 16);
        const int off = w3_pair_piece(C, pc, lane);
        EXPECT(off >= 0 && off + 16 <= WTAP, "offset %d outside the tap", off);
        EXPECT(off == pc * 1024 + lane * 16, "piece %d lane %d at %d: not contiguous", pc, lane, off);
        const long long want = 2 * w3_offset(s.taps, C, C, 0, m, ch * 32 + (lane >> 4) * 8, cbk * 16 + (lane & 15), pl);
        EXPECT(tap + off == want, "C %d m %d pc %d lane %d: %lld != %lld", C, m, pc, lane, tap + off, want);
      }
    // per-wave loads: RpH3::wo's lane offsets of column block 2 * wc plus rp_load_wf's scalar offset
    // (ch * C + cb * 16) * WROW, WROW = 128
    for (int wc = 0; wc < C / 32; ++wc)
      for (int ch = 0; ch < nch; ++ch)
        for (int cb = 0; cb < 2; ++cb)
          for (int pl = 0; pl < 2; ++pl)
            for (int lane = 0; lane < 64; ++lane) {
              const int off = w3_pair_lane(2 * wc * 16, lane, pl) + (ch * C + cb * 16) * 128;
              EXPECT(off >= 0 && off + 16 <= WTAP, "offset %d outside the tap", off);
              const long long want =
                  2 * w3_offset(s.taps, C, C, 0, m, ch * 32 + (lane >> 4) * 8, (2 * wc + cb) * 16 + (lane & 15), pl);
              EXPECT(tap + off == want, "C %d m %d wc %d ch %d cb %d pl %d lane %d: %lld != %lld", C, m, wc, ch, cb, pl,
                     lane, tap + off, want);
            }
  }
}

int main() {
  const Shape shapes[] = {{1, 1, 32, 128}, {1, 3, 64, 256}, {2, 2, 64, 128}, {1, 11, 64, 512},
                          {8, 2, 64, 512}, {1, 3, 64, 64},  {1, 7, 32, 32}};
  static_assert(w3_offset(3, 64, 256, 0, 0, 0, 0, 0) == 0, "constexpr");
  static_assert(w3_flavour(512) == kW3Wide && w3_flavour(64) == kW3Pair && w3_flavour(32) == kW3Pair && w3_flavour(1) == kW3Cols,
                "flavours");
  int wide = 0, pair = 0;
  for (const Shape& s : shapes) {
    bijection(s);
    if (w3_flavour(s.cout) == kW3Wide) {
      conv_kernels(s);
      ++wide;
    } else if (w3_flavour(s.cout) == kW3Pair && s.cin == s.cout && s.phases == 1) {
      pair_kernels(s);
      ++pair;
    }
  }
  // the column-major flavour (any other cout) is a bijection too
  bijection({1, 3, 32, 1});
  bijection({2, 2, 64, 24});
  if (g_fail) {
    std::printf("w3 layout: %d failures\n", g_fail);
    return 1;
  }
  std::printf("w3 layout ok: %d shapes (%d wide, %d pair)\n", (int)(sizeof shapes / sizeof *shapes), wide, pair);
  return 0;
}
