// Host check of epilogue_form's lane map (distilcodec_nabeel_amd/csrc/dcx_epi_lines.h), no GPU.
// For the tile forms the h3 kernels instantiate (256 x 256 with passes of 128 and of 64 rows, 384 x 128
// with passes of 192), 512 threads, every pass, every row index of a thread (hence every batch), and
// output pitches Cout = BN and 2 BN (tile column 0 and BN), out_mul 1 / 2 / 3:
//   * thread x row index -> (row, 4 channels) covers each element of the pass exactly once;
//   * the 64 lanes of each global instruction (one row index of one wave), as fp32 and as h2 bytes,
//     cover whole 128-byte lines only, 1 KiB in all;
//   * lanes 2 g and 2 g + 1 hold the two halves of one 32-byte h2 unit of one row, the even lane the h
//     piece and the odd lane the l piece, and a lane's piece lies at fp16 offset 2 c of the row;
//   * the 16 LDS reads of every 16-lane group fall on 16 distinct bank quads (16-byte slots mod 256 B).
// The enumeration of the instructions is restated here from dcx_conv_common.h (epilogue_form); the
// offsets come from the header's functions, which the kernel calls.
// Built by `make -C distilcodec_nabeel_amd/csrc epicheck`; plain C++, so it also builds with
// -fsanitize=address,undefined (EPICHECK_FLAGS).
#include <cstdio>
#include <map>
#include <vector>

#include "dcx_epi_lines.h"

using namespace dcx;

static int g_fail = 0;
#define EXPECT(c, ...)                                          \
  do {                                                          \
    if (!(c)) {                                                 \
      if (g_fail++ < 20) {                                      \
        std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); \
        std::printf(__VA_ARGS__);                               \
        std::printf("\n");                                      \
      }                                                         \
    }                                                           \
  } while (0)

struct Form { int BM, BN, RPP; };
constexpr int NT = 512;

// every touched 128-byte line holds all of its eight 16-byte pieces, `total` bytes in all
static void whole_lines(const std::map<long long, unsigned>& lines, int total, const char* what, const Form& f, int wave, int j) {
  int bytes = 0;
  for (const auto& kv : lines) {
    EXPECT(kv.second == 0xffu, "%s BN %d wave %d row index %d: line %lld pieces %02x", what, f.BN, wave, j, kv.first, kv.second);
    bytes += 128;
  }
  EXPECT(bytes == total, "%s BN %d wave %d row index %d: %d bytes", what, f.BN, wave, j, bytes);
}

static int check(const Form& f, int cout, int co0, int out_mul, int ph) {
  const int rstep = epi_rstep(NT, f.BN), rows_t = f.RPP / rstep;
  EXPECT(f.RPP % rstep == 0 && epi_ldsw(f.BN) % 4 == 0, "BN %d RPP %d", f.BN, f.RPP);
  int cases = 0;
  for (int r0 = 0; r0 < f.BM; r0 += f.RPP) {
    std::vector<char> seen((size_t)f.RPP * f.BN, 0);
    for (int wave = 0; wave < NT / 64; ++wave)
      for (int j = 0; j < rows_t; ++j) {
        std::map<long long, unsigned> f32_lines, h2_lines;
        for (int lane = 0; lane < 64; ++lane) {
          const int tid = wave * 64 + lane, rl = epi_row0(tid, f.BN) + j * rstep, cg = epi_chan(tid, f.BN);
          if (rl < 0 || rl >= f.RPP || cg < 0 || cg + kEpiG > f.BN) {
            EXPECT(false, "BN %d tid %d row index %d: row %d channel %d outside the pass", f.BN, tid, j, rl, cg);
            continue;
          }
          for (int e = 0; e < kEpiG; ++e) {
            EXPECT(!seen[(size_t)rl * f.BN + cg + e], "BN %d: row %d channel %d twice", f.BN, rl, cg + e);
            seen[(size_t)rl * f.BN + cg + e] = 1;
          }
          const int co = epi_f32_off(co0, tid, f.BN);
          const long long orow = (long long)(r0 + rl) * out_mul + ph;
          const long long fb = (orow * cout + co) * 4;                     // fp32: ldy = Cout
          const long long hb = (orow * cout * 2 + epi_h2_off(co)) * 2;     // h2: 4 B per element
          EXPECT(fb % 16 == 0 && hb % 16 == 0, "BN %d tid %d: misaligned piece", f.BN, tid);
          f32_lines[fb >> 7] |= 1u << ((fb >> 4) & 7);
          h2_lines[hb >> 7] |= 1u << ((hb >> 4) & 7);
          EXPECT(epi_h2_off(co) == 2 * co, "channel %d: h2 offset %d", co, epi_h2_off(co));
          // the pair of a unit: lane ^ 1, same row, same unit, h piece below the l piece
          const int ptid = tid ^ 1, pco = epi_f32_off(co0, ptid, f.BN);
          EXPECT(epi_row0(ptid, f.BN) == epi_row0(tid, f.BN), "tid %d: partner on another row", tid);
          EXPECT(epi_h2_unit(pco) == epi_h2_unit(co) && epi_h2_odd(co) == ((lane & 1) != 0) && epi_h2_odd(pco) != epi_h2_odd(co),
                 "tid %d: channels %d / %d are no unit's halves", tid, co, pco);
          EXPECT(epi_h2_off(co) == epi_h2_unit(co) * 16 + (lane & 1) * 8, "tid %d: piece at %d", tid, epi_h2_off(co));
        }
        whole_lines(f32_lines, 1024, "fp32", f, wave, j);
        whole_lines(h2_lines, 1024, "h2", f, wave, j);
        for (int g = 0; g < 4; ++g) {
          unsigned quads = 0;
          for (int n = 0; n < 16; ++n) {
            const int tid = wave * 64 + g * 16 + n, rl = epi_row0(tid, f.BN) + j * rstep;
            const int fl = epi_lds_float(rl, tid, f.BN);
            EXPECT(fl % 4 == 0 && fl >= 0 && fl + 4 <= f.RPP * epi_ldsw(f.BN), "BN %d tid %d: LDS float %d", f.BN, tid, fl);
            quads |= 1u << ((fl >> 2) & 15);
          }
          EXPECT(quads == 0xffffu, "BN %d wave %d row index %d lane group %d: bank quads %04x", f.BN, wave, j, g, quads);
        }
        ++cases;
      }
    size_t cnt = 0;
    for (char s : seen) cnt += s;
    EXPECT(cnt == seen.size(), "BN %d pass %d: %zu of %zu elements", f.BN, r0, cnt, seen.size());
  }
  return cases;
}

int main() {
  const Form forms[] = {{256, 256, 128}, {256, 256, 64}, {384, 128, 192}};
  static_assert(epi_chan(65, 256) == 4 && epi_row0(65, 256) == 1 && epi_rstep(512, 128) == 16 && epi_h2_off(12) == 24, "constexpr");
  int cases = 0;
  for (const Form& f : forms)
    for (int nt = 0; nt < 2; ++nt)       // the tile's column: Cout = BN, and the second tile of Cout = 2 BN
      for (int out_mul = 1; out_mul <= 3; ++out_mul)
        for (int ph = 0; ph < out_mul; ++ph) cases += check(f, (nt + 1) * f.BN, nt * f.BN, out_mul, ph);
  if (g_fail) {
    std::printf("epi lines: %d failures\n", g_fail);
    return 1;
  }
  std::printf("epi lines ok: %d forms, %d instructions\n", (int)(sizeof forms / sizeof *forms), cases);
  return 0;
}
