// Host check of conv_gemm_x3dw's activation image (distilcodec_nabeel_amd/csrc/dcx_a3_layout.h), no GPU.
// For every tile form the kernels instantiate (image rows AR = 320 / 256: the 256 x 256 tiles with and
// without halo, 448 / 384: the 384 x 128 tiles), row pitches ldx = 32 ... 1024 and every chunk:
//   * DMA instructions x lanes -> image bytes is a bijection onto the image (AR * 128 bytes);
//   * each lane's source is the (row, piece) its image byte is read as: piece q = plane * 4 + channel
//     group of an h2 row's chunk lies at (q & 3) * 32 + (q >> 2) * 16 of its 128 bytes;
//   * every instruction touches exactly 8 128-byte lines, each run of 8 consecutive lanes one of them
//     (the shape LDS-DMA is fast at, tools/probe/dma_shape.hip);
//   * the fragment addresses the kernel forms (the lane's base a3_image(row, kg) recomputed per tap
//     offset, the l plane at that base ^ 64, 16-row blocks at 2 KiB as immediates) are those of the
//     rows and pieces the MFMA fragment wants, inside the image, and, for each of the four ds_read_b128 lane
//     groups ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32), the 16 addresses of every
//     fragment read (h and l, every row block, every wave row, tap offsets 0 ... 64) fall on 16
//     distinct 16-byte slots mod 256 B.
// The kernel's enumeration of its instructions and fragment reads is restated here from
// dcx_conv_h3.hip (x3dw_tile); the offsets come from the header's functions, which the kernel calls.
// Built by `make -C distilcodec_nabeel_amd/csrc a3check`; plain C++, so it also builds with
// -fsanitize=address,undefined (A3CHECK_FLAGS).
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "dcx_a3_layout.h"

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

struct Form { int AR, BM, WR; };  // image rows, tile rows, rows of a wave tile

// source byte (from the descriptor's base) of piece q of image row `row`, chunk c
static long long want_src(int rbase, int arow, int row, int q, int c) {
  return (long long)(rbase + row) * arow + c * 128 + (q & 3) * 32 + (q >> 2) * 16;
}

// the DMA of one chunk: fills src_of[image byte / 16] with each slot's source offset
static void dma_chunk(const Form& f, int ldx, int rbase, int c, std::vector<long long>& src_of) {
  const int arow = ldx * 4, A_N = f.AR / 8, A_PW = A_N / 4;
  std::vector<char> seen(f.AR * 8, 0);
  // group 0's wave gw issues k = i * 4 + gw, i < A_PW
  for (int gw = 0; gw < 4; ++gw)
    for (int i = 0; i < A_PW; ++i) {
      const int k = i * 4 + gw;
      std::set<long long> lines;
      long long run_line = 0;
      for (int lane = 0; lane < 64; ++lane) {
        const int dst = k * 1024 + lane * 16;  // an LDS-DMA instruction writes 1 KiB in lane order
        const int row = k * kA3BlockRows + a3_lane_row(lane), q = a3_lane_piece(lane);
        EXPECT(row >= 0 && row < f.AR && q >= 0 && q < 8, "AR %d k %d lane %d: row %d piece %d", f.AR, k, lane, row, q);
        EXPECT(a3_image(row, q) == dst, "AR %d k %d lane %d: image byte %d != %d", f.AR, k, lane, a3_image(row, q), dst);
        const long long src = (long long)a3_src_lane(rbase, arow, lane) + a3_src_inst(arow, k, c);
        EXPECT(src == want_src(rbase, arow, row, q, c), "AR %d ldx %d rbase %d c %d k %d lane %d: source %lld != %lld", f.AR,
               ldx, rbase, c, k, lane, src, want_src(rbase, arow, row, q, c));
        EXPECT((rbase + row < 0) == (src < 0), "row %d: source %lld must be negative exactly for negative rows", rbase + row, src);
        const long long line = src >= 0 ? src >> 7 : -((-src + 127) >> 7);
        lines.insert(line);
        if (lane % 8 == 0) run_line = line;
        EXPECT(line == run_line, "AR %d ldx %d k %d lane %d: lanes of a run of 8 on different lines", f.AR, ldx, k, lane);
        if (dst < 0 || dst + 16 > f.AR * 128) {
          EXPECT(false, "AR %d k %d lane %d: byte %d outside the image", f.AR, k, lane, dst);
          continue;
        }
        EXPECT(!seen[dst / 16], "AR %d: image byte %d written twice", f.AR, dst);
        seen[dst / 16] = 1;
        src_of[dst / 16] = src;
      }
      EXPECT(lines.size() == 8, "AR %d ldx %d k %d: %d lines", f.AR, ldx, k, (int)lines.size());
    }
  int cnt = 0;
  for (char s : seen) cnt += s;
  EXPECT(cnt == f.AR * 8, "AR %d: %d of %d slots written", f.AR, cnt, f.AR * 8);
}

// the fragment reads of one step at tap offset `off` (image rows): lane (l15, kg) of wave row wm reads
// row block i, plane pl at (base ^ pl * 64) + i * 2048, base = a3_image(wm * WR + l15 + off, kg)
static void fragment_reads(const Form& f, int ldx, int rbase, int c, int off, const std::vector<long long>& src_of) {
  static const int kGroups[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                     {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                     {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
                                     {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
  const int arow = ldx * 4, WM = f.BM / f.WR, TM = f.WR / 16;
  for (int wm = 0; wm < WM; ++wm)
    for (int i = 0; i < TM; ++i)
      for (int pl = 0; pl < 2; ++pl)
        for (int g = 0; g < 4; ++g) {
          unsigned slots = 0;
          for (int n = 0; n < 16; ++n) {
            const int lane = kGroups[g][n], l15 = lane & 15, kg = lane >> 4;
            const int addr = (a3_image(wm * f.WR + l15 + off, kg) ^ (pl ? kA3PlaneXor : 0)) + i * 2048;
            const int row = wm * f.WR + i * 16 + l15 + off, q = pl * 4 + kg;
            EXPECT(addr == a3_image(row, q), "AR %d off %d wm %d i %d pl %d lane %d: %d != %d", f.AR, off, wm, i, pl, lane,
                   addr, a3_image(row, q));
            if (addr < 0 || addr + 16 > f.AR * 128) {
              EXPECT(false, "AR %d off %d wm %d i %d lane %d: read at %d outside the image", f.AR, off, wm, i, lane, addr);
              continue;
            }
            EXPECT(src_of[addr / 16] == want_src(rbase, arow, row, q, c), "AR %d off %d row %d piece %d: read holds source %lld",
                   f.AR, off, row, q, src_of[addr / 16]);
            slots |= 1u << ((addr >> 4) & 15);
          }
          EXPECT(slots == 0xffffu, "AR %d off %d wm %d i %d pl %d lane group %d: slots %04x (bank conflict)", f.AR, off, wm, i,
                 pl, g, slots);
        }
}

int main() {
  const Form forms[] = {{320, 256, 64}, {256, 256, 64}, {448, 384, 48}, {384, 384, 48}};
  const int ldxs[] = {32, 64, 96, 128, 256, 384, 512, 768, 1024};
  static_assert(a3_image(0, 0) == 0 && a3_image(8, 0) == 1024 && a3_image(3, 5) == 3 * 128 + 7 * 16, "constexpr");
  int checked = 0;
  for (const Form& f : forms) {
    const int halo = f.AR - f.BM;
    for (int ldx : ldxs)
      for (int c = 0; c < ldx / 32; ++c)
        // image row 0 relative to the descriptor: the one-tap forms' descriptor starts at the tile
        for (int rbase : halo ? std::vector<int>{0, -64, -5, 256 - 3, 100000} : std::vector<int>{0}) {
          std::vector<long long> src_of(f.AR * 8, -1);
          dma_chunk(f, ldx, rbase, c, src_of);
          for (int off = 0; off <= halo; ++off) fragment_reads(f, ldx, rbase, c, off, src_of);
          ++checked;
        }
  }
  if (g_fail) {
    std::printf("a3 image: %d failures\n", g_fail);
    return 1;
  }
  std::printf("a3 image ok: %d forms, %d (form, ldx, chunk, base) cases\n", (int)(sizeof forms / sizeof *forms), checked);
  return 0;
}
