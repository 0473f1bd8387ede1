// The LDS image of conv_gemm_x3dw's activation tile (x3dw_tile, every tiling) and the LDS-DMA map
// that fills it: the index functions the kernel takes both its DMA source offsets and its fragment
// addresses from.  Plain C++ (host and device, constexpr): tests/host/a3_image_check.cpp includes it
// without HIP.
//
// An h2 row's 32-channel chunk is 128 contiguous, 128-byte-aligned bytes in memory, [channel group 4]
// [plane 2: h, l][8 fp16]; a piece is 16 of them, q = plane * 4 + channel group.  An LDS-DMA
// instruction writes 1 KiB in lane order, and is fast where each run of 8 consecutive lanes reads
// one 128-byte line (tools/probe/dma_shape.hip, shapes d and g: 62 B per cycle and CU; with the same
// 8 lines spread so that consecutive lanes read different rows, shape f, 16 B, no better than the 64
// lines of one piece of 64 rows).  So instruction k fetches the whole chunk of the 8 rows
// [8 k, 8 k + 8), lanes 8 r ... 8 r + 7 the eight pieces of row 8 k + r, and the image is row-major,
// [AR rows][128 B], with the pieces of a row XOR-permuted by the row: piece q of row R sits in 16-byte
// slot q ^ (R & 6) of its row.
// Fragment reads (ds_read_b128, 16-byte slots mod 256 B, MI355X LDS banking): a 16-lane group holds
// rows base + {0-3, 12-15} of channel group kg and base + {4-11} of kg ^ 1, every row residue mod 8
// once per channel group.  The slot mod 16 is (R & 1) * 8 + (q ^ (R & 6)): for even q the four even
// slots of either half, for odd q the odd ones, each once over the 8 residues, so the 16 lanes fall on
// 16 distinct slots at any base, hence at any tap offset.  q ^ 4 is the other plane: the l address is
// the h address ^ 64.
// The address is not linear in the row, so a tap offset that is no multiple of 8 cannot be a uniform
// add: the kernel recomputes the lane's base per step (a3_image of its row and channel group);
// 16-row blocks (2 KiB, R & 6 unchanged) stay immediates.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DCX_A3_HD __host__ __device__
#else
#define DCX_A3_HD
#endif

namespace dcx {

constexpr int kA3BlockRows = 8;  // rows per DMA instruction (1 KiB of the image)
constexpr int kA3PlaneXor = 64;  // a piece's other plane: image byte ^ 64

// the permutation of a row's pieces: slot <-> piece of image row `row` (an involution)
DCX_A3_HD constexpr int a3_swz(int row, int q) { return q ^ (row & 6); }
// image byte of piece q of image row `row`
DCX_A3_HD constexpr int a3_image(int row, int q) { return row * 128 + a3_swz(row, q) * 16; }

// DMA: lane `lane` of instruction k writes image byte k * 1024 + lane * 16, which is piece
// a3_lane_piece(lane) of image row 8 k + a3_lane_row(lane)
DCX_A3_HD constexpr int a3_lane_row(int lane) { return lane >> 3; }
DCX_A3_HD constexpr int a3_lane_piece(int lane) { return a3_swz(lane >> 3, lane & 7); }
// byte of piece q inside a row's 128-byte chunk
DCX_A3_HD constexpr int a3_piece_src(int q) { return (q & 3) * 32 + (q >> 2) * 16; }
// source offset from the descriptor's base: the lane part (image row 0 at descriptor row rbase, rows
// arow bytes apart; a negative row gives a negative, i.e. out-of-range, offset) and the wave-uniform
// part of instruction k, chunk c
DCX_A3_HD constexpr int a3_src_lane(int rbase, int arow, int lane) {
  return (rbase + a3_lane_row(lane)) * arow + a3_piece_src(a3_lane_piece(lane));
}
DCX_A3_HD constexpr int a3_src_inst(int arow, int k, int c) { return k * kA3BlockRows * arow + c * 128; }

}  // namespace dcx
