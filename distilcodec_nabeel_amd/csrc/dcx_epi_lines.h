// The lane -> (row, channel) map of epilogue_form (dcx_conv_common.h), and the byte offsets its global
// and LDS accesses follow from it.  Plain C++ (host and device, constexpr):
// tests/host/epi_lines_check.cpp includes it without HIP.
//
// A thread owns kEpiG = 4 consecutive channels of a row, so the BN / 4 threads of a row are
// consecutive: the 64 lanes of a wave cover 256 consecutive channels of one row (BN = 256) or 128
// channels of each of two consecutive tile rows (BN = 128), and every 16-byte-per-lane instruction
// moves whole contiguous runs: 1 KiB, or two of 512 B, of fp32 (res, macc, y, y2), and as much of an h2
// image, whose 32-byte unit [h 8 | l 8] of 8 channels is written by the lane pair (2 g, 2 g + 1), the
// even lane the h piece and the odd lane the l piece (store_h2_pair, dcx_planes.h).  With 8 channels
// per thread (epilogue_lds) an instruction touched twice the lines and filled half of each;
// tools/probe/store_shape.hip, DESIGN.md §3.
// The tap forms run this map; the one-tap forms and three ragged 256-column forms keep 8 channels per
// thread (LINES in epilogue_form says why).
// A pass stages RPP tile rows in LDS, LDSW = BN + 4 floats apart; thread tid finishes rows
// epi_row0(tid) + j * epi_rstep(), j < RPP / epi_rstep().
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DCX_EPI_HD __host__ __device__
#else
#define DCX_EPI_HD
#endif

namespace dcx {

constexpr int kEpiG = 4;  // channels per thread: one 16-byte fp32 piece

// first channel of thread tid inside the tile's BN columns
DCX_EPI_HD constexpr int epi_chan(int tid, int BN) { return (tid % (BN / kEpiG)) * kEpiG; }
// first row of thread tid inside a pass, and the distance of its further rows
DCX_EPI_HD constexpr int epi_row0(int tid, int BN) { return tid / (BN / kEpiG); }
DCX_EPI_HD constexpr int epi_rstep(int NT, int BN) { return NT / (BN / kEpiG); }
// staging row pitch in floats, and the float index of the thread's 16-byte LDS read of pass row rl
DCX_EPI_HD constexpr int epi_ldsw(int BN) { return BN + 4; }
DCX_EPI_HD constexpr int epi_lds_float(int rl, int tid, int BN) { return rl * epi_ldsw(BN) + epi_chan(tid, BN); }
// fp32 tensors: float offset of the thread's piece in a row of the tile (column offset co0 of the row)
DCX_EPI_HD constexpr int epi_f32_off(int co0, int tid, int BN) { return co0 + epi_chan(tid, BN); }
// h2 images: a row is [C / 8 units][h 8 | l 8] fp16.  Channel c (a multiple of 4) lies in unit c >> 3;
// its thread stores the unit's h piece if c & 4 == 0 and the l piece otherwise, at this fp16 offset
// (equal to 2 c: the lanes of a row are 16 B apart), and is lane ^ 1 of the unit's other thread
DCX_EPI_HD constexpr int epi_h2_unit(int c) { return c >> 3; }
DCX_EPI_HD constexpr bool epi_h2_odd(int c) { return (c & 4) != 0; }
DCX_EPI_HD constexpr int epi_h2_off(int c) { return epi_h2_unit(c) * 16 + (epi_h2_odd(c) ? 8 : 0); }

}  // namespace dcx
