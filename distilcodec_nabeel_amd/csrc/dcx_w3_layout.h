// The memory layout of the h3 weights (ConvParams::w3, ResPairParams::w1 / w2 under h3): one index
// function, w3_offset, that the packer (dcx_weights.cpp, h2_pack) writes through and from which every
// kernel that fetches the weights by LDS-DMA or per-wave loads takes its source offsets.  Plain C++
// (host and device, constexpr): tests/host/w3_layout_check.cpp includes it without HIP.
//
// An element is (phase r, tap m, input channel ci, output channel co, plane pl: 0 = h', 1 = l') of
// w * 2^w3_shift.  A step, one 32-channel chunk c = ci / 32 of one tap, is cout * 64 halves
// (cout * 128 bytes) in every flavour, steps in [phase][tap][chunk] order, so the total size, the
// descriptor sizes and the phase and tap bases are the same for all of them.  Inside a step, with
// channel group kg = (ci / 8) % 4 and e = ci % 8:
//   kW3Cols  [cout][kg 4][pl 2][e 8]: column-major, a column's chunk 128 contiguous bytes.
//   kW3Wide  [cout / 64][piece 8][64 columns][e 8], piece = pl * 4 + kg: each 64-column block in the
//            order of the conv kernels' LDS image ([piece][BN columns][16 B]), so the 1 KiB a DMA
//            instruction brings in (64 columns of one piece) is contiguous.  cout % 128 == 0.
//   kW3Pair  [cout / 16][pl 2][kg 4][16 columns][e 8]: each (16-column block, plane) in the lane
//            order of a weight fragment (lane l: column l & 15, channel group l >> 4), which is a
//            piece of the pair kernels' ring.  The ResBlock convs, cout 64 / 32.
// (A DMA instruction whose 64 lanes read 16 B each from 64 different 128-byte lines takes in 16 B per
// cycle and CU, one that reads 1 KiB contiguous 64 B: tools/probe/dma_shape.hip.)
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DCX_W3_HD __host__ __device__
#else
#define DCX_W3_HD
#endif

namespace dcx {

enum W3Flavour { kW3Cols = 0, kW3Wide = 1, kW3Pair = 2 };

// the flavour a conv's weights are packed in, by its output channels
DCX_W3_HD constexpr W3Flavour w3_flavour(int cout) {
  return cout % 128 == 0 ? kW3Wide : cout % 16 == 0 ? kW3Pair : kW3Cols;
}

// halves from the start of a step to element e = 0 of (column co, channel group kg, plane pl)
DCX_W3_HD constexpr int w3_in_step(W3Flavour f, int co, int kg, int pl) {
  return f == kW3Wide   ? (co >> 6) * 4096 + (pl * 4 + kg) * 512 + (co & 63) * 8
         : f == kW3Pair ? (co >> 4) * 1024 + pl * 512 + kg * 128 + (co & 15) * 8
                        : co * 64 + kg * 16 + pl * 8;
}
// halves from the start of the tensor to step (phase r, tap m, chunk c)
DCX_W3_HD constexpr long long w3_step(int taps, int cin, int cout, int r, int m, int c) {
  return (((long long)r * taps + m) * (cin / 32) + c) * cout * 64;
}
// index in halves of element (r, m, ci, co, pl) of a [phases][cout][taps][cin] conv
DCX_W3_HD constexpr long long w3_offset(int taps, int cin, int cout, int r, int m, int ci, int co, int pl) {
  return w3_step(taps, cin, cout, r, m, ci >> 5) + w3_in_step(w3_flavour(cout), co, (ci >> 3) & 3, pl) + (ci & 7);
}

// ---- byte offsets as the kernels use them: a descriptor over one phase (conv kernels) or one tap
// (pair kernels), a per-lane part kept in a VGPR and wave-uniform parts added per instruction ----

// conv kernels (conv_gemm_x3dq / x3dw): the step's scalar offset inside the phase
DCX_W3_HD constexpr int w3_step_bytes(int nchunks, int cout, int m, int c) { return (m * nchunks + c) * cout * 128; }
// DMA instruction k of a step's weight tile of BN columns at co0 fills LDS bytes [k, k + 1) KiB of the
// image [piece 8][BN][16 B]: piece (k * 64) / BN, columns (k * 64) % BN + lane.  Its source is the
// lane part plus the instruction part (co0 and the instruction's first column are multiples of 64, so
// the two add up to w3_in_step of the lane's column).
DCX_W3_HD constexpr int w3_wide_lane(int co0, int lane) { return w3_in_step(kW3Wide, co0 + lane, 0, 0) * 2; }
DCX_W3_HD constexpr int w3_wide_piece(int bn, int k) {
  const int u = k * 64, pc = u / bn, col = u - pc * bn;
  return w3_in_step(kW3Wide, col, pc & 3, pc >> 2) * 2;
}

// pair kernels (conv_res_pair_h3, C = cout = cin): piece pc of a tap, pc = (chunk * (C / 16) + column
// block) * 2 + plane, is ring bytes [pc, pc + 1) KiB in lane order; the per-wave fragment loads
// (DCX_RP_RING=0) read the same 16 B per lane straight from memory.  Offsets inside the tap.
DCX_W3_HD constexpr int w3_pair_lane(int col0, int lane, int pl) {
  return w3_in_step(kW3Pair, col0 + (lane & 15), lane >> 4, pl) * 2;
}
DCX_W3_HD constexpr int w3_pair_piece(int C, int pc, int lane) {
  const int cbk = (pc >> 1) % (C / 16), ch = (pc >> 1) / (C / 16);
  return ch * C * 128 + w3_pair_lane(cbk * 16, lane, pc & 1);
}

}  // namespace dcx
