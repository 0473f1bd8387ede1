// Host launchers of the conv kernel families, one file each, for the dispatch in dcx_conv.hip
// (launch_conv, launch_conv_group, launch_conv_split_group).  The templates are defined and
// explicitly instantiated in their family's file for the shapes the dispatch names.
#pragma once
#include "dcx_kernels.h"

namespace dcx {

inline const Knobs& knobs(const ConvParams& p) {
  static const Knobs kDefaultKnobs{};
  return p.kn ? *p.kn : kDefaultKnobs;
}

// Tiles of a launch over (phase, clip, row tile, column tile), the order flat_tile decodes
template <int BM, int BN>
inline long long flat_tiles(const ConvParams& p, int batch, int phases) {
  return (long long)((p.Lq + BM - 1) / BM) * (p.Cout / BN) * batch * phases;
}
// The flat launch: one workgroup of `threads` per BM x BN tile, p with batch / phases set
template <int BM, int BN, class Kern>
hipError_t launch_flat(Kern kern, const ConvParams& p, int batch, int phases, int threads, hipStream_t s) {
  ConvParams q = p;
  q.batch = batch;
  q.phases = phases;
  hipLaunchKernelGGL(kern, dim3((unsigned)flat_tiles<BM, BN>(p, batch, phases)), dim3(threads), 0, s, q);
  return hipGetLastError();
}

// dcx_conv_x6w8.hip: conv_gemm_x6w8 (persistent), planes input or (af32) fp32 input split while staging
template <int BM, int BN, int WM, int WN, int HALO, bool ARGMIN>
hipError_t launch_x6w8(const ConvParams& p, int batch, int phases, hipStream_t s);
template <int BM, int BN, int WM, int WN, int HALO>
hipError_t launch_x6w8_af32(const ConvParams& p, int batch, int phases, hipStream_t s);

// dcx_conv_x6.hip: conv_gemm_x6lm (HALO = 0) / x6pp, x6pf (fp32 input, 512 x 64 tiles), x6dm, x6dq and
// the grouped launches (g filled by the dispatch, `blocks` its tile count)
template <int HALO>
hipError_t launch_x6pp(const ConvParams& p, int batch, int phases, hipStream_t s, const char** kname);
hipError_t launch_x6pf(const ConvParams& p, int batch, int phases, hipStream_t s, const char** kname);
template <int HALO, int BN>
hipError_t launch_x6dm(const ConvParams& p, int batch, int phases, hipStream_t s, const char** kname);
template <int BN>
hipError_t launch_x6dq(const ConvParams& p, int batch, int phases, hipStream_t s, const char** kname);
hipError_t launch_x6dq_group(const ConvGroup& g, int bn, unsigned blocks, hipStream_t s, const char** kname);
hipError_t launch_x6pp_group(const ConvGroup& g, unsigned blocks, hipStream_t s, const char** kname);

// dcx_conv_h3.hip: conv_gemm_x3dq / x3dm (BN = 256, 128), conv_gemm_x3dw (bsel = x3dq_bn's 512 or 384)
// and the grouped launches of either
bool x3dq_ok(const ConvParams& p, int bn, bool wide = false);
int x3dq_bn(const ConvParams& p);
template <int BN>
hipError_t launch_x3dq(const ConvParams& p, int batch, int phases, hipStream_t s, const char** kname);
hipError_t launch_x3dw(const ConvParams& p, int bsel, int batch, int phases, hipStream_t s, const char** kname);
hipError_t launch_h3_group(const ConvGroup& g, int bsel, bool split, unsigned blocks, hipStream_t s, const char** kname);

#if defined(DCX_CLOCK_DIAG) || defined(DCX_SEG_DIAG) || defined(DCX_TILE_DIAG)
// each file's DCX_DIAG_FILE (dcx_conv_common.h)
int diag_conv(int set, unsigned long long* out, int n, int reset);
int diag_vq(int set, unsigned long long* out, int n, int reset);
int diag_x6w8(int set, unsigned long long* out, int n, int reset);
int diag_x6(int set, unsigned long long* out, int n, int reset);
int diag_h3(int set, unsigned long long* out, int n, int reset);
#endif

}  // namespace dcx
