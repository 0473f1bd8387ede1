// Row helpers shared by the bandwidth-bound kernels (dcx_misc.hip, dcx_ragged.hip): the wave
// reduction and the LayerNorm finish of one row held by one wave.
#pragma once
#include "dcx_kernels.h"
#include "dcx_planes.h"

namespace dcx {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// ---------------------------------------------------------------------------------------------
// LayerNorm over the channel axis of each row.  channels_first_form=1 follows the reference's
// custom channels_first LayerNorm `(x-u)/sqrt(s+eps)*w+b` (convnext_utils.py:208-213);
// 0 follows F.layer_norm (`(x-u)*rsqrt(s+eps)*w+b`, convnext_utils.py:205).  Biased variance.
// 2: the channels_first form on a bf16 input under the reference's CUDA autocast (the encoder
// stem, whose Conv1d returns bf16; DCX_GEMM_BF16): `x.mean(1)` and `x - u` run in bf16 (fp32
// arithmetic, bf16 results), `.pow(2)` is on autocast's fp32 list, so s is the fp32 mean of the
// squared bf16 differences and the rest is fp32.
// One wave per row, NV float4 per lane (C = 256*NV).
// ---------------------------------------------------------------------------------------------
template <int NV>
__device__ __forceinline__ void ln_finish(f32x4 (&v)[NV], int C, float eps, int cf, const float* __restrict__ w,
                                          const float* __restrict__ b, float* __restrict__ yrow,
                                          unsigned short* __restrict__ y6, Layout lay, long long row, int lane,
                                          int* __restrict__ ash_row, float* __restrict__ amax_row) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
  float mean = wave_sum(s) / (float)C;
  if (cf == 2) {  // v := bf16(x - bf16(mean)); the fp32 steps below then see u = 0
    mean = bf16_val(bf16_bits(mean));
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = round_bf16x4(v[i] - mean);
    mean = 0.f;
  }
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const f32x4 d = v[i] - mean;
    sq += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
  }
  const float var = wave_sum(sq) / (float)C;
  const float den = sqrtf(var + eps);
  const float rstd = 1.0f / den;
  f32x4 ov[NV];
  float am = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (lane + 64 * i) * 4;
    const f32x4 wv = *reinterpret_cast<const f32x4*>(w + c);
    const f32x4 bv = *reinterpret_cast<const f32x4*>(b + c);
    f32x4 o;
    if (cf) {  // 1, 2
      o = (v[i] - mean) / den * wv + bv;
    } else {
      o = (v[i] - mean) * rstd * wv + bv;
    }
    ov[i] = o;
    am = fmaxf(am, fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fmaxf(fabsf(o.z), fabsf(o.w))));
    if (yrow) *reinterpret_cast<f32x4*>(yrow + c) = o;
  }
  if (!y6) return;
  // h2 (an h3 one-tap consumer): the row scaled by 2^h2_shift(its exact max |o|), the shift and the
  // max recorded per row (dcx_kernels.h)
  float sc = 1.0f;
  if (lay == LAYOUT_H2) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) am = fmaxf(am, __shfl_xor(am, off, 64));
    const int sh = h2_shift(am);
    sc = __builtin_ldexpf(1.0f, sh);
    if (lane == 0) {
      ash_row[row] = sh;
      if (amax_row) amax_row[row] = am;
    }
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (lane + 64 * i) * 4;
    const f32x4 o = ov[i];
    if (lay == LAYOUT_BF16) store_bf16x4(y6, row, C, c, o.x, o.y, o.z, o.w);
    else if (lay == LAYOUT_H2) store_h2_4(y6, row, C, c, o.x, o.y, o.z, o.w, sc);
    else store_planes4(y6, row, C, c, o.x, o.y, o.z, o.w);
  }
}

}  // namespace dcx
