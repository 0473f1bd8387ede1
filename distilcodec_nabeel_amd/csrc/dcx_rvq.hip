// Residual VQ (ResidualVQ, residual_vq.py:140-259): the steps between the layers' searches and the
// chain's decode.  Both kernels are bandwidth-bound row passes: one wave per row, 8 channels (two
// 16-byte loads, 16-byte stores per plane) per lane and step, no cross-lane traffic but the row sums.
#include "dcx_kernels.h"
#include "dcx_planes.h"

namespace dcx {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void load8(const float* p, float (&v)[8]) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    v[e] = a[e];
    v[4 + e] = b[e];
  }
}
__device__ __forceinline__ void store8(float* p, const float (&v)[8]) {
  *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
  *reinterpret_cast<f32x4*>(p + 4) = f32x4{v[4], v[5], v[6], v[7]};
}
// 8 channels of one row in the layout lay (planes or compact bf16)
__device__ __forceinline__ void store_image8(unsigned short* y6, Layout lay, long long row, int C, int c,
                                             const float (&v)[8]) {
  if (lay == LAYOUT_BF16) store_bf16x8(y6, row, C, c, v);
  else store_planes8(y6, row, C, c, v);
}

// One layer's step of the chain, per row: e = E_k[c_k], then in one pass
//   codes_out[row * R] = c_k               (the [rows][R] codes tensor, the caller's pointer at layer k)
//   fup = e (first) or fup + e             (fp32, so the sum is in layer order)
//   dst = fl32(src - e)                    (the next layer's input; dst may be src)
//   op6 = dst in the next search's layout  (compact bf16 hi, or planes)
//   x2 / x2d / xr2 = |dst|^2 (fp64 sum, rounded once for x2), |dst - bf16(dst)|^2: what row_sqnorm
//   gives the search, by the same shuffle reduction (no atomics: the same bits every run)
// and thread 0 zeroes the rescore's pair counter as row_sqnorm does.  Null outputs are skipped; the
// last layer passes dst = null and runs the codes / fup part alone.
__global__ void __launch_bounds__(256) vq_residual_step_kernel(VqResidualArgs a) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (a.zero_me && blockIdx.x == 0 && threadIdx.x == 0) *a.zero_me = 0;
  if (row >= a.rows) return;
  int c = a.ck[row];
  if (c < 0 || c >= a.ncodes) c = 0;  // the search only writes codes of the codebook
  if (lane == 0 && a.codes_out) a.codes_out[row * a.R] = c;
  const int C = a.dim;
  const float* e = a.codebook + (long long)c * C;
  const float* src = a.src + row * C;
  double s = 0.0, r = 0.0;
  for (int ch = lane * 8; ch < C; ch += 512) {
    float ev[8];
    load8(e + ch, ev);
    if (a.fup) {
      float f[8];
      if (a.fup_first) {
#pragma unroll
        for (int k = 0; k < 8; ++k) f[k] = ev[k];
      } else {
        load8(a.fup + row * C + ch, f);
#pragma unroll
        for (int k = 0; k < 8; ++k) f[k] += ev[k];
      }
      store8(a.fup + row * C + ch, f);
    }
    if (!a.dst) continue;
    float v[8];
    load8(src + ch, v);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      v[k] -= ev[k];
      s += (double)v[k] * v[k];
      const double d = (double)v[k] - (double)bf16_val(bf16_bits(v[k]));
      r += d * d;
    }
    store8(a.dst + row * C + ch, v);
    if (a.op6) store_image8(a.op6, a.op_layout, row, C, ch, v);
  }
  if (!a.dst) return;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    s += __shfl_xor(s, off, 64);
    r += __shfl_xor(r, off, 64);
  }
  if (lane == 0) {
    if (a.x2) a.x2[row] = (float)s;
    if (a.x2d) a.x2d[row] = s;
    if (a.xr2) a.xr2[row] = (float)r;
  }
}

hipError_t launch_vq_residual_step(const VqResidualArgs& a, hipStream_t s) {
  if (!a.ck || !a.codebook || a.rows < 0 || a.dim < 8 || a.dim % 8 || a.ncodes < 1 || a.R < 1) return hipErrorInvalidValue;
  if (a.dst && !a.src) return hipErrorInvalidValue;
  if (a.op6 && (!a.dst || (a.op_layout != LAYOUT_PLANES && a.op_layout != LAYOUT_BF16))) return hipErrorInvalidValue;
  if (a.rows == 0) return hipSuccess;
  hipLaunchKernelGGL(vq_residual_step_kernel, dim3((unsigned)((a.rows + 3) / 4)), dim3(256), 0, s, a);
  return hipGetLastError();
}

// out[row] = sum_k masked(E_k[idx[row][k]]) in fp32, in layer order (get_output_from_indices,
// residual_vq.py:103-138, before project_out).  Index rules of gather_rows per entry: -1 is the
// masked code and adds nothing, other negative indices wrap, anything still outside [0, ncodes) reads
// row 0 and is counted.  clip_len / frames as in gather_rows: a row at or beyond its clip's length is
// written as zeros and its indices are not read.  out (fp32) and / or out6 (planes or compact bf16).
__global__ void __launch_bounds__(256) gather_sum_rows_kernel(GatherSumArgs a) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.rows) return;
  const int C = a.dim;
  const float* e[kMaxCodebooks];
  bool live = !(a.clip_len && row % a.frames >= a.clip_len[row / a.frames]);
#pragma unroll
  for (int k = 0; k < kMaxCodebooks; ++k) {
    e[k] = nullptr;
    if (!live || k >= a.R) continue;
    const int raw = a.idx[row * a.R + k];
    if (raw == -1) continue;
    int i = raw < 0 ? raw + a.ncodes : raw;
    if (i < 0 || i >= a.ncodes) {
      if (lane == 0 && a.n_invalid) atomicAdd(a.n_invalid, 1);
      i = 0;
    }
    e[k] = a.table[k] + (long long)i * C;
  }
  for (int ch = lane * 8; ch < C; ch += 512) {
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    bool first = true;
#pragma unroll
    for (int k = 0; k < kMaxCodebooks; ++k) {
      if (!e[k]) continue;
      float v[8];
      load8(e[k] + ch, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = first ? v[j] : acc[j] + v[j];
      first = false;
    }
    if (a.out) store8(a.out + row * C + ch, acc);
    if (a.out6) store_image8(a.out6, a.out_layout, row, C, ch, acc);
  }
}

hipError_t launch_gather_sum_rows(const GatherSumArgs& a, hipStream_t s) {
  if (!a.idx || a.rows < 0 || a.dim < 8 || a.dim % 8 || a.ncodes < 1 || a.R < 1 || a.R > kMaxCodebooks ||
      (!a.out && !a.out6) || (a.clip_len && (a.frames < 1 || a.rows % a.frames)))
    return hipErrorInvalidValue;
  for (int k = 0; k < a.R; ++k)
    if (!a.table[k]) return hipErrorInvalidValue;
  if (a.out6 && a.out_layout != LAYOUT_PLANES && a.out_layout != LAYOUT_BF16) return hipErrorInvalidValue;
  if (a.rows == 0) return hipSuccess;
  hipLaunchKernelGGL(gather_sum_rows_kernel, dim3((unsigned)((a.rows + 3) / 4)), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace dcx
