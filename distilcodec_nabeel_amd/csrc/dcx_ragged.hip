// Ragged (packed) batches on gfx950: the three steps of the encode path that know where a clip begins
// and ends, for clips of different lengths concatenated row-wise with no padding (RaggedSeg,
// dcx_kernels.h).  Everything else on that path (1x1 convs, LayerNorms, the VQ search) works on
// independent rows and runs unchanged on the sum of the clips' frames.
//  * ragged_frames: the STFT input, whole n_fft-sample frames of each clip's reflect-padded signal;
//  * ragged_unfold: the stem conv's input, each row followed by its neighbours of the same clip
//    (zeros beyond the clip's edges), so the k7 conv runs as a one-tap GEMM;
//  * dwconv_ln_seg / dwconv_ln_run_seg: the ConvNeXt block front (dcx_misc.hip dwconv_ln_kernel /
//    dwconv_ln_run_kernel, the same per-row arithmetic in the same order) with tiles and runs
//    enumerated per clip from the plan's prefix sums.
// All are streaming kernels with 16-byte accesses along the contiguous axis; a work item finds its
// clip by a binary search of a [batch + 1] prefix array (L2-resident, log2(batch) reads).
// The slot form (SL, dcx_tokenize_slots; RaggedSeg::n_dev): the padded layout, batch equal slots whose
// sample counts are read from device memory.  A work item finds its slot by a division, takes the
// slot's length L from n_dev and writes the rows from L to the slot's end as zeros; everything else is
// the packed form's code, so a slot's live rows get the arithmetic a clip of that length gets alone.
#include "dcx_kernels.h"
#include "dcx_planes.h"
#include "dcx_ln.h"

#include <algorithm>

namespace dcx {

// clip b with cu[b] <= i < cu[b + 1] (cu strictly increasing: every clip has at least one frame)
__device__ __forceinline__ int seg_find(const int* __restrict__ cu, int batch, int i) {
  int lo = 0, hi = batch;  // cu[lo] <= i < cu[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cu[mid] <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

// slot form: the slot's sample count (clamped) and the frames a clip of n samples has alone
// (dcx_num_frames(n + 1); none below the reflect pad's length, dcx_ragged_plan's rule)
__device__ __forceinline__ int slot_samples(const RaggedSeg& g, int b) { return min(max(g.n_dev[b], 0), g.slot_samples); }
__device__ __forceinline__ int slot_rows(const RaggedSeg& g, int n) {
  const int len = n + g.fr_extra;
  return n < g.fr_min || len < g.fr_nfft ? 0 : (len - g.fr_nfft) / g.fr_hop + 1;
}

// a dwconv_ln output row beyond its slot's length: zeros in every form (an h2 row with the shift and
// the maximum of a zero row), one wave per row as ln_finish
template <int NV>
__device__ __forceinline__ void ln_zero_row(int C, float* __restrict__ y, unsigned short* __restrict__ y6, Layout lay,
                                            long long row, int lane, int* __restrict__ ash_row,
                                            float* __restrict__ amax_row) {
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (lane + 64 * i) * 4;
    if (y) *reinterpret_cast<f32x4*>(y + row * C + c) = f32x4{0.f, 0.f, 0.f, 0.f};
    if (!y6) continue;
    if (lay == LAYOUT_BF16) store_bf16x4(y6, row, C, c, 0.f, 0.f, 0.f, 0.f);
    else if (lay == LAYOUT_H2) store_h2_4(y6, row, C, c, 0.f, 0.f, 0.f, 0.f);
    else store_planes4(y6, row, C, c, 0.f, 0.f, 0.f, 0.f);
  }
  if (y6 && lay == LAYOUT_H2 && lane == 0) {
    ash_row[row] = h2_shift(0.f);
    if (amax_row) amax_row[row] = 0.f;
  }
}

// ---------------------------------------------------------------------------------------------
// STFT framing.  Clip b's padded signal is [0, x_0 .. x_{n-1}] (the reference's one-sample left pad,
// distil_codec.py:133-136), reflect-padded by `pad` on both sides (mel_spec.py:30-37); frame t holds
// its samples t * hop - pad .. + n_fft - 1.  One thread writes 4 samples of one frame.
// ---------------------------------------------------------------------------------------------
template <bool SL>
__global__ void __launch_bounds__(256) ragged_frames_kernel(const float* __restrict__ audio, const RaggedSeg g,
                                                             float* __restrict__ frames,
                                                             unsigned short* __restrict__ frames6, int n_fft, int hop,
                                                             int pad) {
  const int per = n_fft / 4;
  const long long total4 = (long long)g.rows * per;
  for (long long i4 = (long long)blockIdx.x * blockDim.x + threadIdx.x; i4 < total4;
       i4 += (long long)gridDim.x * blockDim.x) {
    const int row = (int)(i4 / per), j = (int)(i4 - (long long)row * per) * 4;
    int b, t;
    long long s0, n;  // n: with the leading zero
    bool live = true;
    if constexpr (SL) {
      b = row / g.slot_frames;
      t = row - b * g.slot_frames;
      s0 = (long long)b * g.slot_samples;
      const int nb = slot_samples(g, b);
      n = (long long)nb + 1;
      live = t < slot_rows(g, nb);  // a row beyond the slot's length: zeros, nothing read
    } else {
      b = seg_find(g.cu_frames, g.batch, row);
      t = row - g.cu_frames[b];
      s0 = g.cu_samples[b];
      n = (long long)g.cu_samples[b + 1] - s0 + 1;
    }
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      long long src = (long long)t * hop + j + e - pad;
      if (src < 0) src = -src;
      if (src >= n) src = 2 * (n - 1) - src;
      v[e] = live && src > 0 ? audio[s0 + src - 1] : 0.f;
    }
    if (frames) *reinterpret_cast<f32x4*>(frames + (long long)row * n_fft + j) = f32x4{v[0], v[1], v[2], v[3]};
    if (frames6) store_planes4(frames6, row, n_fft, j, v[0], v[1], v[2], v[3]);
  }
}

hipError_t launch_ragged_frames(const float* audio, const RaggedSeg& g, float* frames, unsigned short* frames6,
                                int n_fft, int hop, int pad, hipStream_t s) {
  if (n_fft % 8 || g.rows < 1 || g.batch < 1) return hipErrorInvalidValue;
  const long long total4 = (long long)g.rows * (n_fft / 4);
  const unsigned gx = (unsigned)std::min<long long>((total4 + 255) / 256, 65536);
  if (g.n_dev)
    hipLaunchKernelGGL(ragged_frames_kernel<true>, dim3(gx), dim3(256), 0, s, audio, g, frames, frames6, n_fft, hop, pad);
  else
    hipLaunchKernelGGL(ragged_frames_kernel<false>, dim3(gx), dim3(256), 0, s, audio, g, frames, frames6, n_fft, hop, pad);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Segment-aware unfold.  One wave per output row: y[row][j] = x[row + j - taps / 2] where that row
// belongs to the same clip, else zeros (the conv's zero padding at the clip's own edges).  Rows move
// as 16-byte units whatever their layout.
// ---------------------------------------------------------------------------------------------
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

template <bool SL>
__global__ void __launch_bounds__(256) ragged_unfold_kernel(const u32x4* __restrict__ x, u32x4* __restrict__ y,
                                                             const RaggedSeg g, int units, int taps) {
  const int lane = threadIdx.x & 63;
  const int nwaves = gridDim.x * 4;
  for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < g.rows; row += nwaves) {  // wave-uniform
    int r0, r1;
    bool live = true;
    if constexpr (SL) {
      const int b = row / g.slot_frames;
      r0 = b * g.slot_frames;
      r1 = r0 + slot_rows(g, slot_samples(g, b));
      live = row < r1;  // a row beyond the slot's length: zeros
    } else {
      const int b = seg_find(g.cu_frames, g.batch, row);
      r0 = g.cu_frames[b], r1 = g.cu_frames[b + 1];
    }
    u32x4* dst = y + (long long)row * taps * units;
    for (int i = lane; i < taps * units; i += 64) {
      const int j = i / units, u = i - j * units;
      const int src = row + j - taps / 2;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (live && src >= r0 && src < r1) v = x[(long long)src * units + u];
      dst[i] = v;
    }
  }
}

hipError_t launch_ragged_unfold(const void* x, void* y, const RaggedSeg& g, int row_bytes, int taps, hipStream_t s) {
  if (row_bytes < 16 || row_bytes % 16 || taps < 1 || taps % 2 == 0 || g.rows < 1 || g.batch < 1)
    return hipErrorInvalidValue;
  const unsigned gx = (unsigned)std::min((g.rows + 3) / 4, 16384);
  if (g.n_dev)
    hipLaunchKernelGGL(ragged_unfold_kernel<true>, dim3(gx), dim3(256), 0, s, reinterpret_cast<const u32x4*>(x),
                       reinterpret_cast<u32x4*>(y), g, row_bytes / 16, taps);
  else
    hipLaunchKernelGGL(ragged_unfold_kernel<false>, dim3(gx), dim3(256), 0, s, reinterpret_cast<const u32x4*>(x),
                       reinterpret_cast<u32x4*>(y), g, row_bytes / 16, taps);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// dwconv_ln on a ragged batch, tiled form (launches below 8192 rows): dwconv_ln_kernel with the
// workgroup's tile looked up in cu_tiles (the clips' tile counts at DW_R rows per tile).  L is the
// tile's own clip's frame count, so the halo rows beyond the clip are staged as zeros and their taps
// dropped exactly as for a clip alone.
// ---------------------------------------------------------------------------------------------
template <int NV, int DW_R, bool SL>
__global__ void __launch_bounds__(256) dwconv_ln_seg_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                             unsigned short* __restrict__ y6, Layout lay,
                                                             const float* __restrict__ dww, const float* __restrict__ dwb,
                                                             const float* __restrict__ lnw, const float* __restrict__ lnb,
                                                             const RaggedSeg g, const int* __restrict__ cu_tiles, int bf,
                                                             int* ash_row, float* amax_row) {
  constexpr int C = 256 * NV, C4 = C / 4, ROWS = DW_R + 6;
  __shared__ f32x4 tile[ROWS * C4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int t0, L;
  long long base;
  if constexpr (SL) {  // the slot's tiles over its whole row count; L: the rows that hold data
    const int per = (g.slot_frames + DW_R - 1) / DW_R;
    const int bidx = (int)blockIdx.x / per;
    t0 = ((int)blockIdx.x - bidx * per) * DW_R;
    base = (long long)bidx * g.slot_frames;
    L = slot_rows(g, slot_samples(g, bidx));
    for (int rr = wave; rr < DW_R; rr += 4) {
      const int t = t0 + rr;
      if (t >= L && t < g.slot_frames) ln_zero_row<NV>(C, y, y6, lay, base + t, lane, ash_row, amax_row);
    }
    if (t0 >= L) return;  // wholly beyond the slot's length: before any load (and the block's barrier)
  } else {
    const int bidx = seg_find(cu_tiles, g.batch, (int)blockIdx.x);
    t0 = ((int)blockIdx.x - cu_tiles[bidx]) * DW_R;
    base = g.cu_frames[bidx];
    L = g.cu_frames[bidx + 1] - (int)base;
  }
  const float* xb = x + base * C;
  // stage rows t0 - 3 .. t0 + DW_R + 2 (all loads issued before any LDS store)
  constexpr int PER = (ROWS * C4 + 255) / 256;
  f32x4 st[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int i = threadIdx.x + k * 256;
    const int r = i / C4, c4 = i - r * C4;
    const int tt = t0 - 3 + r;
    const bool ok = i < ROWS * C4 && tt >= 0 && tt < L;
    st[k] = ok ? *reinterpret_cast<const f32x4*>(xb + (long long)tt * C + c4 * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    if (bf) st[k] = round_bf16x4(st[k]);
  }
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int i = threadIdx.x + k * 256;
    if (i < ROWS * C4) tile[i] = st[k];
  }
  f32x4 wv[NV][7], bv[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (lane + 64 * i) * 4;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      wv[i][j] = *reinterpret_cast<const f32x4*>(dww + j * C + c);
      if (bf) wv[i][j] = round_bf16x4(wv[i][j]);
    }
    bv[i] = *reinterpret_cast<const f32x4*>(dwb + c);
    if (bf) bv[i] = round_bf16x4(bv[i]);
  }
  __syncthreads();
  for (int rr = wave; rr < DW_R; rr += 4) {
    const int t = t0 + rr;
    if (t >= L) break;  // wave-uniform
    f32x4 v[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c4 = lane + 64 * i;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 7; ++j) {
        const int tt = t + j - 3;
        const f32x4 pr = tile[(rr + j) * C4 + c4] * wv[i][j];
        if (tt >= 0 && tt < L) acc += pr;
      }
      v[i] = acc + bv[i];
      if (bf) v[i] = round_bf16x4(v[i]);
    }
    const long long row = base + t;
    ln_finish<NV>(v, C, 1e-6f, 0, lnw, lnb, y ? y + row * C : nullptr, y6, lay, row, lane, ash_row, amax_row);
  }
}

// ---------------------------------------------------------------------------------------------
// Register-ring form (launches of >= 8192 rows): dwconv_ln_run_kernel with the wave's run looked up
// in cu_run; a run is RW consecutive rows of one clip (the last run of a clip may be shorter).
// ---------------------------------------------------------------------------------------------
template <int NV, int RW, int D, bool SL>
__global__ void __launch_bounds__(256) dwconv_ln_run_seg_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                 unsigned short* __restrict__ y6, Layout lay,
                                                                 const float* __restrict__ dww,
                                                                 const float* __restrict__ dwb,
                                                                 const float* __restrict__ lnw,
                                                                 const float* __restrict__ lnb, const RaggedSeg g, int bf,
                                                                 int* ash_row, float* amax_row) {
  constexpr int C = 256 * NV, C4 = C / 4, S = 7 + D;
  __shared__ f32x4 wsh[7 * C4];
  for (int i = threadIdx.x; i < 7 * C4; i += 256) {
    const f32x4 wv = reinterpret_cast<const f32x4*>(dww)[i];
    wsh[i] = bf ? round_bf16x4(wv) : wv;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int run = (int)blockIdx.x * 4 + wave;
  if (run >= g.n_run) return;  // whole wave, after the block's only barrier
  int t0, L;
  long long base;
  if constexpr (SL) {  // the slot's runs over its whole row count; L: the rows that hold data
    const int per = (g.slot_frames + RW - 1) / RW;
    const int bidx = run / per;
    t0 = (run - bidx * per) * RW;
    base = (long long)bidx * g.slot_frames;
    L = slot_rows(g, slot_samples(g, bidx));
    for (int t = max(t0, L); t < min(t0 + RW, g.slot_frames); ++t)
      ln_zero_row<NV>(C, y, y6, lay, base + t, lane, ash_row, amax_row);
    if (t0 >= L) return;  // wholly beyond the slot's length: before any load
  } else {
    const int bidx = seg_find(g.cu_run, g.batch, run);
    base = g.cu_frames[bidx];
    L = g.cu_frames[bidx + 1] - (int)base;
    t0 = (run - g.cu_run[bidx]) * RW;
  }
  const int t1 = min(t0 + RW, L);
  const float* xb = x + base * C;
  f32x4 win[S][NV], bv[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    bv[i] = *reinterpret_cast<const f32x4*>(dwb + (lane + 64 * i) * 4);
    if (bf) bv[i] = round_bf16x4(bv[i]);
  }
  auto load_row = [&](f32x4 (&dst)[NV], int tt) {  // row clamped into the clip: out-of-range taps are dropped below
    const float* src = xb + (long long)min(max(tt, 0), L - 1) * C;
#pragma unroll
    for (int i = 0; i < NV; ++i) dst[i] = *reinterpret_cast<const f32x4*>(src + (lane + 64 * i) * 4);
  };
  auto round_row = [&](f32x4 (&r)[NV]) {
#pragma unroll
    for (int i = 0; i < NV; ++i) r[i] = round_bf16x4(r[i]);
  };
  // rows t0 - 3 .. t0 + 2 + D in slots 0 .. 5 + D (row r in slot (r - t0 + 3) mod S)
#pragma unroll
  for (int k = 0; k < 6 + D; ++k) load_row(win[k], t0 - 3 + k);
  if (bf) {
#pragma unroll
    for (int k = 0; k < 6; ++k) round_row(win[k]);
  }
  for (int t = t0;; t += S) {
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const int tk = t + k;
      if (tk >= t1) return;  // wave-uniform
      if (bf) round_row(win[(k + 6) % S]);  // row tk + 3, first used now
      if (tk + 3 + D < t1 + 3) load_row(win[(k + S - 1) % S], tk + 3 + D);  // into row tk - 4's slot
      f32x4 v[NV];
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c4 = lane + 64 * i;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 7; ++j) {
          const int tt = tk + j - 3;
          const f32x4 pr = win[(k + j) % S][i] * wsh[j * C4 + c4];
          if (tt >= 0 && tt < L) acc += pr;
        }
        v[i] = acc + bv[i];
        if (bf) v[i] = round_bf16x4(v[i]);
      }
      const long long row = base + tk;
      ln_finish<NV>(v, C, 1e-6f, 0, lnw, lnb, y ? y + row * C : nullptr, y6, lay, row, lane, ash_row, amax_row);
    }
  }
}

#define DCX_RAGGED_ARGS x, y, y6, lay, dww, dwb, lnw, lnb, g

template <int NV>
static void launch_run_seg_nv(const float* x, float* y, unsigned short* y6, Layout lay, const float* dww, const float* dwb,
                              const float* lnw, const float* lnb, const RaggedSeg& g, int bf, hipStream_t s,
                              int* ash_row, float* amax_row) {
  const dim3 grid((unsigned)((g.n_run + 3) / 4)), block(256);
  constexpr int D = NV >= 4 ? 1 : 2;  // as launch_dwconv_ln_nv
#define DCX_RUN_SEG(RW)                                                                                                   \
  if (g.n_dev)                                                                                                           \
    hipLaunchKernelGGL((dwconv_ln_run_seg_kernel<NV, RW, D, true>), grid, block, 0, s, DCX_RAGGED_ARGS, bf, ash_row, amax_row); \
  else                                                                                                                   \
    hipLaunchKernelGGL((dwconv_ln_run_seg_kernel<NV, RW, D, false>), grid, block, 0, s, DCX_RAGGED_ARGS, bf, ash_row, amax_row)
  switch (g.rw) {
    case 32: DCX_RUN_SEG(32); break;
    case 16: DCX_RUN_SEG(16); break;
    case 8: DCX_RUN_SEG(8); break;
    default: DCX_RUN_SEG(4); break;
  }
#undef DCX_RUN_SEG
}

template <int NV>
static void launch_tiled_seg_nv(const float* x, float* y, unsigned short* y6, Layout lay, const float* dww,
                                const float* dwb, const float* lnw, const float* lnb, const RaggedSeg& g, bool small,
                                int bf, hipStream_t s, int* ash_row, float* amax_row) {
  const dim3 block(256);
  if (g.n_dev) {
    if (small)
      hipLaunchKernelGGL((dwconv_ln_seg_kernel<NV, 4, true>), dim3((unsigned)g.n_t4), block, 0, s, DCX_RAGGED_ARGS, nullptr, bf, ash_row, amax_row);
    else
      hipLaunchKernelGGL((dwconv_ln_seg_kernel<NV, 16, true>), dim3((unsigned)g.n_t16), block, 0, s, DCX_RAGGED_ARGS, nullptr, bf, ash_row, amax_row);
  } else if (small) {
    hipLaunchKernelGGL((dwconv_ln_seg_kernel<NV, 4, false>), dim3((unsigned)g.n_t4), block, 0, s, DCX_RAGGED_ARGS, g.cu_t4, bf, ash_row, amax_row);
  } else {
    hipLaunchKernelGGL((dwconv_ln_seg_kernel<NV, 16, false>), dim3((unsigned)g.n_t16), block, 0, s, DCX_RAGGED_ARGS, g.cu_t16, bf, ash_row, amax_row);
  }
}

hipError_t launch_dwconv_ln_ragged(const float* x, float* y, unsigned short* y6, Layout lay, const float* dww,
                                   const float* dwb, const float* lnw, const float* lnb, const RaggedSeg& g, int C,
                                   int bf16, const Knobs* kn, hipStream_t s, int* ash_row, float* amax_row) {
  if (y6 && lay == LAYOUT_H2 && !ash_row) return hipErrorInvalidValue;
  if (g.batch < 1 || g.rows < 1 || g.n_t16 < 1 || g.n_t4 < 1 || g.n_run < 1) return hipErrorInvalidValue;
  const bool tiled = kn && kn->dwconv_tiled;
  // launch_dwconv_ln's thresholds: the register-ring runs from 8192 rows on, 4-row tiles while 16-row
  // tiles would leave most CUs idle
  if (!tiled && g.rows >= 8192) {
    if (g.rw != dwconv_run_rows(g.rows)) return hipErrorInvalidValue;
    switch (C) {
      case 256: launch_run_seg_nv<1>(DCX_RAGGED_ARGS, bf16, s, ash_row, amax_row); break;
      case 512: launch_run_seg_nv<2>(DCX_RAGGED_ARGS, bf16, s, ash_row, amax_row); break;
      case 768: launch_run_seg_nv<3>(DCX_RAGGED_ARGS, bf16, s, ash_row, amax_row); break;
      case 1024: launch_run_seg_nv<4>(DCX_RAGGED_ARGS, bf16, s, ash_row, amax_row); break;
      default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
  }
  const bool small = g.n_t16 < 512;
  switch (C) {
    case 256: launch_tiled_seg_nv<1>(DCX_RAGGED_ARGS, small, bf16, s, ash_row, amax_row); break;
    case 512: launch_tiled_seg_nv<2>(DCX_RAGGED_ARGS, small, bf16, s, ash_row, amax_row); break;
    case 768: launch_tiled_seg_nv<3>(DCX_RAGGED_ARGS, small, bf16, s, ash_row, amax_row); break;
    case 1024: launch_tiled_seg_nv<4>(DCX_RAGGED_ARGS, small, bf16, s, ash_row, amax_row); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

#undef DCX_RAGGED_ARGS

// ---------------------------------------------------------------------------------------------
// The slot form's results beyond each slot's length: codes -1, x_pjt_in rows zero (the row-wise steps
// ran on those rows too).  One wave per row; a live row is left as it is.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) slots_mask_kernel(const RaggedSeg g, int32_t* __restrict__ codes, int R,
                                                          float* __restrict__ pin, int dim) {
  const int lane = threadIdx.x & 63;
  const int nwaves = gridDim.x * 4;
  for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < g.rows; row += nwaves) {  // wave-uniform
    const int b = row / g.slot_frames;
    if (row - b * g.slot_frames < slot_rows(g, slot_samples(g, b))) continue;
    for (int r = lane; r < R; r += 64) codes[(long long)row * R + r] = -1;
    if (pin)
      for (int c = lane * 4; c < dim; c += 256)
        *reinterpret_cast<f32x4*>(pin + (long long)row * dim + c) = f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

hipError_t launch_slots_mask(const RaggedSeg& g, int32_t* codes, int R, float* pin, int dim, hipStream_t s) {
  if (!g.n_dev || !codes || g.rows < 1 || g.slot_frames < 1 || R < 1 || dim < 4 || dim % 4) return hipErrorInvalidValue;
  const unsigned gx = (unsigned)std::min((g.rows + 3) / 4, 16384);
  hipLaunchKernelGGL(slots_mask_kernel, dim3(gx), dim3(256), 0, s, g, codes, R, pin, dim);
  return hipGetLastError();
}

}  // namespace dcx
