// Microbenchmark: bytes per cycle per CU that LDS-DMA (buffer_load ... lds, 1 KiB per wave
// instruction) takes in, by the shape of the piece's source.  One 512-thread workgroup per CU, all
// eight waves issuing pieces into a 64 KiB LDS ring (8 pieces per wave and group, at most two groups
// in flight per wave), alone and with 96 v_mfma_f32_16x16x32_f16 per wave between groups.  Shapes:
//   a  64 lanes x 16 B at 128 B stride   (an h3 weight piece of the column-major layout)
//   b  64 lanes x 16 B at 2 KiB stride   (an h3 activation piece at C = 512)
//   c  1 KiB contiguous
//   d  8 rows x 128 B at 2 KiB stride
//   e  16 runs x 64 B at 128 B stride
//   f  d's 8 rows x 128 B, rows fastest over the lanes: lane j takes piece j >> 3 of row j & 7
//   g  d with the 8 pieces of a row XOR-permuted: lane j takes piece (j & 7) ^ (((r >> 1) & 3) << 1) of row r = j >> 3
//      (f and g: the two lane orders of conv_gemm_x3dw's activation image, csrc/dcx_a3_layout.h; a
//      piece q = plane * 4 + channel group lies at (q & 3) * 32 + (q >> 2) * 16 of the row's 128 B)
// In every shape consecutive pieces of a wave walk one block (a: the 8 pieces of 64 columns, b: the
// 128 of 64 rows, d, f, g: the 16 of 8 rows, e: the 2 of 16 runs), so each covers the buffer once per
// sweep.  The buffer is 2 MiB (resident in every XCD's L2; every workgroup reads all of it) or
// 2 GiB (streamed: every byte is read once per run).  It only measures: every offset is taken modulo the buffer's size, under a
// descriptor of exactly that size, and the iteration count is fixed.
// Build: hipcc -O3 --offload-arch=gfx950 dma_shape.hip -o dma_shape
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <vector>
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;

constexpr int kGroup = 8;        // pieces per wave and group
constexpr int kRing = 64 * 1024;  // bytes

#define CHECK(x)                                                                     \
  do {                                                                               \
    hipError_t e_ = (x);                                                             \
    if (e_ != hipSuccess) {                                                          \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                        \
      return 1;                                                                      \
    }                                                                                \
  } while (0)

// lane part and (wave-uniform) piece part of the source offset of piece P
__device__ __forceinline__ unsigned h2_piece(int q) { return (q & 3) * 32 + (q >> 2) * 16; }
template <int SHAPE>
__device__ __forceinline__ unsigned lane_off(int lane) {
  if constexpr (SHAPE == 0) return lane * 128;
  else if constexpr (SHAPE == 1) return lane * 2048;
  else if constexpr (SHAPE == 2) return lane * 16;
  else if constexpr (SHAPE == 3) return (lane >> 3) * 2048 + (lane & 7) * 16;
  else if constexpr (SHAPE == 4) return (lane >> 2) * 128 + (lane & 3) * 16;
  else if constexpr (SHAPE == 5) return (lane & 7) * 2048 + h2_piece(lane >> 3);
  else return (lane >> 3) * 2048 + h2_piece((lane & 7) ^ (((lane >> 4) & 3) << 1));
}
template <int SHAPE>
__device__ __forceinline__ unsigned piece_off(unsigned P) {
  if constexpr (SHAPE == 0) return (P >> 3) * 8192 + (P & 3) * 32 + ((P >> 2) & 1) * 16;
  else if constexpr (SHAPE == 1) return (P >> 7) * 131072 + (P & 127) * 16;
  else if constexpr (SHAPE == 2) return P * 1024;
  else if constexpr (SHAPE == 3 || SHAPE >= 5) return (P >> 4) * 16384 + (P & 15) * 128;
  else return (P >> 1) * 2048 + (P & 1) * 64;
}

// LDS: the ring, and as much again unused so that a CU holds one workgroup
template <int SHAPE, bool MFMA>
__global__ void __launch_bounds__(512, 1) k(const char* buf, unsigned bytes, int iters, float* out, unsigned long long* cyc) {
  __shared__ __attribute__((aligned(16))) char lds[kRing + 32 * 1024];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void*)buf, 0, bytes, 0x00020000);
  const unsigned np_mask = bytes / 1024 - 1;  // pieces in the buffer (a power of two) - 1
  const unsigned voff = lane_off<SHAPE>(lane);
  // this wave's first piece: workgroups and waves start a sweep apart
  unsigned P = (blockIdx.x * 8 + wave) * (unsigned)iters * kGroup;
  f16x8 a8, b8;
  for (int i = 0; i < 8; ++i) { a8[i] = (_Float16)(0.001f * (lane + i)); b8[i] = (_Float16)(0.002f * (lane - i)); }
  f32x4 acc[4] = {};
  char* const dst = lds + wave * kGroup * 1024;
  __syncthreads();
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int it = 0; it < iters; ++it) {
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");  // the group before the last has landed
#pragma unroll
    for (int i = 0; i < kGroup; ++i) {
      const unsigned soff = piece_off<SHAPE>((P + i) & np_mask);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_ptr_t)(dst + i * 1024), 16, voff, soff, 0, 0);
    }
    P += kGroup;
    if constexpr (MFMA) {
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int u = 0; u < 96; ++u) acc[u & 3] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a8, b8, acc[u & 3], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  // keep the MFMAs and the ring alive
  out[blockIdx.x * 512 + threadIdx.x] = acc[0][0] + acc[1][1] + acc[2][2] + acc[3][3] + (float)lds[threadIdx.x * 16];
  if (threadIdx.x == 0) cyc[blockIdx.x] = t1 - t0;
}

typedef void (*kern_t)(const char*, unsigned, int, float*, unsigned long long*);

int main() {
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  const int cus = prop.multiProcessorCount;
  const size_t big = 2048ull << 20, small = 2ull << 20;  // big = cus * 8 waves * iters * 8 KiB at 256 CUs
  char* buf;
  float* out;
  unsigned long long* cyc;
  CHECK(hipMalloc(&buf, big));
  CHECK(hipMemset(buf, 1, big));
  CHECK(hipMalloc(&out, (size_t)cus * 512 * sizeof(float)));
  CHECK(hipMalloc(&cyc, (size_t)cus * sizeof(unsigned long long)));
  constexpr int kShapes = 7;
  const kern_t kerns[2][kShapes] = {{k<0, false>, k<1, false>, k<2, false>, k<3, false>, k<4, false>, k<5, false>, k<6, false>},
                                    {k<0, true>, k<1, true>, k<2, true>, k<3, true>, k<4, true>, k<5, true>, k<6, true>}};
  const char* names[kShapes] = {"a 64 x 16 B / 128 B", "b 64 x 16 B / 2 KiB", "c 1 KiB contiguous", "d 8 x 128 B / 2 KiB",
                                "e 16 x 64 B / 128 B", "f d, rows fastest", "g d, pieces XOR-ed"};
  const int iters = 128, reps = 7;  // 8 MiB per CU and run
  std::vector<unsigned long long> hc(cus);
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  printf("%d CUs, one 512-thread workgroup each, %d groups of %d pieces per wave; %d runs per line\n", cus, iters, kGroup, reps);
  printf("B/cycle/CU: bytes per shader-clock cycle of the workgroup, median over the CUs; GB/s/CU from the launch's wall time\n");
  printf("%-8s %-5s %-22s %8s %8s %8s   %8s %8s\n", "buffer", "mfma", "shape", "B/c min", "B/c med", "B/c max", "GB/s med", "cyc/grp");
  for (int sz = 0; sz < 2; ++sz)
    for (int mf = 0; mf < 2; ++mf)
      for (int sh = 0; sh < kShapes; ++sh) {
        const unsigned bytes = (unsigned)(sz ? big : small);
        std::vector<double> bpc, gbs;
        for (int rep = -1; rep < reps; ++rep) {  // run -1 warms up
          CHECK(hipEventRecord(e0));
          hipLaunchKernelGGL(kerns[mf][sh], dim3(cus), dim3(512), 0, 0, buf, bytes, iters, out, cyc);
          CHECK(hipEventRecord(e1));
          CHECK(hipEventSynchronize(e1));
          CHECK(hipGetLastError());
          float ms;
          CHECK(hipEventElapsedTime(&ms, e0, e1));
          CHECK(hipMemcpy(hc.data(), cyc, (size_t)cus * sizeof(unsigned long long), hipMemcpyDeviceToHost));
          if (rep < 0) continue;
          std::sort(hc.begin(), hc.end());
          const double per_cu = 8.0 * iters * kGroup * 1024;
          bpc.push_back(per_cu / (double)hc[cus / 2]);
          gbs.push_back(per_cu / (ms * 1e-3) / 1e9);
        }
        std::sort(bpc.begin(), bpc.end());
        std::sort(gbs.begin(), gbs.end());
        printf("%-8s %-5s %-22s %8.2f %8.2f %8.2f   %8.1f %8.0f\n", sz ? "2 GiB" : "2 MiB", mf ? "96" : "-", names[sh],
               bpc.front(), bpc[reps / 2], bpc.back(), gbs[reps / 2], 8.0 * kGroup * 1024 / bpc[reps / 2]);
        fflush(stdout);
      }
  return 0;
}
