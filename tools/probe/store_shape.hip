// Microbenchmark: bytes per ns per CU that plain global stores (16 B per lane, 1 KiB per wave
// instruction) drain at, by the shape of the instruction's footprint.  One 512-thread workgroup per
// CU, as a conv_gemm_x3dw tile; every wave walks 4 KiB blocks of its own with four instructions per
// block, so every shape writes every byte of the buffer exactly once.  Shapes (offsets in a block):
//   a   lane j writes 16 B at 32 j, a second instruction the other halves: 2 KiB touched and half
//       filled per instruction (epilogue_form's 8-channel groups at BN = 256)
//   b   1 KiB contiguous per instruction (4-channel groups: a wave covers 256 channels of a row)
//   c0  a's 32-byte lane stride on rows of 512 B that lie 1 KiB apart: four half-filled 512-byte runs
//       per instruction (BN = 128 under a ConvT with out_mul 2)
//   c   two whole 512-byte runs 1 KiB apart per instruction (b's lanes on those rows)
// and, for a and b, the c2 mix: one load stream and two store streams of the same shape (the loaded
// values are what is stored; the next block's loads are issued ahead of this block's stores).
// A run is 4 MiB per CU and stream in bursts of 256 KiB (one 256 x 256 fp32 tile), each ended by
// vmcnt(0) and a barrier, or in one burst; with every CU active (1 GiB per stream, beyond L2 and the
// 256 MiB last-level cache) or with one CU in five.  It only measures: every offset lies inside the
// stream's region by construction (block index < blocks per region, lane offset < 4 KiB), and the
// iteration counts are fixed.
// Build: hipcc -O3 --offload-arch=gfx950 store_shape.hip -o store_shape
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kBlock = 4096;                   // bytes per wave and iteration (4 instructions)
constexpr int kIters = 128;                    // per wave: 8 waves x 128 x 4 KiB = 4 MiB per CU and stream
constexpr size_t kPerCu = 8ull * kIters * kBlock;

#define CHECK(x)                                              \
  do {                                                        \
    hipError_t e_ = (x);                                      \
    if (e_ != hipSuccess) {                                   \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); \
      return 1;                                               \
    }                                                         \
  } while (0)

// byte offset of lane `lane` in instruction n (0 .. 3) of a block
template <int SHAPE>
__host__ __device__ constexpr unsigned lane_off(int n, int lane) {
  if constexpr (SHAPE == 0) return (n >> 1) * 2048 + lane * 32 + (n & 1) * 16;
  else if constexpr (SHAPE == 1) return n * 1024 + lane * 16;
  else if constexpr (SHAPE == 2) return (lane >> 4) * 1024 + (n >> 1) * 512 + (lane & 15) * 32 + (n & 1) * 16;
  else return ((n & 1) * 2 + (lane >> 5)) * 1024 + (n >> 1) * 512 + (lane & 31) * 16;
}

// LDS: more than half a CU's, so that a CU holds one workgroup
template <int SHAPE, bool MIX>
__global__ void __launch_bounds__(512, 1) k(const char* ld, char* st0, char* st1, const f32x4* seed, int burst, int every,
                                            unsigned long long* ticks, float* sink) {
  __shared__ __attribute__((aligned(16))) char lds[96 * 1024];
  if (blockIdx.x % every) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t base = (size_t)blockIdx.x * kPerCu;
  f32x4 v[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) v[n] = seed[(threadIdx.x * 4 + n) & 4095];
  auto load = [&](int it, f32x4(&x)[4]) {
    const size_t o = base + ((size_t)it * 8 + wave) * kBlock;
#pragma unroll
    for (int n = 0; n < 4; ++n) x[n] = *reinterpret_cast<const f32x4*>(ld + o + lane_off<SHAPE>(n, lane));
  };
  lds[threadIdx.x] = 0;
  __syncthreads();
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  if constexpr (MIX) load(0, v);
  for (int it = 0; it < kIters; ++it) {
    const size_t o = base + ((size_t)it * 8 + wave) * kBlock;
    f32x4 nx[4];
    if constexpr (MIX) load(min(it + 1, kIters - 1), nx);
#pragma unroll
    for (int n = 0; n < 4; ++n) *reinterpret_cast<f32x4*>(st0 + o + lane_off<SHAPE>(n, lane)) = v[n];
    if constexpr (MIX) {
#pragma unroll
      for (int n = 0; n < 4; ++n) *reinterpret_cast<f32x4*>(st1 + o + lane_off<SHAPE>(n, lane)) = v[n];
#pragma unroll
      for (int n = 0; n < 4; ++n) v[n] = nx[n];
    }
    if ((it + 1) % burst == 0) {  // the end of a tile's epilogue: drained, then the workgroup meets
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
  if (threadIdx.x == 0) ticks[blockIdx.x] = t1 - t0;
  if (v[0][0] == 1.2345e-33f) sink[0] = (float)lds[threadIdx.x];
}

__global__ void fill(unsigned* p, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    unsigned x = (unsigned)i * 2654435761u + (unsigned)(i >> 32);
    x ^= x >> 15, x *= 2246822519u, x ^= x >> 13;
    p[i] = (x & 0x3fffffffu) | 0x20000000u;  // finite floats of mixed magnitude and sign-free
  }
}

typedef void (*kern_t)(const char*, char*, char*, const f32x4*, int, int, unsigned long long*, float*);

int main() {
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  const int cus = prop.multiProcessorCount;
  const size_t region = (size_t)cus * kPerCu;
  char* buf;
  f32x4* seed;
  float* sink;
  unsigned long long* ticks;
  CHECK(hipMalloc(&buf, 3 * region));
  CHECK(hipMalloc(&seed, 4096 * sizeof(f32x4)));
  CHECK(hipMalloc(&sink, sizeof(float)));
  CHECK(hipMalloc(&ticks, (size_t)cus * sizeof(unsigned long long)));
  hipLaunchKernelGGL(fill, dim3(4096), dim3(256), 0, 0, (unsigned*)buf, 3 * region / 4);
  hipLaunchKernelGGL(fill, dim3(16), dim3(256), 0, 0, (unsigned*)seed, 4096 * 4);
  CHECK(hipDeviceSynchronize());
  constexpr int kKern = 6;
  const kern_t kerns[kKern] = {k<0, false>, k<1, false>, k<2, false>, k<3, false>, k<0, true>, k<1, true>};
  const char* names[kKern] = {"a  16 B at 32 j, halves", "b  1 KiB contiguous",     "c0 4 x 512 B half-filled",
                              "c  2 x 512 B whole",      "d  mix 1 ld + 2 st of a", "d  mix 1 ld + 2 st of b"};
  const int streams[kKern] = {1, 1, 1, 1, 3, 3};
  const int reps = 7;
  std::vector<unsigned long long> ht(cus);
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  printf("%d CUs, one 512-thread workgroup per active CU, %zu KiB per CU and stream; median of %d runs (min-max)\n", cus,
         kPerCu >> 10, reps);
  printf("B/ns/CU: bytes moved (loads + stores) per ns of the workgroup (100 MHz stamps around all bursts and the last\n"
         "drain), median over the active CUs; GB/s: all bytes over the launch's wall time\n");
  printf("%-8s %-9s %-26s %22s %10s\n", "active", "burst", "shape", "B/ns/CU med (min-max)", "GB/s med");
  for (int every : {1, 5})
    for (int burst : {8, kIters})
      for (int kn = 0; kn < kKern; ++kn) {
        std::vector<double> bpn, gbs;
        for (int rep = -1; rep < reps; ++rep) {  // run -1 warms up
          CHECK(hipMemset(ticks, 0, (size_t)cus * sizeof(unsigned long long)));
          CHECK(hipEventRecord(e0));
          hipLaunchKernelGGL(kerns[kn], dim3(cus), dim3(512), 0, 0, buf, buf + region, buf + 2 * region, seed, burst, every,
                             ticks, sink);
          CHECK(hipEventRecord(e1));
          CHECK(hipEventSynchronize(e1));
          CHECK(hipGetLastError());
          float ms;
          CHECK(hipEventElapsedTime(&ms, e0, e1));
          CHECK(hipMemcpy(ht.data(), ticks, (size_t)cus * sizeof(unsigned long long), hipMemcpyDeviceToHost));
          if (rep < 0) continue;
          std::vector<unsigned long long> act;
          for (int i = 0; i < cus; i += every) act.push_back(ht[i]);
          std::sort(act.begin(), act.end());
          const double per_cu = (double)streams[kn] * kPerCu;
          bpn.push_back(per_cu / ((double)act[act.size() / 2] * 10.0));
          gbs.push_back(per_cu * act.size() / (ms * 1e-3) / 1e9);
        }
        std::sort(bpn.begin(), bpn.end());
        std::sort(gbs.begin(), gbs.end());
        printf("%-8s %-9s %-26s %8.2f (%5.2f-%5.2f) %10.1f\n", every == 1 ? "all" : "1 in 5", burst == 8 ? "256 KiB" : "4 MiB",
               names[kn], bpn[reps / 2], bpn.front(), bpn.back(), gbs[reps / 2]);
        fflush(stdout);
      }
  return 0;
}
