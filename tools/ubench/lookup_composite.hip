// Microbenchmark (gate of the composite final step of the IB check and variable chains): chains of LEN dependent
// 4-bit table steps (5, the check body's shape, or 7, the degree-8 variable body's), served by the LDS, in three forms. The table image has lookup_rate.hip's addresses, the decoders'
// quad layout (row e = t*16+m of 128 bytes, one dword per bank, 32 KiB at LDS byte 0); the composite
// C(t, m)[y] = tab(tab(t, m), y), 16 nibbles = 8 bytes per entry, 32 lane copies, stands in one 64-KiB
// super-region at LDS byte 65536.
//   a  LEN ds_read_u8 steps (today's chain)
//   b  LEN-2 ds_read_u8 steps, then ds_read_b64 at (t<<12)|(m<<8)|8*(lane&31), v_lshrrev_b64 by 4y, v_and 15
//   c  LEN-2 ds_read_u8 steps, then ds_read_b32 at (t<<12)|(m<<8)|(y>>3)<<7|4*(lane&31), v_bfe_u32 at 4(y&7)
// m and y are shared by a lane's chains, as a codeword's inputs are shared by the chains of a check.
// Prints one JSON line for 8 and for 16 chains per wave-lane: LEN-step chains per clock per CU at the nominal
// 2.4 GHz (16 waves per CU, one block per CU). Every launch's result is checked against the host's chain.
// build: hipcc --offload-arch=gfx950 -O3 -o lookup_composite lookup_composite.hip
// run:   lookup_composite a | b | c [5 | 7]    (one form per process; the chain length defaults to 5)
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

typedef __attribute__((address_space(3))) const uint8_t lds8_t;
typedef __attribute__((address_space(3))) const uint32_t lds32_t;
typedef __attribute__((address_space(3))) const uint64_t lds64_t;

constexpr uint32_t kCompBase = 65536, kLdsBytes = 131072;

__host__ __device__ inline uint32_t tab(uint32_t e) { return (e * 13 + 5) & 15; }
__host__ __device__ inline uint32_t first_m(uint32_t thread, uint32_t block) { return (thread * 7 + block) & 15; }

template <int FORM, int NC, int LEN>
__global__ __launch_bounds__(1024) void chains(const uint32_t* __restrict__ img, const uint32_t* __restrict__ cimg,
                                                int iters, uint32_t* out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  uint32_t* l32 = reinterpret_cast<uint32_t*>(lds);
  for (int i = threadIdx.x; i < 8192; i += blockDim.x) l32[i] = img[i >> 5];
  if (FORM != 0)   // entry e = 64 dwords: b, lane l owns dwords 2l and 2l+1; c, dwords 0..31 the low half, 32..63 the high
    for (int i = threadIdx.x; i < 16384; i += blockDim.x) {
      const int e = i >> 6, w = i & 63;
      l32[kCompBase / 4 + i] = FORM == 1 ? cimg[2 * e + (w & 1)] : cimg[2 * e + (w >> 5)];
    }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const uint32_t lane4 = (uint32_t)(lane & 31) << 2;
  uint32_t tl[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) tl[k] = (lane + k) & 15;
  uint32_t m = first_m(threadIdx.x, blockIdx.x);
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int s = 0; s < (FORM == 0 ? LEN : LEN - 2); ++s) {
      m = (m + 5) & 15;
      const uint32_t mt = (m << 7) | lane4;
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        uint32_t x;
        asm("v_lshl_or_b32 %0, %1, 11, %2" : "=v"(x) : "v"(tl[k]), "v"(mt));
        tl[k] = *(lds8_t*)(size_t)x;
      }
    }
    if (FORM != 0) {
      const uint32_t mm = (m + 5) & 15, y = (m + 10) & 15;
      m = y;
      if (FORM == 1) {
        const uint32_t ct = (mm << 8) | (lane4 << 1) | kCompBase, sh = y << 2;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
          uint32_t x;
          asm("v_lshl_or_b32 %0, %1, 12, %2" : "=v"(x) : "v"(tl[k]), "v"(ct));
          const uint64_t v = *(lds64_t*)(size_t)x;
          uint64_t r;
          asm("v_lshrrev_b64 %0, %1, %2" : "=v"(r) : "v"(sh), "v"(v));
          tl[k] = (uint32_t)r & 15u;
        }
      } else {
        const uint32_t ct = (mm << 8) | ((y >> 3) << 7) | lane4 | kCompBase, sh = (y & 7) << 2;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
          uint32_t x;
          asm("v_lshl_or_b32 %0, %1, 12, %2" : "=v"(x) : "v"(tl[k]), "v"(ct));
          const uint32_t v = *(lds32_t*)(size_t)x;
          asm("v_bfe_u32 %0, %1, %2, 4" : "=v"(tl[k]) : "v"(v), "v"(sh));
        }
      }
    }
  }
  uint32_t acc = 0;
#pragma unroll
  for (int k = 0; k < NC; ++k) acc = acc * 3 + tl[k];
  out[blockIdx.x * blockDim.x + threadIdx.x] = acc;
}

static uint32_t host_chain(int nc, int len, uint32_t thread, uint32_t block, int iters) {
  const uint32_t lane = thread & 63;
  uint32_t m = first_m(thread, block), acc = 0;
  std::vector<uint32_t> t(nc);
  for (int k = 0; k < nc; ++k) t[k] = (lane + k) & 15;
  for (int s = 0; s < len * iters; ++s) {
    m = (m + 5) & 15;
    for (int k = 0; k < nc; ++k) t[k] = tab(t[k] * 16 + m);
  }
  for (int k = 0; k < nc; ++k) acc = acc * 3 + t[k];
  return acc;
}

#define CHECK(x)                                                                   \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess) {                                                        \
      fprintf(stderr, "%s: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__);  \
      return 2;                                                                    \
    }                                                                              \
  } while (0)

template <int FORM, int NC, int LEN>
int run(const uint32_t* img, const uint32_t* cimg, uint32_t* out, int ncu) {
  const int iters = 1024, check_iters = 3, block = 1024, grid = ncu, reps = 5;
  auto k = chains<FORM, NC, LEN>;
  CHECK(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));
  std::vector<uint32_t> h((size_t)grid * block);
  hipLaunchKernelGGL(k, dim3(grid), dim3(block), kLdsBytes, 0, img, cimg, check_iters, out);
  CHECK(hipGetLastError());
  CHECK(hipMemcpy(h.data(), out, h.size() * 4, hipMemcpyDeviceToHost));
  size_t bad = 0;
  for (int b = 0; b < grid; ++b)
    for (int t = 0; t < block; ++t) bad += h[(size_t)b * block + t] != host_chain(NC, LEN, t, b, check_iters);
  hipEvent_t a, b;
  CHECK(hipEventCreate(&a));
  CHECK(hipEventCreate(&b));
  float ms[reps];
  for (int r = 0; r < reps; ++r) {
    CHECK(hipEventRecord(a));
    hipLaunchKernelGGL(k, dim3(grid), dim3(block), kLdsBytes, 0, img, cimg, iters, out);
    CHECK(hipEventRecord(b));
    CHECK(hipEventSynchronize(b));
    CHECK(hipEventElapsedTime(&ms[r], a, b));
  }
  std::sort(ms, ms + reps);
  const double chains = (double)grid * block * iters * NC;
  const double per = chains / (ms[reps / 2] * 1e-3) / (ncu * 2.4e9);
  const int reads = FORM == 0 ? LEN : LEN - 1;
  printf("{\"form\": \"%c\", \"steps\": %d, \"chains_per_lane\": %d, \"cus\": %d, \"ms_median\": %.4f, \"ms_min\": %.4f, "
         "\"ms_max\": %.4f, \"chains_per_clk_per_cu\": %.3f, \"lds_reads_per_clk_per_cu\": %.2f, "
         "\"mismatches\": %zu}\n",
         "abc"[FORM], LEN, NC, ncu, ms[reps / 2], ms[0], ms[reps - 1], per, per * reads, bad);
  return bad ? 1 : 0;
}

template <int FORM, int LEN>
int run_len(const uint32_t* img, const uint32_t* cimg, uint32_t* out, int ncu) {
  const int r8 = run<FORM, 8, LEN>(img, cimg, out, ncu);
  if (r8 == 2) return 2;
  const int r16 = run<FORM, 16, LEN>(img, cimg, out, ncu);
  return r8 | r16;
}

template <int FORM>
int run_form(int len, const uint32_t* img, const uint32_t* cimg, uint32_t* out, int ncu) {
  return len == 7 ? run_len<FORM, 7>(img, cimg, out, ncu) : run_len<FORM, 5>(img, cimg, out, ncu);
}

int main(int argc, char** argv) {
  const int len = argc == 3 ? atoi(argv[2]) : 5;
  if (argc < 2 || argc > 3 || strlen(argv[1]) != 1 || !strchr("abc", argv[1][0]) || (len != 5 && len != 7)) {
    fprintf(stderr, "usage: %s a|b|c [5|7]\n", argv[0]);
    return 2;
  }
  int ncu = 0;
  CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, 0));
  std::vector<uint32_t> hi(256), hc(512, 0);
  for (int e = 0; e < 256; ++e) {
    hi[e] = tab(e) * 0x01010101u;
    for (int y = 0; y < 16; ++y) hc[2 * e + (y >> 3)] |= tab(tab(e) * 16 + y) << (4 * (y & 7));
  }
  uint32_t *img, *cimg, *out;
  CHECK(hipMalloc(&img, 1024));
  CHECK(hipMalloc(&cimg, 2048));
  CHECK(hipMalloc(&out, (size_t)ncu * 1024 * 4));
  CHECK(hipMemcpy(img, hi.data(), 1024, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(cimg, hc.data(), 2048, hipMemcpyHostToDevice));
  switch (argv[1][0]) {
    case 'a': return run_form<0>(len, img, cimg, out, ncu);
    case 'b': return run_form<1>(len, img, cimg, out, ncu);
    default: return run_form<2>(len, img, cimg, out, ncu);
  }
}
