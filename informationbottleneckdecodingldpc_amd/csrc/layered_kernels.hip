// Layered (row-serial) normalised / offset min-sum decoder, fp32, fused on chip (include/ibldpc.h
// "Layered min-sum"; host plan in layered_plan.h).
//
// One WAVE owns one codeword: its APP LLRs P[n_v] and the compressed state of every check (m1', m2', the
// argmin position and the sign bits of the check's outgoing messages R — R[e] is rebuilt from them, bit for
// bit) live in the wave's own slice of LDS through all iterations. A layer's checks share no variable, so a
// wave walks the tasks (up to 64 checks of one degree, lane = check) of layer after layer with no barrier at
// all: everything a task reads was written by the same wave, and a wave's LDS operations complete in order.
// A workgroup is cw_per_group such waves (as many codewords as fit in 160 KiB, at most 8); workgroups walk
// the groups of cw_per_group consecutive codewords with a grid-stride loop, wave w of group g decoding codeword
// g * cw_per_group + w. The early stop is therefore per codeword by construction: a wave that finds its
// syndrome zero writes its output and takes its next codeword while its neighbours go on.
//
// Codewords travel through a [B][N] scratch buffer (lay_transpose before and after), so a wave loads and
// stores its codeword as contiguous rows (waves reading and writing the caller's [N][B] arrays directly, one
// 4-byte element per 64-byte segment, measured slower: DESIGN.md "Layered min-sum").
//
// Arithmetic: every operation is one rounded fp32 operation (the file is compiled with -ffp-contract=off:
// alpha * m - beta and Q + R must not become FMAs).
#include "common.h"
#include "layered_plan.h"

namespace ibl {

// Diagnostic builds (-DIBL_LAY_TRACE=1, tools/variants.py laytrace): wave 0 of workgroup 0 records, for its
// first codeword's second iteration, three clocks per task — start, variable indices arrived, end (all its
// LDS writes done) — into LayeredArgs::trace. The product build has none of it.
#ifndef IBL_LAY_TRACE
#define IBL_LAY_TRACE 0
#endif

namespace {

#if IBL_LAY_TRACE
__device__ __forceinline__ uint64_t lay_clock() {
  __builtin_amdgcn_s_waitcnt(0);   // every outstanding load / store of the wave is done
  const uint64_t t = __builtin_readcyclecounter();
  __builtin_amdgcn_sched_barrier(0);
  return t;
}
#endif

__device__ __forceinline__ uint32_t lay_bits(float x) { return __builtin_bit_cast(uint32_t, x); }
// `mag` with the sign bit of `sign`: one v_and_or_b32. mag is +0 or positive — a corrected magnitude
// max(alpha m - beta, 0) or the initial 0 — so its own sign bit is clear.
__device__ __forceinline__ float lay_signed(float mag, uint32_t sign) {
  return __builtin_bit_cast(float, lay_bits(mag) | (sign & 0x80000000u));
}

// One task of checks of degree D: lane < cnt owns check `slot`; v-index rows at idx + 64 k.
// The kernel is bound by vector-ALU issue (two waves a SIMD), so the body is written for few instructions
// per edge; every step keeps the VALUES of the specification:
//   - clamp = median(x, -L, +L) (x is finite);
//   - no P, R or Q is ever -0 (lay_fused loads the channel values as x + 0; P - R is -0 only for P = -0,
//     Q + R only for Q = R = -0, and a magnitude max(., 0) is +0), so the sign bit of Q IS (Q < 0): the check's
//     parity is the XOR of the Q words' sign bits, and the sign of R[e] the sign bit of (that XOR ^ Q_e);
//   - m2 = median(m1, m2, a) before m1 = min(m1, a): the running two smallest; the position moves only on
//     a < m1, so it is the FIRST position attaining the minimum;
//   - state word: argmin position << 16 | sign bits of R, edge k at bit D - 1 - k (shifted in one edge at a
//     time by v_alignbit_b32).
template <int D>
__device__ __forceinline__ void lay_cn(float* __restrict__ P, float* __restrict__ M1, float* __restrict__ M2,
                                       uint32_t* __restrict__ PS, const int32_t* __restrict__ idx, int slot,
                                       float alpha, float beta, float L, uint64_t* tr) {
  int v[D];
#pragma unroll
  for (int k = 0; k < D; ++k) v[k] = idx[64 * k];
#if IBL_LAY_TRACE
  if (tr) {
    const uint64_t t = lay_clock();
    if ((threadIdx.x & 63u) == 0) tr[1] = t;
  }
#endif
  const float m1o = M1[slot], m2o = M2[slot];
  const uint32_t ps = PS[slot];
  const uint32_t poso = ps >> 16;
  float q[D];
  float m1 = __builtin_inff(), m2 = __builtin_inff();
  uint32_t pos = 0, sx = 0;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const float r = lay_signed((uint32_t)k == poso ? m2o : m1o, ps << (32 - D + k));
    const float x = __builtin_amdgcn_fmed3f(P[v[k]] - r, -L, L);
    q[k] = x;
    sx ^= lay_bits(x);
    const float a = fabsf(x);
    pos = a < m1 ? (uint32_t)k : pos;
    m2 = __builtin_amdgcn_fmed3f(m1, m2, a);
    m1 = fminf(m1, a);
  }
  const float m1n = fmaxf(alpha * m1 - beta, 0.f), m2n = fmaxf(alpha * m2 - beta, 0.f);
  uint32_t sg = 0;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const uint32_t t = sx ^ lay_bits(q[k]);   // sign bit: s ^ neg_e, R[e] is negated
    P[v[k]] = q[k] + lay_signed((uint32_t)k == pos ? m2n : m1n, t);
    sg = __builtin_amdgcn_alignbit(sg, t, 31);   // (sg << 1) | (t >> 31)
  }
  M1[slot] = m1n;
  M2[slot] = m2n;
  PS[slot] = (pos << 16) | sg;
}

__device__ __forceinline__ void lay_cn_any(int d, float* P, float* M1, float* M2, uint32_t* PS, const int32_t* idx,
                                           int slot, float alpha, float beta, float L, uint64_t* tr) {
  switch (d) {
#define LAY_CASE(D) case D: lay_cn<D>(P, M1, M2, PS, idx, slot, alpha, beta, L, tr); break;
    LAY_CASE(2) LAY_CASE(3) LAY_CASE(4) LAY_CASE(5) LAY_CASE(6) LAY_CASE(7) LAY_CASE(8) LAY_CASE(9)
    LAY_CASE(10) LAY_CASE(11) LAY_CASE(12) LAY_CASE(13) LAY_CASE(14) LAY_CASE(15) LAY_CASE(16)
#undef LAY_CASE
    default: break;
  }
}

}  // namespace

__global__ __launch_bounds__(64 * kLayMaxCw) void lay_fused(const LayeredArgs a) {
  extern __shared__ __align__(16) unsigned char lay_lds[];
  const int lane = (int)(threadIdx.x & 63u);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int ncw = a.cw_per_group;
  if (wave >= ncw) return;
  unsigned char* base = lay_lds + (size_t)wave * (size_t)a.cw_bytes;
  float* P = reinterpret_cast<float*>(base);
  float* M1 = P + a.n_v;
  float* M2 = M1 + a.n_c;
  uint32_t* PS = reinterpret_cast<uint32_t*>(M2 + a.n_c);
  const float alpha = a.alpha, beta = a.beta, L = a.llr_max;
  for (int g = (int)blockIdx.x; g < a.ngroups; g += (int)gridDim.x) {
    const int b = g * ncw + wave;
    if (b >= a.B) break;   // wave-uniform; later groups of this workgroup lie further still
    // + 0: a -0 channel value enters as +0 (equal as a value); no later step produces a -0 from inputs
    // without one, which lay_cn's sign-bit arithmetic relies on
    float* row = a.buf + (size_t)b * (size_t)a.n_v;
    for (int v = lane; v < a.n_v; v += 64) P[v] = row[v] + 0.f;
    for (int c = lane; c < a.n_c; c += 64) {
      M1[c] = 0.f;
      M2[c] = 0.f;
      PS[c] = 0u;
    }
    int it = 1;
    for (;; ++it) {
      for (int t = 0; t < a.n_tasks; ++t) {
        const int first = sload(a.task, 4 * t), cnt = sload(a.task, 4 * t + 1), d = sload(a.task, 4 * t + 2),
                  s0 = sload(a.task, 4 * t + 3);
        uint64_t* tr = nullptr;
#if IBL_LAY_TRACE
        if (a.trace && blockIdx.x == 0 && wave == 0 && g == (int)blockIdx.x && it == 2) {
          tr = a.trace + 3 * t;
          const uint64_t t0 = lay_clock();
          if (lane == 0) tr[0] = t0;
        }
#endif
        if (lane < cnt) lay_cn_any(d, P, M1, M2, PS, a.idx + first + lane, s0 + lane, alpha, beta, L, tr);
        __builtin_amdgcn_wave_barrier();   // the next task's reads stay behind this task's writes (other lanes')
#if IBL_LAY_TRACE
        if (tr) {
          const uint64_t t2 = lay_clock();
          if (lane == 0) tr[2] = t2;
        }
#endif
      }
      if (it >= a.imax) break;
      if (a.early) {
        // syndrome of the hard decisions after the complete iteration; leaves at the first task with an
        // unsatisfied check (the common case while the codeword has not converged)
        bool bad = false;
        for (int t = 0; t < a.n_tasks && !bad; ++t) {
          const int first = sload(a.task, 4 * t), cnt = sload(a.task, 4 * t + 1), d = sload(a.task, 4 * t + 2);
          uint32_t par = 0;
          if (lane < cnt) {
            const int32_t* ix = a.idx + first + lane;
            for (int k = 0; k < d; ++k) par ^= (P[ix[64 * k]] < 0.f) ? 1u : 0u;
          }
          bad = __builtin_amdgcn_readfirstlane((int)(__ballot(par != 0) != 0ull)) != 0;
        }
        if (!bad) break;
      }
    }
    for (int v = lane; v < a.n_v; v += 64) row[v] = P[v];
    if (a.iters && lane == 0) a.iters[b] = it;
  }
}

// dst[c][r] = src[r][c] for r < rows, c < cols (fp32; 64 x 64 tiles through LDS, 256 threads)
__global__ __launch_bounds__(256) void lay_transpose(const float* __restrict__ src, float* __restrict__ dst, int rows,
                                                     int cols) {
  __shared__ float tile[64][65];
  const int tx = (int)(threadIdx.x & 63u), ty = (int)(threadIdx.x >> 6);
  const unsigned tiles_x = (unsigned)((cols + 63) / 64);
  const size_t r0 = (size_t)(blockIdx.x / tiles_x) * 64, c0 = (size_t)(blockIdx.x % tiles_x) * 64;
  for (int j = ty; j < 64; j += 4) {
    const size_t r = r0 + j, c = c0 + tx;
    if (r < (size_t)rows && c < (size_t)cols) tile[j][tx] = src[r * (size_t)cols + c];
  }
  __syncthreads();
  for (int j = ty; j < 64; j += 4) {
    const size_t c = c0 + j, r = r0 + tx;
    if (r < (size_t)rows && c < (size_t)cols) dst[c * (size_t)rows + r] = tile[tx][j];
  }
}

hipError_t lay_fused_occupancy(int cw_per_group, size_t lds, int* blocks_per_cu, size_t* private_bytes) {
  const void* f = (const void*)lay_fused;
  hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
  if (e != hipSuccess) return e;
  hipFuncAttributes fa;
  if ((e = hipFuncGetAttributes(&fa, f)) != hipSuccess) return e;
  *private_bytes = fa.localSizeBytes;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, f, 64 * cw_per_group, lds);
}

hipError_t launch_lay_fused(const LayeredArgs& a, int grid, size_t lds, hipStream_t s) {
  if (!a.buf || !a.task || !a.idx || a.cw_per_group < 1 || a.cw_per_group > kLayMaxCw || a.n_tasks < 1 ||
      a.B < 1 || a.ngroups < 1 || grid < 1 || lds < (size_t)a.cw_per_group * (size_t)a.cw_bytes ||
      lds > (size_t)kLdsBytes)
    return hipErrorInvalidValue;
  LayeredArgs args = a;
  void* p[] = {&args};
  return hipLaunchKernel((const void*)lay_fused, dim3(grid), dim3(64 * a.cw_per_group), p, lds, s);
}

hipError_t launch_lay_transpose(const float* src, float* dst, int rows, int cols, hipStream_t s) {
  if (!src || !dst || rows < 1 || cols < 1) return hipErrorInvalidValue;
  const uint64_t tiles = (uint64_t)((cols + 63) / 64) * (uint64_t)((rows + 63) / 64);
  if (tiles > 0x7fffffffull) return hipErrorInvalidValue;
  void* p[] = {(void*)&src, (void*)&dst, (void*)&rows, (void*)&cols};
  return hipLaunchKernel((const void*)lay_transpose, dim3((unsigned)tiles), dim3(256), p, 0, s);
}

}  // namespace ibl
