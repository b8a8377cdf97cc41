// Layered (row-serial) belief-propagation decoder, fp32 (include/ibldpc.h "Layered BP"; host plan in layered_plan.h
// "layered BP"): the fused on-chip kernel and the per-layer kernels over HBM. Both run one check core, lay_bp<D>, in
// one operation order, so they give the same bits.
//
// The schedule, the task walk, the per-codeword stop, the masks and the staging are those of the layered min-sum
// decoder (layered_kernels.hip), whose transpose, pack, syndrome, finalise and stage-out kernels this decoder
// launches as they stand. What differs is the check update — the forward-backward box-plus of the flooding fp32 BP
// check node (boxplus.h), stated once in layered_bp_core.h for this file and layered_half_kernels.hip — and the state:
// BP has no compressed form of a check's outgoing messages, so R is kept whole, one fp32 word per edge and codeword.
//
// Arithmetic: Q = P - R and P = Q + R' are one rounded fp32 operation each, Q is NOT clamped (the specification says
// why). The file is built with -ffp-contract=off like layered_kernels.hip; the box-plus states its one fused
// multiply-add itself.
#include "common.h"
#include "boxplus.h"
#include "layered_plan.h"
#include "layered_bp_core.h"

namespace ibl {

namespace {

// One task of checks of degree D of the fused kernel: the lane's check reads its variable indices at idx + 64 k and
// keeps its messages at R + cnt k (idx, R: the task's, already advanced by the lane).
template <int D>
__device__ __forceinline__ void laybp_cn(float* __restrict__ P, float* __restrict__ R, const int32_t* __restrict__ idx,
                                         int cnt, float L) {
  int v[D];
#pragma unroll
  for (int k = 0; k < D; ++k) v[k] = idx[64 * k];
  lay_bp<D>([&](int k) { return P[v[k]]; }, [&](int k) { return R[cnt * k]; }, [&](int k, float x) { P[v[k]] = x; },
            [&](int k, float x) { R[cnt * k] = x; }, L);
}

}  // namespace

// The fused kernel: lay_fused_body's walk with the wave's slice of LDS P[n_v] | R[E] (cw_bytes = 4 N + 4 E). A task
// record is {first idx, count, degree, first R word}: edge k of lane i has its variable at idx[first + 64 k + i]
// (padded rows, as the min-sum plan's) and its message at R[rfirst + count k + i] (unpadded: R is exactly E words,
// which is what the fit rule counts), so the lanes of a task touch consecutive words of both.
__global__ __launch_bounds__(64 * kLayMaxCw) void laybp_fused(const LayeredArgs a) {
  extern __shared__ __align__(16) unsigned char laybp_lds[];
  const int lane = (int)(threadIdx.x & 63u);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int ncw = a.cw_per_group;
  if (wave >= ncw) return;
  float* P = reinterpret_cast<float*>(laybp_lds + (size_t)wave * (size_t)a.cw_bytes);
  float* R = P + a.n_v;
  const int n_e = a.cw_bytes / 4 - a.n_v;
  const float L = a.llr_max;
  for (int g = (int)blockIdx.x; g < a.ngroups; g += (int)gridDim.x) {
    const int b = g * ncw + wave;
    if (b >= a.B) break;   // wave-uniform; later groups of this workgroup lie further still
    float* row = a.buf + (size_t)b * (size_t)a.n_v;
    for (int v = lane; v < a.n_v; v += 64) P[v] = row[v] + 0.f;   // a -0 channel value enters as +0
    for (int e = lane; e < n_e; e += 64) R[e] = 0.f;
    int it = 1;
    for (;; ++it) {
      for (int t = 0; t < a.n_tasks; ++t) {
        const int first = sload(a.task, 4 * t), cnt = sload(a.task, 4 * t + 1), d = sload(a.task, 4 * t + 2),
                  r0 = sload(a.task, 4 * t + 3);
        if (lane < cnt) {
          switch (d) {
#define LAY_CASE(D) case D: laybp_cn<D>(P, R + r0 + lane, a.idx + first + lane, cnt, L); break;
            LAYBP_CASES
#undef LAY_CASE
            default: break;
          }
        }
        __builtin_amdgcn_wave_barrier();   // the next task's reads stay behind this task's writes (other lanes')
      }
      if (it >= a.imax) break;
      if (a.early) {
        // syndrome of the hard decisions after the complete iteration; leaves at the first task with an
        // unsatisfied check
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

hipError_t laybp_fused_occupancy(int cw_per_group, size_t lds, int* blocks_per_cu, size_t* private_bytes) {
  const void* f = (const void*)laybp_fused;
  hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
  if (e != hipSuccess) return e;
  hipFuncAttributes fa;
  if ((e = hipFuncGetAttributes(&fa, f)) != hipSuccess) return e;
  *private_bytes = fa.localSizeBytes;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, f, 64 * cw_per_group, lds);
}

hipError_t launch_laybp_fused(const LayeredArgs& a, int grid, size_t lds, hipStream_t s) {
  if (!a.buf || !a.task || !a.idx || a.cw_per_group < 1 || a.cw_per_group > kLayMaxCw || a.n_tasks < 1 || a.B < 1 ||
      a.ngroups < 1 || grid < 1 || a.n_v < 1 || (size_t)a.cw_bytes < (size_t)4 * (size_t)a.n_v ||
      lds < (size_t)a.cw_per_group * (size_t)a.cw_bytes || lds > (size_t)kLdsBytes)
    return hipErrorInvalidValue;
  LayeredArgs args = a;
  void* p[] = {&args};
  return hipLaunchKernel((const void*)laybp_fused, dim3(grid), dim3(64 * a.cw_per_group), p, lds, s);
}

// ---------------------------------------------------------------------------------------------------------------
// Per-layer path over HBM: lane = codeword, P[n_v][ldb] and R[E][ldb] (row = CSR edge: the check's first edge, from
// its record, plus k), one launch per layer, a wave item (check of the layer, tile of 64 codewords). The masks, the
// counter and the stop are the min-sum path's, and so are its pack, syndrome, finalise and stage-out kernels.
// LayPassArgs serves with M1 = R; M2 and PS are not read.
namespace {

// Rows are a wave-uniform base (scalar loads and the wave's tile) plus the lane, as in lay_cn_rows_wide. kFirst: the
// first iteration, R = 0 without a load (P - 0 is P), so the E rows are neither zeroed nor read before they are
// written.
template <int D, bool kFirst>
__device__ __forceinline__ void laybp_cn_rows(const LayPassArgs& a, int e0, size_t tcol, uint32_t lane, size_t ldb) {
  const auto prow = [&](int k) { return a.P + ((size_t)sload(a.cols, e0 + k) * ldb + tcol); };
  const auto rrow = [&](int k) { return a.M1 + ((size_t)(e0 + k) * ldb + tcol); };
  float p[D], r[D];
#pragma unroll
  for (int k = 0; k < D; ++k) p[k] = prow(k)[lane];
#pragma unroll
  for (int k = 0; k < D; ++k) r[k] = kFirst ? 0.f : rrow(k)[lane];
  lay_bp<D>([&](int k) { return p[k]; }, [&](int k) { return r[k]; }, [&](int k, float x) { prow(k)[lane] = x; },
            [&](int k, float x) { rrow(k)[lane] = x; }, a.llr_max);
}

template <bool kFirst>
__device__ __forceinline__ void laybp_layer_body(const LayPassArgs a, int slot0, int n_checks) {
  if (sload(a.running, 0) == 0) return;
  const int lane = (int)(threadIdx.x & 63u);
  const int64_t item = (int64_t)blockIdx.x * kLayPassWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (item >= (int64_t)n_checks * a.ntiles) return;
  const int tile = (int)(item % a.ntiles);
  const int slot = slot0 + (int)(item / a.ntiles);
  const uint64_t dm = (uint64_t)(uint32_t)sload(reinterpret_cast<const int32_t*>(a.done), 2 * tile) |
                      ((uint64_t)(uint32_t)sload(reinterpret_cast<const int32_t*>(a.done), 2 * tile + 1) << 32);
  if (dm == ~0ull) return;            // wave-uniform: the whole tile is finished, before any vector load
  if ((dm >> lane) & 1ull) return;    // a finished (or padding) lane loads and stores nothing
  const int e0 = sload(a.rec, 2 * slot), d = sload(a.rec, 2 * slot + 1);
  const size_t ldb = (size_t)a.ntiles * kLayTile;
  const size_t tcol = (size_t)tile * kLayTile;
  switch (d) {
#define LAY_CASE(D) case D: laybp_cn_rows<D, kFirst>(a, e0, tcol, (uint32_t)lane, ldb); break;
    LAYBP_CASES
#undef LAY_CASE
    default: break;
  }
}

}  // namespace

__global__ __launch_bounds__(64 * kLayPassWaves) void laybp_layer(const LayPassArgs a, int slot0, int n_checks) {
  laybp_layer_body<false>(a, slot0, n_checks);
}
__global__ __launch_bounds__(64 * kLayPassWaves) void laybp_layer_first(const LayPassArgs a, int slot0, int n_checks) {
  laybp_layer_body<true>(a, slot0, n_checks);
}

// P = llr + 0 (a -0 enters as +0), padding lanes 0; masks, counter and iters reset. R is left as it is: the first
// iteration does not read it. item = (row < n_v, tile).
__global__ __launch_bounds__(64 * kLayPassWaves) void laybp_stage_in(const LayPassArgs a, const float* __restrict__ llr,
                                                                     int imax) {
  const int lane = (int)(threadIdx.x & 63u);
  const int64_t item = (int64_t)blockIdx.x * kLayPassWaves + (int64_t)(threadIdx.x >> 6);
  if (item >= (int64_t)a.n_v * a.ntiles) return;
  const int tile = (int)(item % a.ntiles);
  const int64_t row = item / a.ntiles;
  const size_t ldb = (size_t)a.ntiles * kLayTile;
  const int b = tile * kLayTile + lane;
  a.P[(size_t)row * ldb + (size_t)b] = b < a.B ? llr[(size_t)row * (size_t)a.B + (size_t)b] + 0.f : 0.f;
  if (row == 0) {
    if (a.iters && b < a.B) a.iters[b] = imax;
    if (lane == 0) {
      const int left = a.B - tile * kLayTile;   // >= 1
      a.done[tile] = left >= kLayTile ? 0ull : ~0ull << left;
      a.unsat[tile] = 0ull;
      if (tile == 0) *a.running = a.B;
    }
  }
}

namespace {
bool laybp_args_ok(const LayPassArgs& a) {
  return a.P && a.M1 && a.done && a.unsat && a.running && a.rec && a.cols && a.n_v >= 1 && a.n_c >= 1 && a.B >= 1 &&
         a.ntiles == pass_tiles(a.B);
}
hipError_t laybp_launch(const void* f, int64_t items, void** p, hipStream_t s) {
  const int64_t grid = (items + kLayPassWaves - 1) / kLayPassWaves;
  if (grid < 1 || grid > 0x7fffffffll) return hipErrorInvalidValue;
  return hipLaunchKernel(f, dim3((unsigned)grid), dim3(64 * kLayPassWaves), p, 0, s);
}
}  // namespace

hipError_t launch_laybp_stage_in(const LayPassArgs& a, const float* llr, int imax, hipStream_t s) {
  if (!laybp_args_ok(a) || !llr) return hipErrorInvalidValue;
  LayPassArgs args = a;
  void* p[] = {&args, (void*)&llr, (void*)&imax};
  return laybp_launch((const void*)laybp_stage_in, (int64_t)a.n_v * a.ntiles, p, s);
}

hipError_t launch_laybp_layer(const LayPassArgs& a, bool first, int slot0, int n_checks, hipStream_t s) {
  if (!laybp_args_ok(a) || slot0 < 0 || n_checks < 0 || (int64_t)slot0 + n_checks > a.n_c) return hipErrorInvalidValue;
  if (n_checks == 0) return hipSuccess;
  LayPassArgs args = a;
  void* p[] = {&args, (void*)&slot0, (void*)&n_checks};
  return laybp_launch(first ? (const void*)laybp_layer_first : (const void*)laybp_layer, pass_items(n_checks, a.B), p,
                      s);
}

// the largest private (scratch) segment over the kernels of this file that a per-layer handle launches
hipError_t laybp_pass_private_bytes(size_t* bytes) {
  *bytes = 0;
  for (const void* f : {(const void*)laybp_stage_in, (const void*)laybp_layer, (const void*)laybp_layer_first}) {
    hipFuncAttributes fa;
    const hipError_t e = hipFuncGetAttributes(&fa, f);
    if (e != hipSuccess) return e;
    *bytes = std::max(*bytes, (size_t)fa.localSizeBytes);
  }
  return hipSuccess;
}

}  // namespace ibl
