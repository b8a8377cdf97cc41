// Layered belief-propagation decoder with half-precision state (include/ibldpc.h "Layered BP, half-precision state";
// host plan in layered_plan.h "layered BP, half state"): the fused on-chip kernel and the per-layer kernels over HBM.
// P and R are stored as IEEE binary16, the arithmetic is the fp32 decoder's: both kernels run its check core,
// lay_bp<D> (layered_bp_core.h), in its operation order, and give each other's bits.
//
// The conversions sit in the loads and stores. h(x) = (_Float16)med3(x, -65504, +65504) compiles to v_med3_f32 and
// v_cvt_f16_f32, which rounds to nearest even (never the packed round-toward-zero conversion); subnormal halves are
// kept (amdhsa_float_denorm_mode_16_64 is 3). The message that enters P is the ROUNDED one, P = h(Q + f(h(R'))): the
// store of R hands the rounded value back to the core (lay_bp_put).
//
// h turns a tiny negative sum into -0, which the fp32 kernels never hold. Every decision here therefore compares the
// VALUE with 0 — f(P) < 0 — and no kernel looks at a sign bit; the fp32 lay_pack, which reads fp32 rows, cannot serve
// a half row, so this file packs the hard decisions itself.
//
// Built with -ffp-contract=off -fno-honor-nans like layered_bp_kernels.hip, for the same reasons.
#include "common.h"
#include "boxplus.h"
#include "layered_plan.h"
#include "layered_bp_core.h"

namespace ibl {

namespace {

constexpr float kHalfMax = 65504.f;

// h: clamp to the finite halves, round to nearest even
__device__ __forceinline__ _Float16 layhp_h(float x) {
  return (_Float16)__builtin_amdgcn_fmed3f(x, -kHalfMax, kHalfMax);
}
__device__ __forceinline__ uint32_t layhp_bits(_Float16 x) { return (uint32_t)__builtin_bit_cast(uint16_t, x); }
__device__ __forceinline__ _Float16 layhp_half(uint32_t w, int j) {
  return __builtin_bit_cast(_Float16, (uint16_t)(w >> (16 * j)));
}

// One task of checks of degree D of the fused kernel: laybp_cn on half words
template <int D>
__device__ __forceinline__ void layhp_cn(_Float16* __restrict__ P, _Float16* __restrict__ R,
                                         const int32_t* __restrict__ idx, int cnt, float L) {
  int v[D];
#pragma unroll
  for (int k = 0; k < D; ++k) v[k] = idx[64 * k];
  lay_bp<D>([&](int k) { return (float)P[v[k]]; }, [&](int k) { return (float)R[cnt * k]; },
            [&](int k, float x) { P[v[k]] = layhp_h(x); },
            [&](int k, float x) {
              const _Float16 r = layhp_h(x);
              R[cnt * k] = r;
              return (float)r;
            },
            L);
}

}  // namespace

// The fused kernel: laybp_fused's walk with the wave's slice of LDS P16[n_v] | R16[E] (cw_bytes = 2 N + 2 E rounded up
// to 4), 2-byte accesses. The task records and the [B][n_v] fp32 rows are the fp32 kernel's; the wave converts as it
// stages a row in and out.
__global__ __launch_bounds__(64 * kLayMaxCw) void layhp_fused(const LayeredArgs a) {
  extern __shared__ __align__(16) unsigned char layhp_lds[];
  const int lane = (int)(threadIdx.x & 63u);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int ncw = a.cw_per_group;
  if (wave >= ncw) return;
  _Float16* P = reinterpret_cast<_Float16*>(layhp_lds + (size_t)wave * (size_t)a.cw_bytes);
  _Float16* R = P + a.n_v;
  const int n_e = a.cw_bytes / 2 - a.n_v;   // E, or E + 1 when 2 N + 2 E was rounded up: inside the slice either way
  const float L = a.llr_max;
  for (int g = (int)blockIdx.x; g < a.ngroups; g += (int)gridDim.x) {
    const int b = g * ncw + wave;
    if (b >= a.B) break;   // wave-uniform; later groups of this workgroup lie further still
    float* row = a.buf + (size_t)b * (size_t)a.n_v;
    for (int v = lane; v < a.n_v; v += 64) P[v] = layhp_h(row[v] + 0.f);   // a -0 channel value enters as +0
    for (int e = lane; e < n_e; e += 64) R[e] = (_Float16)0.f;
    int it = 1;
    for (;; ++it) {
      for (int t = 0; t < a.n_tasks; ++t) {
        const int first = sload(a.task, 4 * t), cnt = sload(a.task, 4 * t + 1), d = sload(a.task, 4 * t + 2),
                  r0 = sload(a.task, 4 * t + 3);
        if (lane < cnt) {
          switch (d) {
#define LAY_CASE(D) case D: layhp_cn<D>(P, R + r0 + lane, a.idx + first + lane, cnt, L); break;
            LAYBP_CASES
#undef LAY_CASE
            default: break;
          }
        }
        __builtin_amdgcn_wave_barrier();   // the next task's reads stay behind this task's writes (other lanes')
      }
      if (it >= a.imax) break;
      if (a.early) {
        // syndrome of the hard decisions (by value: -0 decides 0) after the complete iteration
        bool bad = false;
        for (int t = 0; t < a.n_tasks && !bad; ++t) {
          const int first = sload(a.task, 4 * t), cnt = sload(a.task, 4 * t + 1), d = sload(a.task, 4 * t + 2);
          uint32_t par = 0;
          if (lane < cnt) {
            const int32_t* ix = a.idx + first + lane;
            for (int k = 0; k < d; ++k) par ^= ((float)P[ix[64 * k]] < 0.f) ? 1u : 0u;
          }
          bad = __builtin_amdgcn_readfirstlane((int)(__ballot(par != 0) != 0ull)) != 0;
        }
        if (!bad) break;
      }
    }
    for (int v = lane; v < a.n_v; v += 64) row[v] = (float)P[v];
    if (a.iters && lane == 0) a.iters[b] = it;
  }
}

hipError_t layhp_fused_occupancy(int cw_per_group, size_t lds, int* blocks_per_cu, size_t* private_bytes) {
  const void* f = (const void*)layhp_fused;
  hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
  if (e != hipSuccess) return e;
  hipFuncAttributes fa;
  if ((e = hipFuncGetAttributes(&fa, f)) != hipSuccess) return e;
  *private_bytes = fa.localSizeBytes;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, f, 64 * cw_per_group, lds);
}

hipError_t launch_layhp_fused(const LayeredArgs& a, int grid, size_t lds, hipStream_t s) {
  if (!a.buf || !a.task || !a.idx || a.cw_per_group < 1 || a.cw_per_group > kLayMaxCw || a.n_tasks < 1 || a.B < 1 ||
      a.ngroups < 1 || grid < 1 || a.n_v < 1 || (a.cw_bytes & 3) != 0 ||
      (size_t)a.cw_bytes < (size_t)2 * (size_t)a.n_v || lds < (size_t)a.cw_per_group * (size_t)a.cw_bytes ||
      lds > (size_t)kLdsBytes)
    return hipErrorInvalidValue;
  LayeredArgs args = a;
  void* p[] = {&args};
  return hipLaunchKernel((const void*)layhp_fused, dim3(grid), dim3(64 * a.cw_per_group), p, lds, s);
}

// ---------------------------------------------------------------------------------------------------------------
// Per-layer path over HBM: P16 [n_v][ldb] and R16 [E][ldb] halves, a lane owning two consecutive codewords (one dword
// of a row), ldb = 128 ntiles2. One launch per layer, a wave item (check of the layer, tile of kLayHalfTile = 128
// codewords): a row access is 256 bytes per wave as on the fp32 path, and a lane runs two independent box-plus
// chains. The masks, the counter and the packed hard decisions stay per 64 codewords (the fp32 path's
// lay_syndrome_packed and lay_finalise are launched as they stand); the mask words of a tile of 128 past the batch
// are all ones.
namespace {

// finished bits of the lane's two codewords (bit j: codeword 2 lane + j of the tile); *all: the whole tile is finished
__device__ __forceinline__ uint32_t layhp_finished(const uint64_t* done, int tile2, int lane, bool* all) {
  const int32_t* w = reinterpret_cast<const int32_t*>(done);
  const uint64_t d0 = (uint64_t)(uint32_t)sload(w, 4 * tile2) | ((uint64_t)(uint32_t)sload(w, 4 * tile2 + 1) << 32),
                 d1 = (uint64_t)(uint32_t)sload(w, 4 * tile2 + 2) | ((uint64_t)(uint32_t)sload(w, 4 * tile2 + 3) << 32);
  *all = (d0 & d1) == ~0ull;
  const uint64_t dm = (lane >> 5) ? d1 : d0;
  return (uint32_t)(dm >> ((lane & 31) * 2)) & 3u;
}

// One check of degree D for the lane's two codewords. The row dwords are loaded first, the core runs once per
// codeword on its half of each, and the dwords go back whole: a finished codeword's half is stored as it was
// loaded (P: bit-stable; R: not read again). kFirst: the first iteration, R = 0 without a load, so the E rows are
// neither zeroed nor read before they are written; a lane-half that is finished there is padding and gets R = 0.
template <int D, bool kFirst>
__device__ __forceinline__ void layhp_cn_rows(const LayHalfArgs& a, int e0, size_t tcol, uint32_t lane, size_t ldb,
                                              uint32_t fin) {
  const auto prow = [&](int k) {
    return reinterpret_cast<uint32_t*>(a.P + ((size_t)sload(a.cols, e0 + k) * ldb + tcol));
  };
  const auto rrow = [&](int k) { return reinterpret_cast<uint32_t*>(a.R + ((size_t)(e0 + k) * ldb + tcol)); };
  uint32_t p[D], r[D];
#pragma unroll
  for (int k = 0; k < D; ++k) p[k] = prow(k)[lane];
#pragma unroll
  for (int k = 0; k < D; ++k) r[k] = kFirst ? 0u : rrow(k)[lane];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    // both chains run whatever `fin` says, so that they stay independent straight-line code the scheduler can
    // interleave; a finished codeword's values are finite and its results are dropped at the insertion
    const bool live = !((fin >> j) & 1u);
    const uint32_t keep = j ? 0x0000FFFFu : 0xFFFF0000u;
    lay_bp<D>([&](int k) { return (float)layhp_half(p[k], j); }, [&](int k) { return (float)layhp_half(r[k], j); },
              [&](int k, float x) {
                const uint32_t w = (p[k] & keep) | (layhp_bits(layhp_h(x)) << (16 * j));
                p[k] = live ? w : p[k];
              },
              [&](int k, float x) {
                const _Float16 m = layhp_h(x);
                const uint32_t w = (r[k] & keep) | (layhp_bits(m) << (16 * j));
                r[k] = live ? w : r[k];
                return (float)m;
              },
              a.llr_max);
  }
#pragma unroll
  for (int k = 0; k < D; ++k) {
    prow(k)[lane] = p[k];
    rrow(k)[lane] = r[k];
  }
}

template <bool kFirst>
__device__ __forceinline__ void layhp_layer_body(const LayHalfArgs a, int slot0, int n_checks) {
  if (sload(a.running, 0) == 0) return;
  const int lane = (int)(threadIdx.x & 63u);
  const int64_t item = (int64_t)blockIdx.x * kLayPassWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (item >= (int64_t)n_checks * a.ntiles2) return;
  const int tile = (int)(item % a.ntiles2);
  const int slot = slot0 + (int)(item / a.ntiles2);
  bool all;
  const uint32_t fin = layhp_finished(a.done, tile, lane, &all);
  if (all) return;           // wave-uniform: the whole tile is finished, before any vector load
  if (fin == 3u) return;     // the lane's two codewords are finished (or padding)
  const int e0 = sload(a.rec, 2 * slot), d = sload(a.rec, 2 * slot + 1);
  const size_t ldb = (size_t)a.ntiles2 * kLayHalfTile;
  const size_t tcol = (size_t)tile * kLayHalfTile;
  switch (d) {
#define LAY_CASE(D) case D: layhp_cn_rows<D, kFirst>(a, e0, tcol, (uint32_t)lane, ldb, fin); break;
    LAYBP_CASES
#undef LAY_CASE
    default: break;
  }
}

}  // namespace

__global__ __launch_bounds__(64 * kLayPassWaves) void layhp_layer(const LayHalfArgs a, int slot0, int n_checks) {
  layhp_layer_body<false>(a, slot0, n_checks);
}
__global__ __launch_bounds__(64 * kLayPassWaves) void layhp_layer_first(const LayHalfArgs a, int slot0, int n_checks) {
  layhp_layer_body<true>(a, slot0, n_checks);
}

// P = h(llr + 0) (a -0 enters as +0), padding codewords 0; masks, counter and iters reset. R is left as it is: the
// first iteration does not read it. item = (row < n_v, tile of 128).
__global__ __launch_bounds__(64 * kLayPassWaves) void layhp_stage_in(const LayHalfArgs a, const float* __restrict__ llr,
                                                                     int imax) {
  const int lane = (int)(threadIdx.x & 63u);
  const int64_t item = (int64_t)blockIdx.x * kLayPassWaves + (int64_t)(threadIdx.x >> 6);
  if (item >= (int64_t)a.n_v * a.ntiles2) return;
  const int tile = (int)(item % a.ntiles2);
  const int64_t row = item / a.ntiles2;
  const size_t ldb = (size_t)a.ntiles2 * kLayHalfTile;
  const int b0 = tile * kLayHalfTile + kLayHalfCw * lane;
  uint32_t w = 0u;
#pragma unroll
  for (int j = 0; j < kLayHalfCw; ++j)
    if (b0 + j < a.B) w |= layhp_bits(layhp_h(llr[(size_t)row * (size_t)a.B + (size_t)(b0 + j)] + 0.f)) << (16 * j);
  *reinterpret_cast<uint32_t*>(a.P + ((size_t)row * ldb + (size_t)b0)) = w;
  if (row == 0) {
    if (a.iters) {
#pragma unroll
      for (int j = 0; j < kLayHalfCw; ++j)
        if (b0 + j < a.B) a.iters[b0 + j] = imax;
    }
    if (lane < kLayHalfCw) {
      const int t64 = kLayHalfCw * tile + lane;
      a.done[t64] = half_done_word(t64, a.B);   // all ones for a mask word past the batch
      a.unsat[t64] = 0ull;
    }
    if (lane == 0 && tile == 0) *a.running = a.B;
  }
}

// Hard decisions of the half rows in lay_pack's form: bits[tile][v] bit b = (f(P[v][64 tile + b]) < 0), by value (a
// -0 decides 0), finished codewords 0. item = (run of 64 variables, tile of 64); lane i reads the 64 halves (128
// bytes) of variable v0 + i.
__global__ __launch_bounds__(64 * kLayPassWaves) void layhp_pack(const LayHalfArgs a) {
  if (sload(a.running, 0) == 0) return;
  const int lane = (int)(threadIdx.x & 63u);
  const int64_t item = (int64_t)blockIdx.x * kLayPassWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int nruns = (a.n_v + kLayTile - 1) / kLayTile;
  if (item >= (int64_t)nruns * a.ntiles) return;
  const int tile = (int)(item % a.ntiles);
  const int run = (int)(item / a.ntiles);
  const int32_t* dw = reinterpret_cast<const int32_t*>(a.done);
  const uint64_t dm = (uint64_t)(uint32_t)sload(dw, 2 * tile) | ((uint64_t)(uint32_t)sload(dw, 2 * tile + 1) << 32);
  if (dm == ~0ull) return;
  const int v = run * kLayTile + lane;
  if (v >= a.n_v) return;
  const size_t ldb = (size_t)a.ntiles2 * kLayHalfTile;
  const uint4* src = reinterpret_cast<const uint4*>(a.P + ((size_t)v * ldb + (size_t)tile * kLayTile));
  uint64_t word = 0ull;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const uint4 x = src[q];
    const uint32_t ws[4] = {x.x, x.y, x.z, x.w};
    uint32_t n = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      n |= ((float)layhp_half(ws[i], 0) < 0.f ? 1u : 0u) << (2 * i);
      n |= ((float)layhp_half(ws[i], 1) < 0.f ? 1u : 0u) << (2 * i + 1);
    }
    word |= (uint64_t)n << (8 * q);
  }
  a.bits[(size_t)tile * (size_t)a.n_v + (size_t)v] = word & ~dm;
}

// out[row][b] = f(P[row][b]) for b < B (padding codewords never reach the caller); item = (row < n_v, tile of 128)
__global__ __launch_bounds__(64 * kLayPassWaves) void layhp_stage_out(const LayHalfArgs a, float* __restrict__ out) {
  const int lane = (int)(threadIdx.x & 63u);
  const int64_t item = (int64_t)blockIdx.x * kLayPassWaves + (int64_t)(threadIdx.x >> 6);
  if (item >= (int64_t)a.n_v * a.ntiles2) return;
  const int tile = (int)(item % a.ntiles2);
  const int64_t row = item / a.ntiles2;
  const int b0 = tile * kLayHalfTile + kLayHalfCw * lane;
  if (b0 >= a.B) return;
  const uint32_t w =
      *reinterpret_cast<const uint32_t*>(a.P + ((size_t)row * (size_t)a.ntiles2 * kLayHalfTile + (size_t)b0));
#pragma unroll
  for (int j = 0; j < kLayHalfCw; ++j)
    if (b0 + j < a.B) out[(size_t)row * (size_t)a.B + (size_t)(b0 + j)] = (float)layhp_half(w, j);
}

namespace {
bool layhp_args_ok(const LayHalfArgs& a) {
  return a.P && a.R && a.done && a.unsat && a.running && a.bits && a.rec && a.cols && a.n_v >= 1 && a.n_c >= 1 &&
         a.B >= 1 && a.ntiles == pass_tiles(a.B) && a.ntiles2 == half_tiles(a.B) && a.llr_max > 0.f;
}
hipError_t layhp_launch(const void* f, int64_t items, void** p, hipStream_t s) {
  const int64_t grid = (items + kLayPassWaves - 1) / kLayPassWaves;
  if (grid < 1 || grid > 0x7fffffffll) return hipErrorInvalidValue;
  return hipLaunchKernel(f, dim3((unsigned)grid), dim3(64 * kLayPassWaves), p, 0, s);
}
}  // namespace

hipError_t launch_layhp_stage_in(const LayHalfArgs& a, const float* llr, int imax, hipStream_t s) {
  if (!layhp_args_ok(a) || !llr) return hipErrorInvalidValue;
  LayHalfArgs args = a;
  void* p[] = {&args, (void*)&llr, (void*)&imax};
  return layhp_launch((const void*)layhp_stage_in, (int64_t)a.n_v * a.ntiles2, p, s);
}

hipError_t launch_layhp_layer(const LayHalfArgs& a, bool first, int slot0, int n_checks, hipStream_t s) {
  if (!layhp_args_ok(a) || slot0 < 0 || n_checks < 0 || (int64_t)slot0 + n_checks > a.n_c) return hipErrorInvalidValue;
  if (n_checks == 0) return hipSuccess;
  LayHalfArgs args = a;
  void* p[] = {&args, (void*)&slot0, (void*)&n_checks};
  return layhp_launch(first ? (const void*)layhp_layer_first : (const void*)layhp_layer, half_items(n_checks, a.B), p,
                      s);
}

// pack the hard decisions of the half rows, then the fp32 path's packed syndrome and finalise (three launches)
hipError_t launch_layhp_stop(const LayHalfArgs& a, int it, hipStream_t s) {
  if (!layhp_args_ok(a)) return hipErrorInvalidValue;
  LayHalfArgs args = a;
  void* p[] = {&args};
  const hipError_t e = layhp_launch((const void*)layhp_pack, pass_items(pass_pack_runs(a.n_v), a.B), p, s);
  if (e != hipSuccess) return e;
  // the fp32 path's kernels read only what the two paths share
  LayPassArgs f{};
  f.done = a.done; f.unsat = a.unsat; f.running = a.running; f.bits = a.bits; f.rec = a.rec; f.cols = a.cols;
  f.iters = a.iters; f.n_v = a.n_v; f.n_c = a.n_c; f.B = a.B; f.ntiles = a.ntiles;
  return launch_lay_syndrome_finalise(f, it, s);
}

hipError_t launch_layhp_stage_out(const LayHalfArgs& a, float* out, hipStream_t s) {
  if (!layhp_args_ok(a) || !out) return hipErrorInvalidValue;
  LayHalfArgs args = a;
  void* p[] = {&args, (void*)&out};
  return layhp_launch((const void*)layhp_stage_out, (int64_t)a.n_v * a.ntiles2, p, s);
}

// the largest private (scratch) segment over the kernels of this file that a per-layer handle launches
hipError_t layhp_pass_private_bytes(size_t* bytes) {
  *bytes = 0;
  for (const void* f : {(const void*)layhp_stage_in, (const void*)layhp_layer, (const void*)layhp_layer_first,
                        (const void*)layhp_pack, (const void*)layhp_stage_out}) {
    hipFuncAttributes fa;
    const hipError_t e = hipFuncGetAttributes(&fa, f);
    if (e != hipSuccess) return e;
    *bytes = std::max(*bytes, (size_t)fa.localSizeBytes);
  }
  return hipSuccess;
}

}  // namespace ibl
