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

// Narrow and wide handles (include/ibldpc.h "Layered min-sum", wide handles; layered_plan.h layered_is_wide). A handle
// whose code has a check of degree above kLayMaxD = 16 is wide and runs lay_fused_wide, lay_layer_wide and
// layfix_layer_wide instead of lay_fused, lay_layer and layfix_layer, for EVERY check of the code: kernels of their
// own, because the degree bodies of one kernel share one register allocation and unrolled degree-32 bodies inside
// lay_layer would cost the narrow codes their occupancy. The arithmetic is written once for both (lay_minsum,
// layfix_minsum); what differs is where the state lives:
//   fp32        narrow: one word PS, argmin position << 16 | sign bits of R. Wide: the sign bits fill PS (edge k at
//               bit D - 1 - k in both) and the position has a word of its own, PO: four 4-byte words per check and
//               codeword;
//   fixed point narrow: one word S (layered_plan.h fix_state_word). Wide: two words in two arrays S / S1 [n_c][ldb]
//               (fix_state_words_wide): m2' << 11 | m1' << 5 | position, and the sign bits of R, edge k at bit k.
// The wide form of a kernel takes the added array as an argument of its own. Syndrome, pack, finalise, stage-out,
// the compaction plan and commit serve both as they stand.
//
// The degrees with an unrolled body: 2..kLayMaxD on a narrow handle, 2..kLayWideMaxD on a wide one. Every kernel
// that switches on a check's degree defines LAY_CASE(D) around one of the two lists.
#define LAY_CASES_16                                                                                           \
  LAY_CASE(2) LAY_CASE(3) LAY_CASE(4) LAY_CASE(5) LAY_CASE(6) LAY_CASE(7) LAY_CASE(8) LAY_CASE(9) LAY_CASE(10) \
  LAY_CASE(11) LAY_CASE(12) LAY_CASE(13) LAY_CASE(14) LAY_CASE(15) LAY_CASE(16)
#define LAY_CASES_32                                                                                             \
  LAY_CASES_16 LAY_CASE(17) LAY_CASE(18) LAY_CASE(19) LAY_CASE(20) LAY_CASE(21) LAY_CASE(22) LAY_CASE(23)        \
  LAY_CASE(24) LAY_CASE(25) LAY_CASE(26) LAY_CASE(27) LAY_CASE(28) LAY_CASE(29) LAY_CASE(30) LAY_CASE(31)        \
  LAY_CASE(32)

// The fp32 check update of one check of degree D, the one statement of it for every kernel: load(k) is P of edge k,
// store(k, x) writes it back, and both are called inside the unrolled edge loops, so a caller's memory accesses sit
// where the arithmetic uses them. In: the corrected minima m1s, m2s, the first argmin position pos and the sign bits
// of R of the previous iteration (edge k at bit D - 1 - k of `signs`; higher bits are ignored); out: those of this one
// (`signs` then holds nothing else). Where the four words live is the caller's business.
// The kernels are bound by vector-ALU issue (two waves a SIMD on the fused one), so the body is written for few
// instructions per edge; every step keeps the VALUES of the specification:
//   - clamp = median(x, -L, +L) (x is finite);
//   - no P, R or Q is ever -0 (the stage-in loads the channel values as x + 0; P - R is -0 only for P = -0,
//     Q + R only for Q = R = -0, and a magnitude max(., 0) is +0), so the sign bit of Q IS (Q < 0): the check's
//     parity is the XOR of the Q words' sign bits, and the sign of R[e] the sign bit of (that XOR ^ Q_e);
//   - m2 = median(m1, m2, a) before m1 = min(m1, a): the running two smallest; the position moves only on
//     a < m1, so it is the FIRST position attaining the minimum;
//   - the sign bits of R are shifted in one edge at a time by v_alignbit_b32.
template <int D, class Load, class Store>
__device__ __forceinline__ void lay_minsum(Load load, Store store, float& m1s, float& m2s, uint32_t& pos,
                                           uint32_t& signs, float alpha, float beta, float L) {
  static_assert(D >= kLayMinD && D <= kLayWideMaxD, "degree body out of range");
  const float m1o = m1s, m2o = m2s;
  const uint32_t poso = pos, ps = signs;
  float q[D];
  float m1 = __builtin_inff(), m2 = __builtin_inff();
  uint32_t at = 0, sx = 0;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const float r = lay_signed((uint32_t)k == poso ? m2o : m1o, ps << (32 - D + k));
    const float x = __builtin_amdgcn_fmed3f(load(k) - r, -L, L);
    q[k] = x;
    sx ^= lay_bits(x);
    const float a = fabsf(x);
    at = a < m1 ? (uint32_t)k : at;
    m2 = __builtin_amdgcn_fmed3f(m1, m2, a);
    m1 = fminf(m1, a);
  }
  const float m1n = fmaxf(alpha * m1 - beta, 0.f), m2n = fmaxf(alpha * m2 - beta, 0.f);
  uint32_t sg = 0;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const uint32_t t = sx ^ lay_bits(q[k]);   // sign bit: s ^ neg_e, R[e] is negated
    store(k, q[k] + lay_signed((uint32_t)k == at ? m2n : m1n, t));
    sg = __builtin_amdgcn_alignbit(sg, t, 31);   // (sg << 1) | (t >> 31)
  }
  m1s = m1n;
  m2s = m2n;
  pos = at;
  signs = sg;
}

// One task of checks of degree D of the fused kernel: lane < cnt owns check `slot`; v-index rows at idx + 64 k.
// Narrow state word PS: argmin position << 16 | sign bits of R (the core's shifts drop the position); wide: PS is
// all sign bits and the position is PO[slot].
template <int D, bool kWide>
__device__ __forceinline__ void lay_cn(float* __restrict__ P, float* __restrict__ M1, float* __restrict__ M2,
                                       uint32_t* __restrict__ PS, uint32_t* __restrict__ PO,
                                       const int32_t* __restrict__ idx, int slot, float alpha, float beta, float L,
                                       uint64_t* tr) {
  static_assert(D <= (kWide ? kLayWideMaxD : kLayMaxD), "degree body out of range");
  int v[D];
#pragma unroll
  for (int k = 0; k < D; ++k) v[k] = idx[64 * k];
#if IBL_LAY_TRACE
  if (tr) {
    const uint64_t t = lay_clock();
    if ((threadIdx.x & 63u) == 0) tr[1] = t;
  }
#endif
  float m1 = M1[slot], m2 = M2[slot];
  uint32_t sg = PS[slot], pos;
  if constexpr (kWide) pos = PO[slot];
  else pos = sg >> 16;
  lay_minsum<D>([&](int k) { return P[v[k]]; }, [&](int k, float x) { P[v[k]] = x; }, m1, m2, pos, sg, alpha, beta, L);
  M1[slot] = m1;
  M2[slot] = m2;
  if constexpr (kWide) {
    PS[slot] = sg;
    PO[slot] = pos;
  } else {
    PS[slot] = (pos << 16) | sg;
  }
}

template <bool kWide>
__device__ __forceinline__ void lay_cn_any(int d, float* P, float* M1, float* M2, uint32_t* PS, uint32_t* PO,
                                           const int32_t* idx, int slot, float alpha, float beta, float L,
                                           uint64_t* tr) {
#define LAY_CASE(D) case D: lay_cn<D, kWide>(P, M1, M2, PS, PO, idx, slot, alpha, beta, L, tr); break;
  if constexpr (kWide) {
    switch (d) {
      LAY_CASES_32
      default: break;
    }
  } else {
    switch (d) {
      LAY_CASES_16
      default: break;
    }
  }
#undef LAY_CASE
}

// The fused kernel. kWide: the wave's slice of LDS is P[n_v], M1, M2, PS, PO [n_c] (cw_bytes = 4 N + 16 n_c).
// (the arguments by value, as the kernels have them: by reference the scalar code of the prologue changes)
template <bool kWide>
__device__ __forceinline__ void lay_fused_body(const LayeredArgs a) {
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
  uint32_t* PO = kWide ? PS + a.n_c : nullptr;
  const float alpha = a.alpha, beta = a.beta, L = a.llr_max;
  for (int g = (int)blockIdx.x; g < a.ngroups; g += (int)gridDim.x) {
    const int b = g * ncw + wave;
    if (b >= a.B) break;   // wave-uniform; later groups of this workgroup lie further still
    // + 0: a -0 channel value enters as +0 (equal as a value); no later step produces a -0 from inputs
    // without one, which lay_minsum's sign-bit arithmetic relies on
    float* row = a.buf + (size_t)b * (size_t)a.n_v;
    for (int v = lane; v < a.n_v; v += 64) P[v] = row[v] + 0.f;
    for (int c = lane; c < a.n_c; c += 64) {
      M1[c] = 0.f;
      M2[c] = 0.f;
      PS[c] = 0u;
      if constexpr (kWide) PO[c] = 0u;
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
        if (lane < cnt)
          lay_cn_any<kWide>(d, P, M1, M2, PS, PO, a.idx + first + lane, s0 + lane, alpha, beta, L, tr);
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

}  // namespace

__global__ __launch_bounds__(64 * kLayMaxCw) void lay_fused(const LayeredArgs a) { lay_fused_body<false>(a); }
__global__ __launch_bounds__(64 * kLayMaxCw) void lay_fused_wide(const LayeredArgs a) { lay_fused_body<true>(a); }

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

hipError_t lay_fused_occupancy(bool wide, int cw_per_group, size_t lds, int* blocks_per_cu, size_t* private_bytes) {
  const void* f = wide ? (const void*)lay_fused_wide : (const void*)lay_fused;
  hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
  if (e != hipSuccess) return e;
  hipFuncAttributes fa;
  if ((e = hipFuncGetAttributes(&fa, f)) != hipSuccess) return e;
  *private_bytes = fa.localSizeBytes;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, f, 64 * cw_per_group, lds);
}

hipError_t launch_lay_fused(const LayeredArgs& a, bool wide, int grid, size_t lds, hipStream_t s) {
  if (!a.buf || !a.task || !a.idx || a.cw_per_group < 1 || a.cw_per_group > kLayMaxCw || a.n_tasks < 1 ||
      a.B < 1 || a.ngroups < 1 || grid < 1 || lds < (size_t)a.cw_per_group * (size_t)a.cw_bytes ||
      lds > (size_t)kLdsBytes || (wide && (size_t)a.cw_bytes < layered_cw_bytes(a.n_v, a.n_c, true)))
    return hipErrorInvalidValue;
  LayeredArgs args = a;
  void* p[] = {&args};
  const void* f = wide ? (const void*)lay_fused_wide : (const void*)lay_fused;
  return hipLaunchKernel(f, dim3(grid), dim3(64 * a.cw_per_group), p, lds, s);
}

hipError_t launch_lay_transpose(const float* src, float* dst, int rows, int cols, hipStream_t s) {
  if (!src || !dst || rows < 1 || cols < 1) return hipErrorInvalidValue;
  const uint64_t tiles = (uint64_t)((cols + 63) / 64) * (uint64_t)((rows + 63) / 64);
  if (tiles > 0x7fffffffull) return hipErrorInvalidValue;
  void* p[] = {(void*)&src, (void*)&dst, (void*)&rows, (void*)&cols};
  return hipLaunchKernel((const void*)lay_transpose, dim3((unsigned)tiles), dim3(256), p, 0, s);
}

// ---------------------------------------------------------------------------------------------------------------
// Per-layer path over HBM (codes too long for LDS; include/ibldpc.h "Layered min-sum", IBL_PATH_PASSES).
//
// lane = codeword. P[n_v][ldb] and the compressed state M1 / M2 / PS [n_c][ldb] (the fused kernel's three words,
// a row per check, rows in layer order) live in device memory; ldb = 64 ntiles. One launch per layer: a wave item
// is (check of the layer, tile of 64 codewords) — the check's CSR offset, degree and variable indices are
// wave-uniform scalar loads, every row access one coalesced 256-byte segment. A layer's checks share no
// variable, so its items are independent; layers are ordered by the stream. Nothing here waits for another
// workgroup.
//
// Per-codeword stop: done[tile] holds a bit per finished codeword (padding lanes are finished from the start).
// After iteration it < imax, the syndrome — lay_pack + lay_syndrome_packed (default), or lay_syndrome, the gather
// form — ORs the unsatisfied codewords of a tile into unsat[tile] and lay_finalise(it) finishes the running codewords whose bit stayed clear: iters[b] = it, done bit, `running`
// decremented. A finished lane stores nothing in any later launch (its P row entries stay at the stop value), a
// wave whose tile is all finished leaves before its first vector load, and every kernel leaves at once when
// `running` is 0. The host enqueues all imax iterations up front and never reads anything back.
namespace {

__device__ __forceinline__ uint64_t lay_mask(const uint64_t* m, int tile) {
  const int32_t* w = reinterpret_cast<const int32_t*>(m);
  return (uint64_t)(uint32_t)sload(w, 2 * tile) | ((uint64_t)(uint32_t)sload(w, 2 * tile + 1) << 32);
}

// One check of degree D for the lane's codeword, narrow handle: column `col` of every row, a 64-bit element index
// per edge; the state word as in lay_cn.
template <int D>
__device__ __forceinline__ void lay_cn_rows(const LayPassArgs& a, int e0, size_t srow, size_t col, size_t ldb) {
  static_assert(D <= kLayMaxD, "degree body out of range");
  size_t v[D];
#pragma unroll
  for (int k = 0; k < D; ++k) v[k] = (size_t)sload(a.cols, e0 + k) * ldb + col;
  float p[D];
#pragma unroll
  for (int k = 0; k < D; ++k) p[k] = a.P[v[k]];
  float m1 = a.M1[srow], m2 = a.M2[srow];
  uint32_t sg = a.PS[srow], pos = sg >> 16;
  lay_minsum<D>([&](int k) { return p[k]; }, [&](int k, float x) { a.P[v[k]] = x; }, m1, m2, pos, sg, a.alpha, a.beta,
                a.llr_max);
  a.M1[srow] = m1;
  a.M2[srow] = m2;
  a.PS[srow] = (pos << 16) | sg;
}

// The same for a wide handle: the position in PO and all of PS sign bits. tcol: the tile's first column, srow: the
// first state word of (slot, tile), both wave-uniform; the lane's codeword is element `lane` of each. A row is
// addressed as a wave-uniform base (the variable index is a scalar load and the tile is the wave's) plus the lane,
// formed again for the store, so a check's D rows cost scalar registers and one 32-bit vector offset, not D 64-bit
// vector addresses.
template <int D>
__device__ __forceinline__ void lay_cn_rows_wide(const LayPassArgs& a, uint32_t* __restrict__ PO, int e0, size_t srow,
                                                 size_t tcol, uint32_t lane, size_t ldb) {
  const auto row = [&](int k) { return a.P + ((size_t)sload(a.cols, e0 + k) * ldb + tcol); };
  float p[D];
#pragma unroll
  for (int k = 0; k < D; ++k) p[k] = row(k)[lane];
  float m1 = (a.M1 + srow)[lane], m2 = (a.M2 + srow)[lane];
  uint32_t sg = (a.PS + srow)[lane], pos = (PO + srow)[lane];
  lay_minsum<D>([&](int k) { return p[k]; }, [&](int k, float x) { row(k)[lane] = x; }, m1, m2, pos, sg, a.alpha,
                a.beta, a.llr_max);
  (a.M1 + srow)[lane] = m1;
  (a.M2 + srow)[lane] = m2;
  (a.PS + srow)[lane] = sg;
  (PO + srow)[lane] = pos;
}

}  // namespace

// P = llr + 0 (a -0 enters as +0), padding lanes 0; state rows 0; masks, counter and iters reset.
// item = (row < max(n_v, n_c), tile). kCompact: also orig = the identity, extent = B, no compaction yet.
// kWide: also the rows of PO, the wide handle's fourth state array.
namespace {
template <bool kCompact, bool kWide = false>
__device__ __forceinline__ void lay_stage_in_body(const LayPassArgs& a, const float* __restrict__ llr, int imax,
                                                  const LayCompactArgs* c, uint32_t* PO = nullptr) {
  const int lane = (int)(threadIdx.x & 63u);
  const int64_t item = (int64_t)blockIdx.x * kLayPassWaves + (int64_t)(threadIdx.x >> 6);
  const int64_t rows = a.n_v > a.n_c ? a.n_v : a.n_c;
  if (item >= rows * a.ntiles) return;
  const int tile = (int)(item % a.ntiles);
  const int64_t row = item / a.ntiles;
  const size_t ldb = (size_t)a.ntiles * kLayTile;
  const int b = tile * kLayTile + lane;
  const size_t at = (size_t)row * ldb + (size_t)b;
  if (row < a.n_v) a.P[at] = b < a.B ? llr[(size_t)row * (size_t)a.B + (size_t)b] + 0.f : 0.f;
  if (row < a.n_c) {
    a.M1[at] = 0.f;
    a.M2[at] = 0.f;
    a.PS[at] = 0u;
    if constexpr (kWide) PO[at] = 0u;
  }
  if (row == 0) {
    if (a.iters && b < a.B) a.iters[b] = imax;
    if constexpr (kCompact) c->orig[b] = b;
    if (lane == 0) {
      const int left = a.B - tile * kLayTile;   // >= 1
      a.done[tile] = left >= kLayTile ? 0ull : ~0ull << left;
      a.unsat[tile] = 0ull;
      if (tile == 0) {
        *a.running = a.B;
        if constexpr (kCompact) {
          c->ctl[kLayCtlExtent] = a.B;
          c->ctl[kLayCtlDo] = 0;
          c->ctl[kLayCtlCount] = 0;
        }
      }
    }
  }
}
}  // namespace

__global__ __launch_bounds__(64 * kLayPassWaves) void lay_stage_in(const LayPassArgs a, const float* __restrict__ llr,
                                                                   int imax) {
  lay_stage_in_body<false>(a, llr, imax, nullptr);
}
__global__ __launch_bounds__(64 * kLayPassWaves) void lay_stage_in_c(const LayPassArgs a, const LayCompactArgs c,
                                                                     const float* __restrict__ llr, int imax) {
  lay_stage_in_body<true>(a, llr, imax, &c);
}
__global__ __launch_bounds__(64 * kLayPassWaves) void lay_stage_in_wide(const LayPassArgs a, uint32_t* PO,
                                                                        const float* __restrict__ llr, int imax) {
  lay_stage_in_body<false, true>(a, llr, imax, nullptr, PO);
}
__global__ __launch_bounds__(64 * kLayPassWaves) void lay_stage_in_c_wide(const LayPassArgs a, const LayCompactArgs c,
                                                                          uint32_t* PO, const float* __restrict__ llr,
                                                                          int imax) {
  lay_stage_in_body<true, true>(a, llr, imax, &c, PO);
}

// One layer: item = (check slot0 + c of the layer, tile), tile fastest. The two kernels differ in the degree list and
// in how the body addresses a row; a wide handle runs lay_layer_wide for every check of its code.
__global__ __launch_bounds__(64 * kLayPassWaves) void lay_layer(const LayPassArgs a, int slot0, int n_checks) {
  if (sload(a.running, 0) == 0) return;
  const int lane = (int)(threadIdx.x & 63u);
  const int64_t item = (int64_t)blockIdx.x * kLayPassWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (item >= (int64_t)n_checks * a.ntiles) return;
  const int tile = (int)(item % a.ntiles);
  const int slot = slot0 + (int)(item / a.ntiles);
  const uint64_t dm = lay_mask(a.done, tile);
  if (dm == ~0ull) return;            // wave-uniform: the whole tile is finished
  if ((dm >> lane) & 1ull) return;    // a finished (or padding) lane loads and stores nothing
  const int e0 = sload(a.rec, 2 * slot), d = sload(a.rec, 2 * slot + 1);
  const size_t ldb = (size_t)a.ntiles * kLayTile;
  const size_t col = (size_t)tile * kLayTile + (size_t)lane;
  const size_t srow = (size_t)slot * ldb + col;
  switch (d) {
#define LAY_CASE(D) case D: lay_cn_rows<D>(a, e0, srow, col, ldb); break;
    LAY_CASES_16
#undef LAY_CASE
    default: break;
  }
}
__global__ __launch_bounds__(64 * kLayPassWaves) void lay_layer_wide(const LayPassArgs a, uint32_t* PO, int slot0,
                                                                     int n_checks) {
  if (sload(a.running, 0) == 0) return;
  const int lane = (int)(threadIdx.x & 63u);
  const int64_t item = (int64_t)blockIdx.x * kLayPassWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (item >= (int64_t)n_checks * a.ntiles) return;
  const int tile = (int)(item % a.ntiles);
  const int slot = slot0 + (int)(item / a.ntiles);
  const uint64_t dm = lay_mask(a.done, tile);
  if (dm == ~0ull) return;
  if ((dm >> lane) & 1ull) return;
  const int e0 = sload(a.rec, 2 * slot), d = sload(a.rec, 2 * slot + 1);
  const size_t ldb = (size_t)a.ntiles * kLayTile;
  const size_t tcol = (size_t)tile * kLayTile;
  const size_t srow = (size_t)slot * ldb + tcol;
  switch (d) {
#define LAY_CASE(D) case D: lay_cn_rows_wide<D>(a, PO, e0, srow, tcol, (uint32_t)lane, ldb); break;
    LAY_CASES_32
#undef LAY_CASE
    default: break;
  }
}

// Syndrome of x = (P < 0), gather form: item = (run of kLaySynRun consecutive slots, tile); a lane XORs the sign
// bits of each check's variables and ORs the checks of the run; one 64-bit atomic OR per wave, only when some
// running codeword of the tile has an unsatisfied check in the run.
__global__ __launch_bounds__(64 * kLayPassWaves) void lay_syndrome(const LayPassArgs a) {
  if (sload(a.running, 0) == 0) return;
  const int lane = (int)(threadIdx.x & 63u);
  const int64_t item = (int64_t)blockIdx.x * kLayPassWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int nruns = (a.n_c + kLaySynRun - 1) / kLaySynRun;
  if (item >= (int64_t)nruns * a.ntiles) return;
  const int tile = (int)(item % a.ntiles);
  const int run = (int)(item / a.ntiles);
  const uint64_t dm = lay_mask(a.done, tile);
  if (dm == ~0ull) return;
  const size_t ldb = (size_t)a.ntiles * kLayTile;
  const size_t col = (size_t)tile * kLayTile + (size_t)lane;
  const int s0 = run * kLaySynRun, s1 = s0 + kLaySynRun < a.n_c ? s0 + kLaySynRun : a.n_c;
  bool bad = false;
  if (!((dm >> lane) & 1ull)) {
    for (int s = s0; s < s1; ++s) {
      const int e0 = sload(a.rec, 2 * s), d = sload(a.rec, 2 * s + 1);
      bool par = false;
      for (int k = 0; k < d; ++k) par ^= a.P[(size_t)sload(a.cols, e0 + k) * ldb + col] < 0.f;
      bad |= par;
    }
  }
  const uint64_t m = __ballot(bad);
  if (m != 0ull && lane == 0) atomicOr(reinterpret_cast<unsigned long long*>(a.unsat) + tile, (unsigned long long)m);
}

// Syndrome, packed form, step 1: bits[tile][v] = ballot(P[v][lane's codeword] < 0), finished lanes 0 (never
// loaded). item = (run of 64 variables, tile); lane i keeps the word of variable v0 + i, one 512-byte store.
__global__ __launch_bounds__(64 * kLayPassWaves) void lay_pack(const LayPassArgs a) {
  if (sload(a.running, 0) == 0) return;
  const int lane = (int)(threadIdx.x & 63u);
  const int64_t item = (int64_t)blockIdx.x * kLayPassWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int nruns = (a.n_v + kLayTile - 1) / kLayTile;
  if (item >= (int64_t)nruns * a.ntiles) return;
  const int tile = (int)(item % a.ntiles);
  const int run = (int)(item / a.ntiles);
  const uint64_t dm = lay_mask(a.done, tile);
  if (dm == ~0ull) return;
  const bool live = !((dm >> lane) & 1ull);
  const size_t ldb = (size_t)a.ntiles * kLayTile;
  const size_t col = (size_t)tile * kLayTile + (size_t)lane;
  const int v0 = run * kLayTile, n = a.n_v - v0 < kLayTile ? a.n_v - v0 : kLayTile;
  uint64_t mine = 0ull;
#pragma unroll 8
  for (int i = 0; i < n; ++i) {
    bool neg = false;
    if (live) neg = a.P[(size_t)(v0 + i) * ldb + col] < 0.f;
    const uint64_t w = __ballot(neg);
    if (lane == i) mine = w;
  }
  if (lane < n) a.bits[(size_t)tile * (size_t)a.n_v + (size_t)(v0 + lane)] = mine;
}

// Step 2: item = (run of 64 consecutive slots, tile), lane = check: the XOR of the packed words of the check's
// variables is the set of codewords that leave it unsatisfied; OR over the wave, one 64-bit atomic OR when
// non-zero. (The variable indices are per-lane loads here: a lane owns a check, not a codeword.)
__global__ __launch_bounds__(64 * kLayPassWaves) void lay_syndrome_packed(const LayPassArgs a) {
  if (sload(a.running, 0) == 0) return;
  const int lane = (int)(threadIdx.x & 63u);
  const int64_t item = (int64_t)blockIdx.x * kLayPassWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int nruns = (a.n_c + kLayTile - 1) / kLayTile;
  if (item >= (int64_t)nruns * a.ntiles) return;
  const int tile = (int)(item % a.ntiles);
  const int run = (int)(item / a.ntiles);
  const uint64_t dm = lay_mask(a.done, tile);
  if (dm == ~0ull) return;
  const uint64_t* bits = a.bits + (size_t)tile * (size_t)a.n_v;
  const int s = run * kLayTile + lane;
  uint64_t w = 0ull;
  if (s < a.n_c) {
    const int e0 = a.rec[2 * s], d = a.rec[2 * s + 1];
    for (int k = 0; k < d; ++k) w ^= bits[a.cols[e0 + k]];
  }
  w &= ~dm;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) w |= (uint64_t)__shfl_xor((unsigned long long)w, off);
  if (w != 0ull && lane == 0) atomicOr(reinterpret_cast<unsigned long long*>(a.unsat) + tile, (unsigned long long)w);
}

// One wave per tile: running codewords whose syndrome is zero are finished at iteration `it`.
// kCompact: the codeword in column col is the caller's orig[col].
namespace {
template <bool kCompact>
__device__ __forceinline__ void lay_finalise_body(const LayPassArgs& a, int it, const LayCompactArgs* c) {
  if (sload(a.running, 0) == 0) return;
  const int lane = (int)(threadIdx.x & 63u);
  const int tile = (int)blockIdx.x * kLayPassWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (tile >= a.ntiles) return;
  const uint64_t dm = lay_mask(a.done, tile), um = lay_mask(a.unsat, tile);
  const uint64_t now = ~dm & ~um;
  if (a.iters && ((now >> lane) & 1ull)) {
    if constexpr (kCompact) a.iters[c->orig[tile * kLayTile + lane]] = it;
    else a.iters[tile * kLayTile + lane] = it;
  }
  if (lane == 0) {
    if (now != 0ull) {
      a.done[tile] = dm | now;
      atomicSub(a.running, (int)__popcll(now));
    }
    if (um != 0ull) a.unsat[tile] = 0ull;
  }
}
}  // namespace

__global__ __launch_bounds__(64 * kLayPassWaves) void lay_finalise(const LayPassArgs a, int it) {
  lay_finalise_body<false>(a, it, nullptr);
}
__global__ __launch_bounds__(64 * kLayPassWaves) void lay_finalise_c(const LayPassArgs a, const LayCompactArgs c,
                                                                     int it) {
  lay_finalise_body<true>(a, it, &c);
}

// out[row][b] = P[row][b] for b < B (padding lanes never reach the caller); item = (row < n_v, tile)
__global__ __launch_bounds__(64 * kLayPassWaves) void lay_stage_out(const LayPassArgs a, float* __restrict__ out) {
  const int lane = (int)(threadIdx.x & 63u);
  const int64_t item = (int64_t)blockIdx.x * kLayPassWaves + (int64_t)(threadIdx.x >> 6);
  if (item >= (int64_t)a.n_v * a.ntiles) return;
  const int tile = (int)(item % a.ntiles);
  const int64_t row = item / a.ntiles;
  const int b = tile * kLayTile + lane;
  if (b < a.B) out[(size_t)row * (size_t)a.B + (size_t)b] = a.P[(size_t)row * (size_t)a.ntiles * kLayTile + (size_t)b];
}
// With compaction: out[row][orig[c]] = P[row][c] for the columns c < extent still in use, running or finished
// since the last compaction; the codewords dropped by a compaction were delivered then.
__global__ __launch_bounds__(64 * kLayPassWaves) void lay_stage_out_c(const LayPassArgs a, const LayCompactArgs c) {
  const int lane = (int)(threadIdx.x & 63u);
  const int64_t item = (int64_t)blockIdx.x * kLayPassWaves + (int64_t)(threadIdx.x >> 6);
  if (item >= (int64_t)a.n_v * a.ntiles) return;
  const int tile = (int)(item % a.ntiles);
  const int64_t row = item / a.ntiles;
  const int extent = sload(c.ctl, kLayCtlExtent);   // <= B
  const int b = tile * kLayTile + lane;
  if (b < extent)
    c.out[(size_t)row * (size_t)a.B + (size_t)c.orig[b]] = a.P[(size_t)row * (size_t)a.ntiles * kLayTile + (size_t)b];
}

// ---- compaction of the running codewords (layered_plan.h "compaction"; include/ibldpc.h) -------------------------
// Attempted after lay_finalise of an iteration: three launches, plan / rows / commit. The plan decides on the device
// (layered_plan.h compact_wanted) and says so in the `do` word; the other two leave at once when it is 0. Nothing
// waits for another workgroup: the three are ordered by the stream, and inside the row move a row belongs to one
// wave. After the commit the running codewords are columns 0 .. R - 1 in their former order, extent = R, the
// finished masks say "finished" for every column >= R, and every tile past ceil(R / 64) is skipped by the kernels
// above as a finished tile always was. orig[c] names the caller's column of the codeword in column c.

// One workgroup: dest[c] for c < extent (layered_plan.h compact_rank). Each wave scans the 64 tile counts of a
// chunk of tiles itself (no LDS, no barrier) and writes every fourth tile of the chunk.
__global__ __launch_bounds__(64 * kLayPassWaves) void lay_compact_plan(const LayPassArgs a, const LayCompactArgs c) {
  const int R = sload(a.running, 0);
  if (R == 0) return;   // `do` is 0: stage-in and every commit leave it so
  const int E = sload(c.ctl, kLayCtlExtent);
  if (!compact_wanted(R, E, c.min_free_pct)) {
    if (threadIdx.x == 0) c.ctl[kLayCtlDo] = 0;
    return;
  }
  const int lane = (int)(threadIdx.x & 63u);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int tE = (E + kLayTile - 1) / kLayTile;   // <= ntiles: the masks and dest hold them
  int below = 0;                                  // running columns of the tiles before the chunk
  for (int t0 = 0; t0 < tE; t0 += 64) {
    const int t = t0 + lane;
    const uint64_t dm = t < tE ? a.done[t] : ~0ull;
    const int cnt = compact_tile_count(dm);
    int inc = cnt;   // inclusive scan over the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int v = __shfl_up(inc, off);
      if (lane >= off) inc += v;
    }
    const int excl = below + inc - cnt;
    for (int j = wave; j < 64 && t0 + j < tE; j += kLayPassWaves) {
      const uint64_t dj = (uint64_t)__shfl((unsigned long long)dm, j);
      const int bj = __shfl(excl, j);
      const int col = (t0 + j) * kLayTile + lane;
      if (col < E) c.dest[col] = compact_rank(dj, lane, bj);
    }
    below += __shfl(inc, 63);
  }
  if (threadIdx.x == 0) c.ctl[kLayCtlDo] = 1;
}

// The row move, in place. item = row of P (n_v), then of M1, M2, PS (n_c each); one wave owns the row and walks its
// source columns c < extent in ascending chunks of kLayCompactChunk x 64: it loads the chunk, waits for the loads,
// then stores — a running element to row[dest[c]], a finished element of a P row to out[row][orig[c]] (the
// codeword leaves the decoder here), finished state elements nowhere.
// Why in place is safe: the map is stable, dest[c] <= c, so every destination of a chunk lies at or below the
// chunk's last source, and the sources of every later chunk lie above it. A store can therefore only hit a source
// of its own chunk or of an earlier one, and all of those were loaded before the chunk's first store: load, wait,
// store per chunk in ascending order is the whole argument. Destinations are distinct, so stores do not collide.
// kWide: the rows of PO, the wide handle's fourth state array, move too.
constexpr int kLayCompactChunk = 4;
namespace {
template <bool kWide>
// (the arguments by value, as the kernels have them: by reference the narrow kernel's scalar allocation changes)
__device__ __forceinline__ void lay_compact_rows_body(const LayPassArgs a, const LayCompactArgs c, uint32_t* PO) {
  if (sload(c.ctl, kLayCtlDo) == 0) return;
  const int lane = (int)(threadIdx.x & 63u);
  const int64_t item = (int64_t)blockIdx.x * kLayPassWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (item >= (int64_t)a.n_v + (kWide ? 4 : 3) * (int64_t)a.n_c) return;
  const int E = sload(c.ctl, kLayCtlExtent);
  const size_t ldb = (size_t)a.ntiles * kLayTile;
  const bool is_p = item < a.n_v;
  // rows move as 32-bit words whatever they hold; no __restrict__: sources and destinations share the row
  uint32_t* row;
  uint32_t* orow = nullptr;
  if (is_p) {
    row = reinterpret_cast<uint32_t*>(a.P) + (size_t)item * ldb;
    orow = reinterpret_cast<uint32_t*>(c.out) + (size_t)item * (size_t)a.B;
  } else {
    const int64_t r = item - a.n_v;
    const int which = (int)(r / a.n_c);
    uint32_t* base = which == 0 ? reinterpret_cast<uint32_t*>(a.M1) : which == 1 ? reinterpret_cast<uint32_t*>(a.M2) : a.PS;
    if constexpr (kWide) base = which == 3 ? PO : base;
    row = base + (size_t)(r % a.n_c) * ldb;
  }
  for (int c0 = 0; c0 < E; c0 += kLayCompactChunk * kLayTile) {
    uint32_t x[kLayCompactChunk];
    int d[kLayCompactChunk];
    bool move[kLayCompactChunk];
#pragma unroll
    for (int j = 0; j < kLayCompactChunk; ++j) {
      const int col = c0 + j * kLayTile + lane;
      d[j] = -1;
      x[j] = 0u;
      move[j] = false;
      if (col < E) {
        d[j] = c.dest[col];
        move[j] = d[j] >= 0 ? d[j] != col : is_p;   // a running element already in place stays
        if (move[j]) x[j] = row[col];
      }
    }
    __builtin_amdgcn_s_waitcnt(0);   // every load of the chunk has returned before its first store
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < kLayCompactChunk; ++j) {
      if (!move[j]) continue;
      if (d[j] >= 0) row[d[j]] = x[j];
      else orow[c.orig[c0 + j * kLayTile + lane]] = x[j];
    }
  }
}
}  // namespace

__global__ __launch_bounds__(64 * kLayPassWaves) void lay_compact_rows(const LayPassArgs a, const LayCompactArgs c) {
  lay_compact_rows_body<false>(a, c, nullptr);
}
__global__ __launch_bounds__(64 * kLayPassWaves) void lay_compact_rows_wide(const LayPassArgs a, const LayCompactArgs c,
                                                                            uint32_t* PO) {
  lay_compact_rows_body<true>(a, c, PO);
}

// One workgroup: orig follows the move (orig[dest[c]] = orig[c], by the row move's ascending chunk rule with a
// workgroup barrier between a chunk's loads and its stores), the finished masks of the new extent, and the words.
__global__ __launch_bounds__(64 * kLayPassWaves) void lay_compact_commit(const LayPassArgs a, const LayCompactArgs c) {
  if (sload(c.ctl, kLayCtlDo) == 0) return;
  const int E = sload(c.ctl, kLayCtlExtent), R = sload(a.running, 0), n = sload(c.ctl, kLayCtlCount);
  const int tid = (int)threadIdx.x;
  for (int c0 = 0; c0 < E; c0 += 64 * kLayPassWaves) {   // E is uniform: every thread meets every barrier
    const int col = c0 + tid;
    int d = -1, o = 0;
    if (col < E) {
      d = c.dest[col];
      if (d >= 0) o = c.orig[col];
    }
    __syncthreads();
    if (d >= 0 && d != col) c.orig[d] = o;
  }
  const int tE = (E + kLayTile - 1) / kLayTile;
  for (int t = tid; t < tE; t += 64 * kLayPassWaves) {
    a.done[t] = compact_done_word(t, R);
    a.unsat[t] = 0ull;
  }
  __syncthreads();   // every wave has read the words before they change
  if (tid == 0) {
    c.ctl[kLayCtlExtent] = R;
    c.ctl[kLayCtlCount] = n + 1;
    c.ctl[kLayCtlDo] = 0;
  }
}

namespace {
bool lay_pass_args_ok(const LayPassArgs& a) {
  return a.P && a.M1 && a.M2 && a.PS && a.done && a.unsat && a.running && a.rec && a.cols && a.n_v >= 1 &&
         a.n_c >= 1 && a.B >= 1 && a.ntiles == pass_tiles(a.B);
}
hipError_t lay_pass_launch(const void* f, int64_t items, void** p, hipStream_t s) {
  const int64_t grid = (items + kLayPassWaves - 1) / kLayPassWaves;
  if (grid < 1 || grid > 0x7fffffffll) return hipErrorInvalidValue;
  return hipLaunchKernel(f, dim3((unsigned)grid), dim3(64 * kLayPassWaves), p, 0, s);
}
bool lay_compact_args_ok(const LayCompactArgs& c) {
  return c.orig && c.dest && c.ctl && c.out && c.min_free_pct >= 1 && c.min_free_pct <= 100;
}
// the largest private (scratch) segment over `kernels`
hipError_t lay_private_bytes(std::initializer_list<const void*> kernels, size_t* bytes) {
  *bytes = 0;
  for (const void* f : kernels) {
    hipFuncAttributes fa;
    const hipError_t e = hipFuncGetAttributes(&fa, f);
    if (e != hipSuccess) return e;
    *bytes = std::max(*bytes, (size_t)fa.localSizeBytes);
  }
  return hipSuccess;
}
}  // namespace

// The launchers that touch the check state take the wide handle's added array (PO here, S1 in fixed point) and
// launch the wide kernel when it is there; nullptr is a narrow handle. The kernels receive it after the structs.
hipError_t launch_lay_stage_in(const LayPassArgs& a, const LayCompactArgs* c, uint32_t* PO, const float* llr,
                               int imax, hipStream_t s) {
  if (!lay_pass_args_ok(a) || !llr || (c && !lay_compact_args_ok(*c))) return hipErrorInvalidValue;
  LayPassArgs args = a;
  LayCompactArgs ca = c ? *c : LayCompactArgs{};
  void* p[5];
  int n = 0;
  p[n++] = &args;
  if (c) p[n++] = &ca;
  if (PO) p[n++] = (void*)&PO;
  p[n++] = (void*)&llr;
  p[n++] = (void*)&imax;
  const void* f = c ? (PO ? (const void*)lay_stage_in_c_wide : (const void*)lay_stage_in_c)
                    : (PO ? (const void*)lay_stage_in_wide : (const void*)lay_stage_in);
  return lay_pass_launch(f, (int64_t)std::max(a.n_v, a.n_c) * a.ntiles, p, s);
}

hipError_t launch_lay_layer(const LayPassArgs& a, uint32_t* PO, int slot0, int n_checks, hipStream_t s) {
  if (!lay_pass_args_ok(a) || slot0 < 0 || n_checks < 0 || (int64_t)slot0 + n_checks > a.n_c)
    return hipErrorInvalidValue;
  if (n_checks == 0) return hipSuccess;
  LayPassArgs args = a;
  void* pn[] = {&args, (void*)&slot0, (void*)&n_checks};
  void* pw[] = {&args, (void*)&PO, (void*)&slot0, (void*)&n_checks};
  return lay_pass_launch(PO ? (const void*)lay_layer_wide : (const void*)lay_layer, pass_items(n_checks, a.B),
                         PO ? pw : pn, s);
}

hipError_t launch_lay_syndrome(const LayPassArgs& a, int packed, hipStream_t s) {
  if (!lay_pass_args_ok(a) || (packed && !a.bits)) return hipErrorInvalidValue;
  LayPassArgs args = a;
  void* p[] = {&args};
  if (!packed) return lay_pass_launch((const void*)lay_syndrome, pass_items(pass_syn_runs(a.n_c), a.B), p, s);
  const hipError_t e = lay_pass_launch((const void*)lay_pack, pass_items(pass_pack_runs(a.n_v), a.B), p, s);
  if (e != hipSuccess) return e;
  return lay_pass_launch((const void*)lay_syndrome_packed, pass_items(pass_pack_runs(a.n_c), a.B), p, s);
}

hipError_t launch_lay_syndrome_finalise(const LayPassArgs& a, int it, hipStream_t s) {
  if (!a.done || !a.unsat || !a.running || !a.bits || !a.rec || !a.cols || a.n_v < 1 || a.n_c < 1 || a.B < 1 ||
      a.ntiles != pass_tiles(a.B))
    return hipErrorInvalidValue;
  LayPassArgs args = a;
  void* ps[] = {&args};
  const hipError_t e = lay_pass_launch((const void*)lay_syndrome_packed, pass_items(pass_pack_runs(a.n_c), a.B), ps, s);
  if (e != hipSuccess) return e;
  void* pf[] = {&args, (void*)&it};
  return lay_pass_launch((const void*)lay_finalise, a.ntiles, pf, s);
}

hipError_t launch_lay_finalise(const LayPassArgs& a, int it, hipStream_t s) {
  if (!lay_pass_args_ok(a)) return hipErrorInvalidValue;
  LayPassArgs args = a;
  void* p[] = {&args, (void*)&it};
  return lay_pass_launch((const void*)lay_finalise, a.ntiles, p, s);
}

hipError_t launch_lay_stage_out(const LayPassArgs& a, float* out, hipStream_t s) {
  if (!lay_pass_args_ok(a) || !out) return hipErrorInvalidValue;
  LayPassArgs args = a;
  void* p[] = {&args, (void*)&out};
  return lay_pass_launch((const void*)lay_stage_out, (int64_t)a.n_v * a.ntiles, p, s);
}

hipError_t launch_lay_finalise_c(const LayPassArgs& a, const LayCompactArgs& c, int it, hipStream_t s) {
  if (!lay_pass_args_ok(a) || !lay_compact_args_ok(c)) return hipErrorInvalidValue;
  LayPassArgs args = a;
  LayCompactArgs ca = c;
  void* p[] = {&args, &ca, (void*)&it};
  return lay_pass_launch((const void*)lay_finalise_c, a.ntiles, p, s);
}

hipError_t launch_lay_stage_out_c(const LayPassArgs& a, const LayCompactArgs& c, hipStream_t s) {
  if (!lay_pass_args_ok(a) || !lay_compact_args_ok(c)) return hipErrorInvalidValue;
  LayPassArgs args = a;
  LayCompactArgs ca = c;
  void* p[] = {&args, &ca};
  return lay_pass_launch((const void*)lay_stage_out_c, (int64_t)a.n_v * a.ntiles, p, s);
}

// PO: the row move then covers the four state arrays
hipError_t launch_lay_compact(const LayPassArgs& a, const LayCompactArgs& c, uint32_t* PO, hipStream_t s) {
  if (!lay_pass_args_ok(a) || !lay_compact_args_ok(c)) return hipErrorInvalidValue;
  LayPassArgs args = a;
  LayCompactArgs ca = c;
  void* p[] = {&args, &ca, (void*)&PO};   // the narrow kernels take the first two
  hipError_t e = hipLaunchKernel((const void*)lay_compact_plan, dim3(1), dim3(64 * kLayPassWaves), p, 0, s);
  if (e != hipSuccess) return e;
  const void* rows = PO ? (const void*)lay_compact_rows_wide : (const void*)lay_compact_rows;
  if ((e = lay_pass_launch(rows, pass_compact_rows(a.n_v, a.n_c, PO != nullptr), p, s)) != hipSuccess) return e;
  return hipLaunchKernel((const void*)lay_compact_commit, dim3(1), dim3(64 * kLayPassWaves), p, 0, s);
}

// The create-time guards: every kernel here is built to run without a private (scratch) segment.
hipError_t lay_compact_private_bytes(size_t* bytes) {
  return lay_private_bytes({(const void*)lay_stage_in_c, (const void*)lay_finalise_c, (const void*)lay_stage_out_c,
                            (const void*)lay_compact_plan, (const void*)lay_compact_rows,
                            (const void*)lay_compact_commit},
                           bytes);
}
hipError_t lay_pass_private_bytes(size_t* bytes) {
  return lay_private_bytes({(const void*)lay_stage_in, (const void*)lay_layer, (const void*)lay_syndrome,
                            (const void*)lay_pack, (const void*)lay_syndrome_packed, (const void*)lay_finalise,
                            (const void*)lay_stage_out},
                           bytes);
}

// ---------------------------------------------------------------------------------------------------------------
// Fixed point, per-layer path over HBM (include/ibldpc.h "Layered min-sum, fixed point").
//
// Integer arithmetic throughout, plain C++ per codeword. A lane owns 4 consecutive codewords: P[n_v][ldb] int8 is
// one dword per row and lane, the check state S[n_c][ldb] one 32-bit word per codeword (fix_state_word: two 6-bit
// corrected magnitudes, the first argmin position, the sign bits of R with edge k at bit k), a lane's four words one
// 16-byte access; ldb = 256 ntiles4. One launch per layer, a wave item (check of the layer, tile of 256
// codewords); the check's record and variable indices are wave-uniform scalar loads as in lay_layer.
//
// The stop is the fp32 path's: done / unsat masks and packed hard decisions per 64 codewords (layfix_pack makes the
// latter from the int8 rows, lay_syndrome_packed and lay_finalise are launched unchanged). The mask words of a
// tile of 256 past the batch are all ones. A lane whose four codewords are finished leaves before its first vector
// load; a lane with some finished stores their bytes and state words back unchanged.
namespace {

__device__ __forceinline__ uint32_t layfix_sign_nibble(uint32_t w) {   // bit i = sign of byte i
  return (((w >> 7) & 0x01010101u) * 0x01020408u) >> 24;
}

// finished bits of the lane's 4 codewords (bit j: codeword 4 lane + j of the tile); *all: the whole tile is finished
__device__ __forceinline__ uint32_t layfix_finished(const uint64_t* done, int tile4, int lane, bool* all) {
  const uint64_t d0 = lay_mask(done, 4 * tile4), d1 = lay_mask(done, 4 * tile4 + 1),
                 d2 = lay_mask(done, 4 * tile4 + 2), d3 = lay_mask(done, 4 * tile4 + 3);
  *all = (d0 & d1 & d2 & d3) == ~0ull;
  const int sub = lane >> 4;
  const uint64_t dm = sub == 0 ? d0 : sub == 1 ? d1 : sub == 2 ? d2 : d3;
  return (uint32_t)(dm >> ((lane & 15) * 4)) & 0xFu;
}

// The fixed-point check update of one check of degree D and ONE codeword, the one statement of it for both layer
// kernels: codeword j of the lane's four, whose APP values are byte j of the row dwords p[D]. Both kernels load the
// rows into registers first and store them after the fourth codeword, so the core takes them as they are: there is no
// memory access to place, as lay_minsum's callables do. In: the corrected minima m1s, m2s
// (6 bits), the first argmin position and the sign bits of R of the previous iteration, edge k at bit k of `signs`
// (higher bits are ignored); out: those of this one. Plain integer C++ (include/ibldpc.h "Layered min-sum, fixed
// point"): messages saturate at q_max, the correction is (alpha16 m + 8) >> 4 less beta_q, floored at 0; the
// position moves only on m < m1, so it is the FIRST position attaining the minimum; P saturates at 127.
template <int D>
__device__ __forceinline__ void layfix_minsum(uint32_t (&p)[D], int j, int& m1s, int& m2s, uint32_t& pos,
                                              uint32_t& signs, int alpha16, int beta, int qm) {
  static_assert(D >= kLayMinD && D <= kLayWideMaxD, "degree body out of range");
  const int m1o = m1s, m2o = m2s;
  const uint32_t poso = pos, so = signs;
  int t[D];
  int m1 = kLayFixQMax + 1, m2 = kLayFixQMax + 1;
  uint32_t at = 0, neg = 0;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const int mag = (uint32_t)k == poso ? m2o : m1o;
    const int r = ((so >> k) & 1u) ? -mag : mag;
    const int x = (int)(int8_t)(p[k] >> (8 * j)) - r;
    t[k] = x;
    neg |= ((uint32_t)x >> 31) << k;
    const int m = min(abs(x), qm);
    at = m < m1 ? (uint32_t)k : at;
    m2 = min(m2, max(m1, m));
    m1 = min(m1, m);
  }
  const int m1n = max(((alpha16 * m1 + 8) >> 4) - beta, 0), m2n = max(((alpha16 * m2 + 8) >> 4) - beta, 0);
  // s ^ neg_e: R[e] is negated; fix_wide_mask: the low D bits, defined at D = 32 too
  const uint32_t sg = ((__popc(neg) & 1) ? ~neg : neg) & fix_wide_mask(D);
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const int mag = (uint32_t)k == at ? m2n : m1n;
    const int r = ((sg >> k) & 1u) ? -mag : mag;
    const int pn = min(max(t[k] + r, -kLayFixApp), kLayFixApp);
    p[k] = (p[k] & ~(0xFFu << (8 * j))) | ((uint32_t)(pn & 0xFF) << (8 * j));
  }
  m1s = m1n;
  m2s = m2n;
  pos = at;
  signs = sg;
}

// One check of degree D for the lane's 4 codewords, narrow handle: bytes at `col` of every P row, words at srow of
// S (fix_state_word), a 64-bit element index per edge.
template <int D>
__device__ __forceinline__ void layfix_cn_rows(const LayFixArgs& a, int e0, size_t srow, size_t col, size_t ldb,
                                               uint32_t fin) {
  static_assert(D <= kLayMaxD, "degree body out of range");
  size_t v[D];
#pragma unroll
  for (int k = 0; k < D; ++k) v[k] = (size_t)sload(a.cols, e0 + k) * ldb + col;
  uint32_t p[D];
#pragma unroll
  for (int k = 0; k < D; ++k) p[k] = *reinterpret_cast<const uint32_t*>(a.P + v[k]);
  const uint4 st = *reinterpret_cast<const uint4*>(a.S + srow);
  uint32_t w[kLayFixCw] = {st.x, st.y, st.z, st.w};
  const int alpha16 = a.alpha16, beta = a.beta_q, qm = a.q_max;
#pragma unroll
  for (int j = 0; j < kLayFixCw; ++j) {
    if ((fin >> j) & 1u) continue;   // frozen at its stop iteration
    int m1 = (int)((w[j] >> 20) & 63u), m2 = (int)(w[j] >> 26);
    uint32_t pos = (w[j] >> 16) & 15u, sg = w[j];
    layfix_minsum<D>(p, j, m1, m2, pos, sg, alpha16, beta, qm);
    w[j] = fix_state_word((uint32_t)m1, (uint32_t)m2, pos, sg);
  }
#pragma unroll
  for (int k = 0; k < D; ++k) *reinterpret_cast<uint32_t*>(a.P + v[k]) = p[k];
  *reinterpret_cast<uint4*>(a.S + srow) = make_uint4(w[0], w[1], w[2], w[3]);
}

// The same for a wide handle: the two state words of fix_state_words_wide in S and S1. tcol, srow: wave-uniform as
// in lay_cn_rows_wide; the lane's four codewords are dword `lane` of a P row's tile and words 4 lane .. 4 lane + 3
// of a state row's.
template <int D>
__device__ __forceinline__ void layfix_cn_rows_wide(const LayFixArgs& a, uint32_t* __restrict__ S1, int e0,
                                                    size_t srow, size_t tcol, uint32_t lane, size_t ldb,
                                                    uint32_t fin) {
  const auto row = [&](int k) {
    return reinterpret_cast<uint32_t*>(a.P + ((size_t)sload(a.cols, e0 + k) * ldb + tcol));
  };
  uint32_t p[D];
#pragma unroll
  for (int k = 0; k < D; ++k) p[k] = row(k)[lane];
  const uint4 st0 = reinterpret_cast<const uint4*>(a.S + srow)[lane], st1 = reinterpret_cast<const uint4*>(S1 + srow)[lane];
  uint32_t w0[kLayFixCw] = {st0.x, st0.y, st0.z, st0.w}, w1[kLayFixCw] = {st1.x, st1.y, st1.z, st1.w};
  const int alpha16 = a.alpha16, beta = a.beta_q, qm = a.q_max;
#pragma unroll
  for (int j = 0; j < kLayFixCw; ++j) {
    if ((fin >> j) & 1u) continue;   // frozen at its stop iteration
    int m1 = (int)fix_wide_m1(w0[j]), m2 = (int)fix_wide_m2(w0[j]);
    uint32_t pos = fix_wide_pos(w0[j]), sg = w1[j];
    layfix_minsum<D>(p, j, m1, m2, pos, sg, alpha16, beta, qm);
    const FixWideWords w = fix_state_words_wide((uint32_t)m1, (uint32_t)m2, pos, sg);
    w0[j] = w.w0;
    w1[j] = w.w1;
  }
#pragma unroll
  for (int k = 0; k < D; ++k) row(k)[lane] = p[k];
  reinterpret_cast<uint4*>(a.S + srow)[lane] = make_uint4(w0[0], w0[1], w0[2], w0[3]);
  reinterpret_cast<uint4*>(S1 + srow)[lane] = make_uint4(w1[0], w1[1], w1[2], w1[3]);
}

}  // namespace

// P = the quantised (IBL_F32) or copied (IBL_I8, -128 -> -127) channel values, padding codewords 0; state words 0;
// masks, counter and iters reset. item = (row < max(n_v, n_c), tile of 256). kWide: also the words of S1, the wide
// handle's second state array.
namespace {
template <bool kWide>
__device__ __forceinline__ void layfix_stage_in_body(const LayFixArgs& a, uint32_t* S1, const void* __restrict__ llr,
                                                     int dtype, int imax) {
  const int lane = (int)(threadIdx.x & 63u);
  const int64_t item = (int64_t)blockIdx.x * kLayPassWaves + (int64_t)(threadIdx.x >> 6);
  const int64_t rows = a.n_v > a.n_c ? a.n_v : a.n_c;
  if (item >= rows * a.ntiles4) return;
  const int tile = (int)(item % a.ntiles4);
  const int64_t row = item / a.ntiles4;
  const size_t ldb = (size_t)a.ntiles4 * kLayFixTile;
  const int b0 = tile * kLayFixTile + kLayFixCw * lane;
  const size_t at = (size_t)row * ldb + (size_t)b0;
  if (row < a.n_v) {
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < kLayFixCw; ++j) {
      int x = 0;
      if (b0 + j < a.B) {
        const size_t src = (size_t)row * (size_t)a.B + (size_t)(b0 + j);
        if (dtype == kF32) {
          // one rounded product, rint to even, clamped as a float, then converted
          const float f = __builtin_rintf(static_cast<const float*>(llr)[src] * a.scale);
          x = (int)fminf(fmaxf(f, -(float)kLayFixApp), (float)kLayFixApp);
        } else {
          x = max((int)static_cast<const int8_t*>(llr)[src], -kLayFixApp);
        }
      }
      w |= (uint32_t)(x & 0xFF) << (8 * j);
    }
    *reinterpret_cast<uint32_t*>(a.P + at) = w;
  }
  if (row < a.n_c) {
    *reinterpret_cast<uint4*>(a.S + at) = make_uint4(0u, 0u, 0u, 0u);
    if constexpr (kWide) *reinterpret_cast<uint4*>(S1 + at) = make_uint4(0u, 0u, 0u, 0u);
  }
  if (row == 0) {
    if (a.iters) {
#pragma unroll
      for (int j = 0; j < kLayFixCw; ++j)
        if (b0 + j < a.B) a.iters[b0 + j] = imax;
    }
    if (lane < kLayFixCw) {
      const int t64 = kLayFixCw * tile + lane;
      const int left = a.B - t64 * kLayTile;   // <= 0: a mask word past the batch
      a.done[t64] = left >= kLayTile ? 0ull : left <= 0 ? ~0ull : ~0ull << left;
      a.unsat[t64] = 0ull;
    }
    if (lane == 0 && tile == 0) *a.running = a.B;
  }
}
}  // namespace

__global__ __launch_bounds__(64 * kLayPassWaves) void layfix_stage_in(const LayFixArgs a, const void* __restrict__ llr,
                                                                      int dtype, int imax) {
  layfix_stage_in_body<false>(a, nullptr, llr, dtype, imax);
}
__global__ __launch_bounds__(64 * kLayPassWaves) void layfix_stage_in_wide(const LayFixArgs a, uint32_t* S1,
                                                                           const void* __restrict__ llr, int dtype,
                                                                           int imax) {
  layfix_stage_in_body<true>(a, S1, llr, dtype, imax);
}

// One layer: item = (check slot0 + c of the layer, tile of 256); narrow and wide as lay_layer and lay_layer_wide
__global__ __launch_bounds__(64 * kLayPassWaves) void layfix_layer(const LayFixArgs a, int slot0, int n_checks) {
  if (sload(a.running, 0) == 0) return;
  const int lane = (int)(threadIdx.x & 63u);
  const int64_t item = (int64_t)blockIdx.x * kLayPassWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (item >= (int64_t)n_checks * a.ntiles4) return;
  const int tile = (int)(item % a.ntiles4);
  const int slot = slot0 + (int)(item / a.ntiles4);
  bool all;
  const uint32_t fin = layfix_finished(a.done, tile, lane, &all);
  if (all) return;             // wave-uniform: the whole tile is finished
  if (fin == 0xFu) return;     // the lane's four codewords are finished (or padding)
  const int e0 = sload(a.rec, 2 * slot), d = sload(a.rec, 2 * slot + 1);
  const size_t ldb = (size_t)a.ntiles4 * kLayFixTile;
  const size_t col = (size_t)tile * kLayFixTile + (size_t)(kLayFixCw * lane);
  const size_t srow = (size_t)slot * ldb + col;
  switch (d) {
#define LAY_CASE(D) case D: layfix_cn_rows<D>(a, e0, srow, col, ldb, fin); break;
    LAY_CASES_16
#undef LAY_CASE
    default: break;
  }
}
__global__ __launch_bounds__(64 * kLayPassWaves) void layfix_layer_wide(const LayFixArgs a, uint32_t* S1, int slot0,
                                                                        int n_checks) {
  if (sload(a.running, 0) == 0) return;
  const int lane = (int)(threadIdx.x & 63u);
  const int64_t item = (int64_t)blockIdx.x * kLayPassWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (item >= (int64_t)n_checks * a.ntiles4) return;
  const int tile = (int)(item % a.ntiles4);
  const int slot = slot0 + (int)(item / a.ntiles4);
  bool all;
  const uint32_t fin = layfix_finished(a.done, tile, lane, &all);
  if (all) return;
  if (fin == 0xFu) return;
  const int e0 = sload(a.rec, 2 * slot), d = sload(a.rec, 2 * slot + 1);
  const size_t ldb = (size_t)a.ntiles4 * kLayFixTile;
  const size_t tcol = (size_t)tile * kLayFixTile;
  const size_t srow = (size_t)slot * ldb + tcol;
  switch (d) {
#define LAY_CASE(D) case D: layfix_cn_rows_wide<D>(a, S1, e0, srow, tcol, (uint32_t)lane, ldb, fin); break;
    LAY_CASES_32
#undef LAY_CASE
    default: break;
  }
}

// Hard decisions of the int8 rows in lay_pack's form: bits[tile][v] bit b = (P[v][64 tile + b] < 0), finished
// codewords 0. item = (run of 64 variables, tile of 64); lane i reads the 64 bytes of variable v0 + i.
__global__ __launch_bounds__(64 * kLayPassWaves) void layfix_pack(const LayFixArgs a) {
  if (sload(a.running, 0) == 0) return;
  const int lane = (int)(threadIdx.x & 63u);
  const int64_t item = (int64_t)blockIdx.x * kLayPassWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int nruns = (a.n_v + kLayTile - 1) / kLayTile;
  if (item >= (int64_t)nruns * a.ntiles) return;
  const int tile = (int)(item % a.ntiles);
  const int run = (int)(item / a.ntiles);
  const uint64_t dm = lay_mask(a.done, tile);
  if (dm == ~0ull) return;
  const int v = run * kLayTile + lane;
  if (v >= a.n_v) return;
  const size_t ldb = (size_t)a.ntiles4 * kLayFixTile;
  const uint4* src = reinterpret_cast<const uint4*>(a.P + (size_t)v * ldb + (size_t)tile * kLayTile);
  uint64_t word = 0ull;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint4 x = src[q];
    const uint32_t n = layfix_sign_nibble(x.x) | (layfix_sign_nibble(x.y) << 4) | (layfix_sign_nibble(x.z) << 8) |
                       (layfix_sign_nibble(x.w) << 12);
    word |= (uint64_t)n << (16 * q);
  }
  a.bits[(size_t)tile * (size_t)a.n_v + (size_t)v] = word & ~dm;
}

// out[row][b] = P[row][b] (IBL_I8) or f32(P) / scale (IBL_F32) for b < B; item = (row < n_v, tile of 256)
__global__ __launch_bounds__(64 * kLayPassWaves) void layfix_stage_out(const LayFixArgs a, void* __restrict__ out,
                                                                       int dtype) {
  const int lane = (int)(threadIdx.x & 63u);
  const int64_t item = (int64_t)blockIdx.x * kLayPassWaves + (int64_t)(threadIdx.x >> 6);
  if (item >= (int64_t)a.n_v * a.ntiles4) return;
  const int tile = (int)(item % a.ntiles4);
  const int64_t row = item / a.ntiles4;
  const int b0 = tile * kLayFixTile + kLayFixCw * lane;
  if (b0 >= a.B) return;
  const uint32_t w = *reinterpret_cast<const uint32_t*>(a.P + (size_t)row * (size_t)a.ntiles4 * kLayFixTile + (size_t)b0);
#pragma unroll
  for (int j = 0; j < kLayFixCw; ++j) {
    if (b0 + j >= a.B) break;
    const int x = (int)(int8_t)(w >> (8 * j));
    const size_t dst = (size_t)row * (size_t)a.B + (size_t)(b0 + j);
    if (dtype == kF32) static_cast<float*>(out)[dst] = (float)x / a.scale;
    else static_cast<int8_t*>(out)[dst] = (int8_t)x;
  }
}

namespace {
bool layfix_args_ok(const LayFixArgs& a) {
  return a.P && a.S && a.done && a.unsat && a.running && a.bits && a.rec && a.cols && a.n_v >= 1 && a.n_c >= 1 &&
         a.B >= 1 && a.ntiles == pass_tiles(a.B) && a.ntiles4 == fix_tiles(a.B) &&
         fix_params_ok(a.alpha16, a.beta_q, a.q_max) && a.scale > 0.f;
}
bool layfix_dtype_ok(int32_t dtype) { return dtype == kF32 || dtype == kI8; }
}  // namespace

hipError_t launch_layfix_stage_in(const LayFixArgs& a, uint32_t* S1, const void* llr, int32_t dtype, int imax,
                                  hipStream_t s) {
  if (!layfix_args_ok(a) || !llr || !layfix_dtype_ok(dtype)) return hipErrorInvalidValue;
  LayFixArgs args = a;
  void* pn[] = {&args, (void*)&llr, (void*)&dtype, (void*)&imax};
  void* pw[] = {&args, (void*)&S1, (void*)&llr, (void*)&dtype, (void*)&imax};
  return lay_pass_launch(S1 ? (const void*)layfix_stage_in_wide : (const void*)layfix_stage_in,
                         (int64_t)std::max(a.n_v, a.n_c) * a.ntiles4, S1 ? pw : pn, s);
}

hipError_t launch_layfix_layer(const LayFixArgs& a, uint32_t* S1, int slot0, int n_checks, hipStream_t s) {
  if (!layfix_args_ok(a) || slot0 < 0 || n_checks < 0 || (int64_t)slot0 + n_checks > a.n_c)
    return hipErrorInvalidValue;
  if (n_checks == 0) return hipSuccess;
  LayFixArgs args = a;
  void* pn[] = {&args, (void*)&slot0, (void*)&n_checks};
  void* pw[] = {&args, (void*)&S1, (void*)&slot0, (void*)&n_checks};
  return lay_pass_launch(S1 ? (const void*)layfix_layer_wide : (const void*)layfix_layer, fix_items(n_checks, a.B),
                         S1 ? pw : pn, s);
}

hipError_t launch_layfix_stop(const LayFixArgs& a, int it, hipStream_t s) {
  if (!layfix_args_ok(a)) return hipErrorInvalidValue;
  LayFixArgs args = a;
  void* p[] = {&args};
  hipError_t e = lay_pass_launch((const void*)layfix_pack, pass_items(pass_pack_runs(a.n_v), a.B), p, s);
  if (e != hipSuccess) return e;
  // the fp32 path's kernels read only what the two paths share
  LayPassArgs f{};
  f.done = a.done; f.unsat = a.unsat; f.running = a.running; f.bits = a.bits; f.rec = a.rec; f.cols = a.cols;
  f.iters = a.iters; f.n_v = a.n_v; f.n_c = a.n_c; f.B = a.B; f.ntiles = a.ntiles;
  void* ps[] = {&f};
  e = lay_pass_launch((const void*)lay_syndrome_packed, pass_items(pass_pack_runs(a.n_c), a.B), ps, s);
  if (e != hipSuccess) return e;
  void* pf[] = {&f, (void*)&it};
  return lay_pass_launch((const void*)lay_finalise, a.ntiles, pf, s);
}

hipError_t launch_layfix_stage_out(const LayFixArgs& a, void* out, int32_t dtype, hipStream_t s) {
  if (!layfix_args_ok(a) || !out || !layfix_dtype_ok(dtype)) return hipErrorInvalidValue;
  LayFixArgs args = a;
  void* p[] = {&args, (void*)&out, (void*)&dtype};
  return lay_pass_launch((const void*)layfix_stage_out, (int64_t)a.n_v * a.ntiles4, p, s);
}

hipError_t layfix_private_bytes(size_t* bytes) {
  return lay_private_bytes({(const void*)layfix_stage_in, (const void*)layfix_layer, (const void*)layfix_pack,
                            (const void*)layfix_stage_out},
                           bytes);
}
// the kernels only a wide handle launches
hipError_t lay_wide_private_bytes(size_t* bytes) {
  return lay_private_bytes({(const void*)lay_fused_wide, (const void*)lay_stage_in_wide,
                            (const void*)lay_stage_in_c_wide, (const void*)lay_layer_wide,
                            (const void*)lay_compact_rows_wide, (const void*)layfix_stage_in_wide,
                            (const void*)layfix_layer_wide},
                           bytes);
}

// ---------------------------------------------------------------------------------------------------------------
// Fixed point, fused on chip (include/ibldpc.h "Layered min-sum, fixed point", the fused kernel; layered_plan.h
// "fixed point, fused").
//
// lay_fused_body in integers: one wave owns one codeword, lane = check of a task, the fp32 kernel's plan, loop over
// groups and per-codeword stop. The wave's slice of LDS is P[ldn] int8 and one state word per check S[n_c]
// (fix_state_word; wide: S and S1, fix_state_words_wide), a quarter to a third of the fp32 slice. The arithmetic is
// layfix_minsum with the lane's D bytes in the low bytes of p[] and j = 0.
// P is read and written one BYTE per lane and edge (ds_read_i8 / ds_write_b8): a layer's checks share no variable,
// so no two lanes of a task touch the same byte, but they do touch different bytes of one dword in one instruction,
// which only a byte store keeps apart (a dword read-modify-write would lose the neighbours' updates).
namespace {

template <int D, bool kWide>
__device__ __forceinline__ void layfix_cn(int8_t* __restrict__ P, uint32_t* __restrict__ S, uint32_t* __restrict__ S1,
                                          const int32_t* __restrict__ idx, int slot, int alpha16, int beta, int qm) {
  static_assert(D <= (kWide ? kLayWideMaxD : kLayMaxD), "degree body out of range");
  int v[D];
#pragma unroll
  for (int k = 0; k < D; ++k) v[k] = idx[64 * k];
  uint32_t p[D];
#pragma unroll
  for (int k = 0; k < D; ++k) p[k] = (uint32_t)(int32_t)P[v[k]];
  int m1, m2;
  uint32_t pos, sg;
  if constexpr (kWide) {
    const uint32_t w0 = S[slot];
    m1 = (int)fix_wide_m1(w0);
    m2 = (int)fix_wide_m2(w0);
    pos = fix_wide_pos(w0);
    sg = S1[slot];
  } else {
    const uint32_t w = S[slot];
    m1 = (int)((w >> 20) & 63u);
    m2 = (int)(w >> 26);
    pos = (w >> 16) & 15u;
    sg = w;
  }
  layfix_minsum<D>(p, 0, m1, m2, pos, sg, alpha16, beta, qm);
#pragma unroll
  for (int k = 0; k < D; ++k) P[v[k]] = (int8_t)p[k];
  if constexpr (kWide) {
    const FixWideWords w = fix_state_words_wide((uint32_t)m1, (uint32_t)m2, pos, sg);
    S[slot] = w.w0;
    S1[slot] = w.w1;
  } else {
    S[slot] = fix_state_word((uint32_t)m1, (uint32_t)m2, pos, sg);
  }
}

template <bool kWide>
__device__ __forceinline__ void layfix_cn_any(int d, int8_t* P, uint32_t* S, uint32_t* S1, const int32_t* idx,
                                              int slot, int alpha16, int beta, int qm) {
#define LAY_CASE(D) case D: layfix_cn<D, kWide>(P, S, S1, idx, slot, alpha16, beta, qm); break;
  if constexpr (kWide) {
    switch (d) {
      LAY_CASES_32
      default: break;
    }
  } else {
    switch (d) {
      LAY_CASES_16
      default: break;
    }
  }
#undef LAY_CASE
}

template <bool kWide>
__device__ __forceinline__ void layfix_fused_body(const LayFixFusedArgs a) {
  extern __shared__ __align__(16) unsigned char lay_lds[];
  const int lane = (int)(threadIdx.x & 63u);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int ncw = a.cw_per_group;
  if (wave >= ncw) return;
  unsigned char* base = lay_lds + (size_t)wave * (size_t)a.cw_bytes;   // cw_bytes and ldn are multiples of 4
  int8_t* P = reinterpret_cast<int8_t*>(base);
  uint32_t* S = reinterpret_cast<uint32_t*>(base + a.ldn);
  uint32_t* S1 = kWide ? S + a.n_c : nullptr;
  const int alpha16 = a.alpha16, beta = a.beta_q, qm = a.q_max;
  for (int g = (int)blockIdx.x; g < a.ngroups; g += (int)gridDim.x) {
    const int b = g * ncw + wave;
    if (b >= a.B) break;   // wave-uniform; later groups of this workgroup lie further still
    int8_t* row = a.buf + (size_t)b * (size_t)a.ldn;
    for (int v = 4 * lane; v < a.ldn; v += 256)
      *reinterpret_cast<uint32_t*>(P + v) = *reinterpret_cast<const uint32_t*>(row + v);
    for (int c = lane; c < a.n_c; c += 64) {
      S[c] = 0u;
      if constexpr (kWide) S1[c] = 0u;
    }
    __builtin_amdgcn_wave_barrier();
    int it = 1;
    for (;; ++it) {
      for (int t = 0; t < a.n_tasks; ++t) {
        const int first = sload(a.task, 4 * t), cnt = sload(a.task, 4 * t + 1), d = sload(a.task, 4 * t + 2),
                  s0 = sload(a.task, 4 * t + 3);
        if (lane < cnt) layfix_cn_any<kWide>(d, P, S, S1, a.idx + first + lane, s0 + lane, alpha16, beta, qm);
        __builtin_amdgcn_wave_barrier();   // the next task's reads stay behind this task's writes (other lanes')
      }
      if (it >= a.imax) break;
      if (a.early) {
        // syndrome of the hard decisions after the complete iteration, as lay_fused_body: leaves at the first task
        // with an unsatisfied check
        bool bad = false;
        for (int t = 0; t < a.n_tasks && !bad; ++t) {
          const int first = sload(a.task, 4 * t), cnt = sload(a.task, 4 * t + 1), d = sload(a.task, 4 * t + 2);
          uint32_t par = 0;
          if (lane < cnt) {
            const int32_t* ix = a.idx + first + lane;
            for (int k = 0; k < d; ++k) par ^= (P[ix[64 * k]] < 0) ? 1u : 0u;
          }
          bad = __builtin_amdgcn_readfirstlane((int)(__ballot(par != 0) != 0ull)) != 0;
        }
        if (!bad) break;
      }
    }
    for (int v = 4 * lane; v < a.ldn; v += 256)
      *reinterpret_cast<uint32_t*>(row + v) = *reinterpret_cast<const uint32_t*>(P + v);
    if (a.iters && lane == 0) a.iters[b] = it;
    __builtin_amdgcn_wave_barrier();   // the next codeword's rows stay behind these reads
  }
}

// tile geometry of the two staging kernels: block -> (first variable, first codeword) of its 64 x 64 tile
__device__ __forceinline__ void layfix_fused_tile(int B, size_t* r0, size_t* c0) {
  const unsigned tiles_x = (unsigned)((B + 63) / 64);
  *r0 = (size_t)(blockIdx.x / tiles_x) * 64;
  *c0 = (size_t)(blockIdx.x % tiles_x) * 64;
}

}  // namespace

__global__ __launch_bounds__(64 * kLayFixFusedBoundCw) void layfix_fused(const LayFixFusedArgs a) {
  layfix_fused_body<false>(a);
}
__global__ __launch_bounds__(64 * kLayFixFusedBoundCw) void layfix_fused_wide(const LayFixFusedArgs a) {
  layfix_fused_body<true>(a);
}

// buf[b][v] = quantised / copied llr[v][b] for v < n_v, b < B, 0 for n_v <= v < ldn: a 64 x 64 tile (variables x
// codewords) through LDS, 256 threads. It is read a row of the caller's array per wave and written a dword of four
// consecutive variables per thread, 16 threads a codeword's 64 bytes.
__global__ __launch_bounds__(256) void layfix_fused_stage_in(const void* __restrict__ llr, int dtype,
                                                             int8_t* __restrict__ buf, int n_v, int ldn, int B,
                                                             float scale) {
  __shared__ int8_t tile[64][68];   // [variable][codeword]
  const int tx = (int)(threadIdx.x & 63u), ty = (int)(threadIdx.x >> 6);
  size_t r0, c0;
  layfix_fused_tile(B, &r0, &c0);
  for (int j = ty; j < 64; j += 4) {
    const size_t r = r0 + j, c = c0 + tx;
    int x = 0;
    if (r < (size_t)n_v && c < (size_t)B) {
      const size_t src = r * (size_t)B + c;
      if (dtype == kF32) {
        // one rounded product, rint to even, clamped as a float, then converted (layfix_stage_in's statement)
        const float f = __builtin_rintf(static_cast<const float*>(llr)[src] * scale);
        x = (int)fminf(fmaxf(f, -(float)kLayFixApp), (float)kLayFixApp);
      } else {
        x = max((int)static_cast<const int8_t*>(llr)[src], -kLayFixApp);
      }
    }
    tile[j][tx] = (int8_t)x;
  }
  __syncthreads();
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    const int id = pass * 256 + (int)threadIdx.x, q = id & 15, j = id >> 4;
    const size_t c = c0 + j, r = r0 + 4 * q;
    if (c < (size_t)B && r < (size_t)ldn) {   // ldn is a multiple of 4: the dword lies inside the row
      uint32_t w = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) w |= (uint32_t)(uint8_t)tile[4 * q + i][j] << (8 * i);
      *reinterpret_cast<uint32_t*>(buf + c * (size_t)ldn + r) = w;
    }
  }
}

// out[v][b] = buf[b][v] (IBL_I8) or f32(buf[b][v]) / scale (IBL_F32): the same tiles, the other way
__global__ __launch_bounds__(256) void layfix_fused_stage_out(const int8_t* __restrict__ buf, void* __restrict__ out,
                                                              int dtype, int n_v, int ldn, int B, float scale) {
  __shared__ int8_t tile[64][68];   // [variable][codeword]
  const int tx = (int)(threadIdx.x & 63u), ty = (int)(threadIdx.x >> 6);
  size_t r0, c0;
  layfix_fused_tile(B, &r0, &c0);
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    const int id = pass * 256 + (int)threadIdx.x, q = id & 15, j = id >> 4;
    const size_t c = c0 + j, r = r0 + 4 * q;
    uint32_t w = 0;
    if (c < (size_t)B && r < (size_t)ldn) w = *reinterpret_cast<const uint32_t*>(buf + c * (size_t)ldn + r);
#pragma unroll
    for (int i = 0; i < 4; ++i) tile[4 * q + i][j] = (int8_t)(w >> (8 * i));
  }
  __syncthreads();
  for (int j = ty; j < 64; j += 4) {
    const size_t r = r0 + j, c = c0 + tx;
    if (r < (size_t)n_v && c < (size_t)B) {
      const int x = (int)tile[j][tx];
      const size_t dst = r * (size_t)B + c;
      if (dtype == kF32) static_cast<float*>(out)[dst] = (float)x / scale;
      else static_cast<int8_t*>(out)[dst] = (int8_t)x;
    }
  }
}

// blocks per CU of the fused kernel and the largest private segment over it and the two staging kernels
hipError_t layfix_fused_occupancy(bool wide, int cw_per_group, size_t lds, int* blocks_per_cu, size_t* private_bytes) {
  const void* f = wide ? (const void*)layfix_fused_wide : (const void*)layfix_fused;
  hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
  if (e != hipSuccess) return e;
  if ((e = lay_private_bytes({f, (const void*)layfix_fused_stage_in, (const void*)layfix_fused_stage_out},
                             private_bytes)) != hipSuccess)
    return e;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, f, 64 * cw_per_group, lds);
}

hipError_t launch_layfix_fused(const LayFixFusedArgs& a, bool wide, int grid, size_t lds, hipStream_t s) {
  if (!a.buf || !a.task || !a.idx || a.cw_per_group < 1 || a.cw_per_group > kLayFixFusedBoundCw || a.n_tasks < 1 ||
      a.B < 1 || a.ngroups < 1 || grid < 1 || a.n_v < 1 || a.n_c < 1 || a.ldn != fixfused_ldn(a.n_v) ||
      (size_t)a.cw_bytes != fixfused_cw_bytes(a.n_v, a.n_c, wide) ||
      lds < (size_t)a.cw_per_group * (size_t)a.cw_bytes || lds > (size_t)kLdsBytes ||
      (int64_t)a.ngroups * a.cw_per_group < a.B || !fix_params_ok(a.alpha16, a.beta_q, a.q_max))
    return hipErrorInvalidValue;
  LayFixFusedArgs args = a;
  void* p[] = {&args};
  const void* f = wide ? (const void*)layfix_fused_wide : (const void*)layfix_fused;
  return hipLaunchKernel(f, dim3(grid), dim3(64 * a.cw_per_group), p, lds, s);
}

hipError_t launch_layfix_fused_stage_in(const void* llr, int32_t dtype, int8_t* buf, int n_v, int B, float scale,
                                        hipStream_t s) {
  if (!llr || !buf || n_v < 1 || B < 1 || !layfix_dtype_ok(dtype) || !(scale > 0.f)) return hipErrorInvalidValue;
  const int64_t tiles = fixfused_stage_tiles(n_v, B);
  if (tiles > 0x7fffffffll) return hipErrorInvalidValue;
  int ldn = fixfused_ldn(n_v);
  void* p[] = {(void*)&llr, (void*)&dtype, (void*)&buf, (void*)&n_v, (void*)&ldn, (void*)&B, (void*)&scale};
  return hipLaunchKernel((const void*)layfix_fused_stage_in, dim3((unsigned)tiles), dim3(256), p, 0, s);
}

hipError_t launch_layfix_fused_stage_out(const int8_t* buf, void* out, int32_t dtype, int n_v, int B, float scale,
                                         hipStream_t s) {
  if (!buf || !out || n_v < 1 || B < 1 || !layfix_dtype_ok(dtype) || !(scale > 0.f)) return hipErrorInvalidValue;
  const int64_t tiles = fixfused_stage_tiles(n_v, B);
  if (tiles > 0x7fffffffll) return hipErrorInvalidValue;
  int ldn = fixfused_ldn(n_v);
  void* p[] = {(void*)&buf, (void*)&out, (void*)&dtype, (void*)&n_v, (void*)&ldn, (void*)&B, (void*)&scale};
  return hipLaunchKernel((const void*)layfix_fused_stage_out, dim3((unsigned)tiles), dim3(256), p, 0, s);
}

#undef LAY_CASES_32
#undef LAY_CASES_16

}  // namespace ibl

