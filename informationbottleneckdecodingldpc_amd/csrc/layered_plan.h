// Host-side planning of the layered (row-serial) min-sum decoder: pure C++17, no HIP (like plan.h).
//
// Built into libibldpc.so (capi_layered.hip includes this header) and, with AddressSanitizer and
// UndefinedBehaviorSanitizer, into the CPU-only checkers tests/asan/layered_plan_check.cpp
// (tests/test_cpu_layered.py), tests/asan/layered_pass_plan_check.cpp (tests/test_cpu_layered_passes.py),
// tests/asan/layered_fixed_plan_check.cpp (tests/test_cpu_layered_fixed.py),
// tests/asan/layered_compact_plan_check.cpp (tests/test_cpu_layered_compact.py),
// tests/asan/layered_wide_plan_check.cpp (tests/test_cpu_layered_wide.py),
// tests/asan/layered_fixed_fused_plan_check.cpp (tests/test_cpu_layered_fixed_fused.py),
// tests/asan/layered_bp_plan_check.cpp (tests/test_cpu_layered_bp.py) and
// tests/asan/layered_half_plan_check.cpp (tests/test_cpu_layered_half.py).
//
// A layer is a set of checks no two of which share a variable; the layers are disjoint, cover every check and
// are decoded in order (include/ibldpc.h "Layered min-sum"). The device plan cuts every layer into tasks of up
// to 64 checks of one degree (lane = check), numbers the checks in task order (their state slots) and lists
// the variable of edge k of lane i of a task at idx[first + 64 k + i] — every task's rows padded to 64 lanes,
// so a lane's index loads need no bound.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

namespace ibl {

constexpr int kLayMinD = 2, kLayMaxD = 16;      // check degrees of the narrow kernels' bodies
constexpr int kLayWideMaxD = 32;                // check degrees up to this run the wide kernels (below)
constexpr int kLayLds = 160 * 1024;             // LDS bytes of a workgroup (gfx950)
constexpr int kLayMaxCw = 8;                    // codewords (= waves) per workgroup at most
constexpr int kLayStateBytes = 12;              // per check and codeword: m1', m2', argmin position | sign bits
constexpr int kLayWideStateBytes = 16;          // wide: m1', m2', 32 sign bits, the argmin position in its own word

// A code (and every handle made for it) is WIDE when some check has a degree above kLayMaxD. A wide handle keeps
// the sign bits of R in a whole 32-bit word and the argmin position in a word of its own, for every check of the
// code, and runs the *_wide kernels; a narrow handle is what it always was. Precondition: a valid indptr.
inline bool layered_is_wide(int32_t n_c, const int32_t* indptr) {
  for (int32_t c = 0; c < n_c; ++c)
    if (indptr[c + 1] - indptr[c] > kLayMaxD) return true;
  return false;
}

// 0 = valid; -1 = malformed (EINVAL: cover, disjointness, shared variable, bad index), -2 = a check degree
// outside [2, 32] (EUNSUPPORTED). *err names the first offending check.
inline int validate_layers(int32_t n_v, int32_t n_c, const int32_t* indptr, const int32_t* cols, int32_t n_layers,
                           const int32_t* layer_ptr, const int32_t* layer_checks, std::string* err) {
  if (n_v <= 0 || n_c <= 0 || !indptr || !cols) return *err = "empty graph", -1;
  if (n_layers < 1 || !layer_ptr || !layer_checks) return *err = "no layers", -1;
  if (layer_ptr[0] != 0) return *err = "layer_ptr[0] must be 0", -1;
  for (int32_t l = 0; l < n_layers; ++l)
    if (layer_ptr[l + 1] < layer_ptr[l]) return *err = "layer_ptr not monotone", -1;
  if (indptr[0] != 0) return *err = "csr_indptr[0] must be 0", -1;
  for (int32_t c = 0; c < n_c; ++c) {
    if (indptr[c + 1] < indptr[c]) return *err = "csr_indptr not monotone", -1;
    for (int32_t e = indptr[c]; e < indptr[c + 1]; ++e)
      if (cols[e] < 0 || cols[e] >= n_v) return *err = "column index out of range in check " + std::to_string(c), -1;
  }
  std::vector<int32_t> layer_of((size_t)n_c, -1);
  std::vector<int32_t> owner((size_t)n_v, -1);   // check of the current layer that holds the variable
  for (int32_t l = 0; l < n_layers; ++l) {
    for (int32_t i = layer_ptr[l]; i < layer_ptr[l + 1]; ++i) {
      const int32_t c = layer_checks[i];
      if (c < 0 || c >= n_c) return *err = "layer " + std::to_string(l) + " names check " + std::to_string(c) +
                                           " out of range", -1;
      if (layer_of[c] >= 0)
        return *err = "check " + std::to_string(c) + " is listed twice (layers " + std::to_string(layer_of[c]) +
                      " and " + std::to_string(l) + ")", -1;
      layer_of[c] = l;
    }
    for (int32_t i = layer_ptr[l]; i < layer_ptr[l + 1]; ++i) {
      const int32_t c = layer_checks[i];
      for (int32_t e = indptr[c]; e < indptr[c + 1]; ++e) {
        const int32_t v = cols[e];
        if (owner[v] >= 0 && owner[v] != c)
          return *err = "checks " + std::to_string(owner[v]) + " and " + std::to_string(c) + " of layer " +
                        std::to_string(l) + " share variable " + std::to_string(v), -1;
        owner[v] = c;
      }
    }
    for (int32_t i = layer_ptr[l]; i < layer_ptr[l + 1]; ++i) {
      const int32_t c = layer_checks[i];
      for (int32_t e = indptr[c]; e < indptr[c + 1]; ++e) owner[cols[e]] = -1;
    }
  }
  for (int32_t c = 0; c < n_c; ++c)
    if (layer_of[c] < 0) return *err = "check " + std::to_string(c) + " is in no layer", -1;
  for (int32_t c = 0; c < n_c; ++c) {
    const int32_t d = indptr[c + 1] - indptr[c];
    if (d < kLayMinD || d > kLayWideMaxD)
      return *err = "check " + std::to_string(c) + " has degree " + std::to_string(d) +
                    ": layered decoding supports check degrees 2..32", -2;
  }
  return 0;
}

// LDS bytes one codeword occupies: its APP LLRs P (fp32 per variable) and the compressed check state
// (4 N + 12 n_c; wide: 4 N + 16 n_c).
inline size_t layered_cw_bytes(int32_t n_v, int32_t n_c, bool wide = false) {
  return (size_t)4 * (size_t)n_v + (size_t)(wide ? kLayWideStateBytes : kLayStateBytes) * (size_t)n_c;
}
// Codewords a workgroup keeps on chip (one wave each): 0 = the code does not fit.
inline int32_t layered_cw_per_group(int32_t n_v, int32_t n_c, bool wide = false) {
  const size_t per = layered_cw_bytes(n_v, n_c, wide);
  return (int32_t)std::min<size_t>((size_t)kLayMaxCw, (size_t)kLayLds / per);
}

struct LayeredPlan {
  std::vector<int32_t> task;       // per task {first idx, count (1..64), degree, first state slot}
  std::vector<int32_t> idx;        // variable of edge k of lane i of a task at [first + 64 k + i]; padding 0
  std::vector<int32_t> slot_of;    // check -> state slot (task order)
  std::vector<int32_t> layer_task; // n_layers + 1: first task of each layer
  int32_t n_tasks = 0, cw_per_group = 0;
  size_t cw_bytes = 0;
  bool wide = false;               // some check has a degree above kLayMaxD: the wide state and fit rule
};

// Precondition: validate_layers(...) == 0.
inline void plan_layered(int32_t n_v, int32_t n_c, const int32_t* indptr, const int32_t* cols, int32_t n_layers,
                         const int32_t* layer_ptr, const int32_t* layer_checks, LayeredPlan* pl) {
  pl->task.clear(); pl->idx.clear(); pl->layer_task.clear();
  pl->slot_of.assign((size_t)n_c, -1);
  int32_t slot = 0;
  for (int32_t l = 0; l < n_layers; ++l) {
    pl->layer_task.push_back((int32_t)(pl->task.size() / 4));
    std::vector<int32_t> ord(layer_checks + layer_ptr[l], layer_checks + layer_ptr[l + 1]);
    auto deg = [&](int32_t c) { return indptr[c + 1] - indptr[c]; };
    std::stable_sort(ord.begin(), ord.end(), [&](int32_t x, int32_t y) { return deg(x) > deg(y); });
    for (size_t i = 0; i < ord.size();) {
      const int32_t d = deg(ord[i]);
      int32_t cnt = 0;
      while (i + cnt < ord.size() && cnt < 64 && deg(ord[i + cnt]) == d) ++cnt;
      const int32_t first = (int32_t)pl->idx.size();
      pl->task.insert(pl->task.end(), {first, cnt, d, slot});
      pl->idx.resize((size_t)first + (size_t)64 * d, 0);
      for (int32_t lane = 0; lane < cnt; ++lane) {
        const int32_t c = ord[i + lane];
        pl->slot_of[c] = slot + lane;
        for (int32_t k = 0; k < d; ++k) pl->idx[(size_t)first + (size_t)64 * k + lane] = cols[indptr[c] + k];
      }
      slot += cnt;
      i += cnt;
    }
  }
  pl->layer_task.push_back((int32_t)(pl->task.size() / 4));
  pl->n_tasks = (int32_t)(pl->task.size() / 4);
  pl->wide = layered_is_wide(n_c, indptr);
  pl->cw_bytes = layered_cw_bytes(n_v, n_c, pl->wide);
  pl->cw_per_group = layered_cw_per_group(n_v, n_c, pl->wide);
}

// ---- per-layer path over HBM (codes of any length; checked by tests/asan/layered_pass_plan_check.cpp) --------
// lane = codeword: P[n_v][ldb] and, per check, the three state rows M1 / M2 / PS [n_c][ldb] (wide: a fourth, PO,
// the argmin position, PS being all sign bits), the checks in layer order (slot = position in layer_checks). One launch per layer; a wave item is (check of the layer, tile of
// kLayTile codewords), tile fastest, kLayPassWaves items per workgroup. The syndrome's item is (run of kLaySynRun
// consecutive slots, tile) in its gather form; its packed form first packs the hard decisions into one 64-bit word
// per (variable, tile), item (run of kLayTile variables, tile), then XORs them per check, item (run of kLayTile
// slots, tile). One 64-bit mask of finished and one of unsatisfied codewords per tile.
constexpr int kLayTile = 64;        // codewords per wave item (one dword per lane and row)
constexpr int kLayPassWaves = 4;    // wave items per workgroup (256 threads)
constexpr int kLaySynRun = 16;      // checks per syndrome item

inline int32_t pass_tiles(int32_t B, int32_t tile = kLayTile) { return (int32_t)(((int64_t)B + tile - 1) / tile); }
// padded row stride (codewords) of a batch of B
inline int64_t pass_ldb(int32_t B, int32_t tile = kLayTile) { return (int64_t)pass_tiles(B, tile) * tile; }
// wave items and workgroups of a launch over n_checks checks (a layer, or the syndrome's runs) for a batch of B
inline int64_t pass_items(int32_t n_checks, int32_t B, int32_t tile = kLayTile) {
  return (int64_t)n_checks * (int64_t)pass_tiles(B, tile);
}
inline int64_t pass_grid(int32_t n_checks, int32_t B, int32_t tile = kLayTile) {
  return (pass_items(n_checks, B, tile) + kLayPassWaves - 1) / kLayPassWaves;
}
inline int32_t pass_syn_runs(int32_t n_c) { return (int32_t)(((int64_t)n_c + kLaySynRun - 1) / kLaySynRun); }
// packed syndrome: runs of kLayTile variables (packing, a lane keeps a variable's word) or checks (lane = check)
inline int32_t pass_pack_runs(int32_t n) { return (int32_t)(((int64_t)n + kLayTile - 1) / kLayTile); }

// byte sizes of the device scratch a per-layer handle of max_batch owns
struct LayeredPassBytes {
  size_t P = 0;       // [n_v][ldb] fp32
  size_t state = 0;   // each of M1, M2, PS (wide: and PO): [n_c][ldb] 4-byte words
  size_t mask = 0;    // each of finished, unsatisfied: one 64-bit word per tile
  size_t counter = 0; // codewords still running
  size_t bits = 0;    // packed hard decisions: one 64-bit word per variable and tile
  size_t total = 0;   // P + 3 (wide: 4) state + 2 mask + counter + bits
};
constexpr int pass_state_arrays(bool wide) { return wide ? 4 : 3; }
inline LayeredPassBytes pass_bytes(int32_t n_v, int32_t n_c, int32_t max_batch, bool wide = false) {
  LayeredPassBytes b;
  const size_t ldb = (size_t)pass_ldb(max_batch);
  b.P = (size_t)4 * (size_t)n_v * ldb;
  b.state = (size_t)4 * (size_t)n_c * ldb;
  b.mask = (size_t)8 * (size_t)pass_tiles(max_batch);
  b.counter = 4;
  b.bits = (size_t)8 * (size_t)n_v * (size_t)pass_tiles(max_batch);
  b.total = b.P + (size_t)pass_state_arrays(wide) * b.state + 2 * b.mask + b.counter + b.bits;
  return b;
}

struct LayeredPassPlan {
  std::vector<int32_t> rec;         // per slot {CSR offset of the check's first edge, degree}
  std::vector<int32_t> check_of;    // slot -> check
  std::vector<int32_t> layer_slot;  // n_layers + 1: first slot of each layer
  int32_t max_layer = 0;            // checks of the largest layer
};

// Precondition: validate_layers(...) == 0.
inline void plan_layered_passes(int32_t n_c, const int32_t* indptr, int32_t n_layers, const int32_t* layer_ptr,
                                const int32_t* layer_checks, LayeredPassPlan* pl) {
  pl->rec.clear(); pl->check_of.clear();
  pl->layer_slot.assign(layer_ptr, layer_ptr + n_layers + 1);
  pl->rec.reserve((size_t)2 * (size_t)n_c);
  pl->check_of.reserve((size_t)n_c);
  pl->max_layer = 0;
  for (int32_t l = 0; l < n_layers; ++l) {
    pl->max_layer = std::max(pl->max_layer, layer_ptr[l + 1] - layer_ptr[l]);
    for (int32_t i = layer_ptr[l]; i < layer_ptr[l + 1]; ++i) {
      const int32_t c = layer_checks[i];
      pl->check_of.push_back(c);
      pl->rec.push_back(indptr[c]);
      pl->rec.push_back(indptr[c + 1] - indptr[c]);
    }
  }
}

// ---- layered BP (include/ibldpc.h "Layered BP"; layered_bp_kernels.hip; checked by
// tests/asan/layered_bp_plan_check.cpp) ---------------------------------------------------------------------------
// BP keeps the check messages R whole: one fp32 word per edge and codeword next to P. Check degrees 2..kLayBpMaxD.
constexpr int kLayBpMaxD = 16;

// the first check whose degree the BP kernels have no body for, or -1. Precondition: a valid indptr.
inline int32_t laybp_unsupported_check(int32_t n_c, const int32_t* indptr) {
  for (int32_t c = 0; c < n_c; ++c) {
    const int32_t d = indptr[c + 1] - indptr[c];
    if (d < kLayMinD || d > kLayBpMaxD) return c;
  }
  return -1;
}
// LDS bytes one codeword occupies in the fused kernel: P (4 N) and R (4 E)
inline size_t laybp_cw_bytes(int32_t n_v, int64_t n_e) { return (size_t)4 * (size_t)n_v + (size_t)4 * (size_t)n_e; }
// Codewords a workgroup keeps on chip (one wave each): 0 = the code does not fit.
inline int32_t laybp_cw_per_group(int32_t n_v, int64_t n_e) {
  return (int32_t)std::min<size_t>((size_t)kLayMaxCw, (size_t)kLayLds / laybp_cw_bytes(n_v, n_e));
}

// The fused kernel's plan: the tasks and variable indices of plan_layered (idx rows padded to 64 lanes), a task's
// fourth word being the first R word of the task instead of a state slot: edge k of lane i of a task has its
// message at R[rfirst + count k + i] — rows of `count` words, not 64, so R is exactly E words, the words a task
// touches for one k are consecutive, and the tasks' ranges tile [0, E) in task order.
struct LayeredBpPlan {
  std::vector<int32_t> task;   // per task {first idx, count (1..64), degree, first R word}
  std::vector<int32_t> idx;    // variable of edge k of lane i of a task at [first + 64 k + i]; padding 0
  int32_t n_tasks = 0, cw_per_group = 0;
  int64_t n_e = 0;
  size_t cw_bytes = 0;
};
// Precondition: validate_layers(...) == 0 and laybp_unsupported_check(...) < 0.
inline void plan_layered_bp(int32_t n_v, int32_t n_c, const int32_t* indptr, const int32_t* cols, int32_t n_layers,
                            const int32_t* layer_ptr, const int32_t* layer_checks, LayeredBpPlan* pl) {
  LayeredPlan ms;
  plan_layered(n_v, n_c, indptr, cols, n_layers, layer_ptr, layer_checks, &ms);
  pl->task = std::move(ms.task);
  pl->idx = std::move(ms.idx);
  pl->n_tasks = ms.n_tasks;
  int64_t r = 0;
  for (int32_t t = 0; t < pl->n_tasks; ++t) {
    pl->task[(size_t)4 * t + 3] = (int32_t)r;
    r += (int64_t)pl->task[(size_t)4 * t + 1] * pl->task[(size_t)4 * t + 2];
  }
  pl->n_e = r;   // == indptr[n_c]: every check is in one task
  pl->cw_bytes = laybp_cw_bytes(n_v, r);
  pl->cw_per_group = laybp_cw_per_group(n_v, r);
}

// Per-layer path: the records and layer slots are plan_layered_passes' (rec = {CSR offset, degree} per slot); the
// message of edge k of the check in a slot is row rec[2 slot] + k of R [E][ldb], the CSR edge itself. Byte sizes of
// the device scratch a handle of max_batch owns: about 4 N + 4 E bytes per codeword.
struct LayeredBpBytes {
  size_t P = 0;       // [n_v][ldb] fp32
  size_t R = 0;       // [E][ldb] fp32
  size_t mask = 0;    // each of finished, unsatisfied: one 64-bit word per tile
  size_t counter = 0;
  size_t bits = 0;    // packed hard decisions: one 64-bit word per variable and tile
  size_t total = 0;   // P + R + 2 mask + counter + bits
};
inline LayeredBpBytes laybp_pass_bytes(int32_t n_v, int64_t n_e, int32_t max_batch) {
  LayeredBpBytes b;
  const size_t ldb = (size_t)pass_ldb(max_batch);
  b.P = (size_t)4 * (size_t)n_v * ldb;
  b.R = (size_t)4 * (size_t)n_e * ldb;
  b.mask = (size_t)8 * (size_t)pass_tiles(max_batch);
  b.counter = 4;
  b.bits = (size_t)8 * (size_t)n_v * (size_t)pass_tiles(max_batch);
  b.total = b.P + b.R + 2 * b.mask + b.counter + b.bits;
  return b;
}

// ---- layered BP, half state (include/ibldpc.h "Layered BP, half-precision state"; layered_half_kernels.hip; checked
// by tests/asan/layered_half_plan_check.cpp) --------------------------------------------------------------------------
// P and R are IEEE binary16. Fused: the wave's LDS slice is P16[N] | R16[E], rounded up to whole dwords so that the
// next wave's slice is aligned; the tasks and variable indices are plan_layered_bp's. Per layer: a lane owns 2
// consecutive codewords (one dword of a row), P16 [n_v][ldb] and R16 [E][ldb] with ldb a multiple of kLayHalfTile; a
// wave item is (check of the layer, tile of kLayHalfTile codewords). The plan (LayeredPassPlan), the masks of
// finished and unsatisfied codewords and the packed hard decisions stay per kLayTile codewords, the mask arrays padded
// to whole tiles of kLayHalfTile (the padding words all ones: finished).
constexpr int kLayHalfCw = 2;                               // codewords per lane
constexpr int kLayHalfTile = kLayHalfCw * kLayTile;         // codewords per wave item

inline size_t layhp_cw_bytes(int32_t n_v, int64_t n_e) {
  return ((size_t)2 * (size_t)n_v + (size_t)2 * (size_t)n_e + 3) / 4 * 4;
}
// Codewords a workgroup keeps on chip (one wave each): 0 = the code does not fit.
inline int32_t layhp_cw_per_group(int32_t n_v, int64_t n_e) {
  return (int32_t)std::min<size_t>((size_t)kLayMaxCw, (size_t)kLayLds / layhp_cw_bytes(n_v, n_e));
}
// The fused kernel's plan: plan_layered_bp's tasks, indices and R layout, with the half state's bytes and fit.
// Precondition: validate_layers(...) == 0 and laybp_unsupported_check(...) < 0.
inline void plan_layered_bp_half(int32_t n_v, int32_t n_c, const int32_t* indptr, const int32_t* cols, int32_t n_layers,
                                 const int32_t* layer_ptr, const int32_t* layer_checks, LayeredBpPlan* pl) {
  plan_layered_bp(n_v, n_c, indptr, cols, n_layers, layer_ptr, layer_checks, pl);
  pl->cw_bytes = layhp_cw_bytes(n_v, pl->n_e);
  pl->cw_per_group = layhp_cw_per_group(n_v, pl->n_e);
}

inline int32_t half_tiles(int32_t B) { return pass_tiles(B, kLayHalfTile); }
inline int64_t half_ldb(int32_t B) { return pass_ldb(B, kLayHalfTile); }
// words of each mask array: the kLayTile tiles of whole tiles of kLayHalfTile
inline int64_t half_mask_words(int32_t B) { return (int64_t)half_tiles(B) * kLayHalfCw; }
inline int64_t half_items(int32_t n_checks, int32_t B) { return pass_items(n_checks, B, kLayHalfTile); }
inline int64_t half_grid(int32_t n_checks, int32_t B) { return pass_grid(n_checks, B, kLayHalfTile); }
// the word `word` of the finished mask as the stage-in writes it for a batch of B: all ones past the batch
constexpr uint64_t half_done_word(int32_t word, int32_t B) {
  const int64_t left = (int64_t)B - (int64_t)word * kLayTile;
  return left >= kLayTile ? 0ull : left <= 0 ? ~0ull : ~0ull << left;
}
// byte sizes of the device scratch a per-layer handle of max_batch owns: about 2 N + 2 E bytes per codeword
inline LayeredBpBytes layhp_pass_bytes(int32_t n_v, int64_t n_e, int32_t max_batch) {
  LayeredBpBytes b;
  const size_t ldb = (size_t)half_ldb(max_batch);
  b.P = (size_t)2 * (size_t)n_v * ldb;
  b.R = (size_t)2 * (size_t)n_e * ldb;
  b.mask = (size_t)8 * (size_t)half_mask_words(max_batch);
  b.counter = 4;
  b.bits = (size_t)8 * (size_t)n_v * (size_t)pass_tiles(max_batch);
  b.total = b.P + b.R + 2 * b.mask + b.counter + b.bits;
  return b;
}

// ---- compaction of the running codewords, fp32 per-layer path (include/ibldpc.h "Layered min-sum", compaction;
// checked by tests/asan/layered_compact_plan_check.cpp) --------------------------------------------------------------
// Between iterations the columns of the running codewords move to the lowest columns of P, M1, M2 and PS, so that
// whole tiles past them are finished and skipped. The two functions below are the policy and the map, shared by the
// device plan kernel (lay_compact_plan) and the host-side checker; constexpr, so the kernels call them as they stand.
constexpr int kLayCompactCtl = 4;   // control words: the three below and one of padding
enum { kLayCtlExtent = 0, kLayCtlDo = 1, kLayCtlCount = 2 };   // columns in use; compaction in progress; count

// Whether the R running codewords of an extent of E columns are compacted: never when none runs, else when the
// move frees at least max(1, ceil(min_free_pct tE / 100)) of the extent's tE tiles.
constexpr bool compact_wanted(int32_t R, int32_t E, int32_t min_free_pct) {
  if (R <= 0 || E <= 0 || R > E) return false;
  const int64_t tE = ((int64_t)E + kLayTile - 1) / kLayTile, tR = ((int64_t)R + kLayTile - 1) / kLayTile;
  const int64_t pct = ((int64_t)min_free_pct * tE + 99) / 100;
  return tE - tR >= (pct > 1 ? pct : 1);
}
// The rank map of one column: `done` is the finished mask of the column's tile, `lane` the column's bit, `below`
// the running columns of the tiles before it. A running column goes to the number of running columns below it
// (stable: never above its own place), a finished one is flushed (-1).
constexpr int32_t compact_rank(uint64_t done, int lane, int32_t below) {
  if ((done >> lane) & 1ull) return -1;
  return below + (int32_t)__builtin_popcountll(~done & ((1ull << lane) - 1ull));
}
// running columns of a tile
constexpr int32_t compact_tile_count(uint64_t done) { return (int32_t)__builtin_popcountll(~done); }
// the finished mask of tile `tile` once R columns are in use: bit set for every column >= R
constexpr uint64_t compact_done_word(int32_t tile, int32_t R) {
  const int64_t left = (int64_t)R - (int64_t)tile * kLayTile;
  return left >= kLayTile ? 0ull : left <= 0 ? ~0ull : ~0ull << left;
}

// byte sizes of the device state compaction adds to a per-layer handle of max_batch (allocated when first enabled)
struct LayeredCompactBytes {
  size_t orig = 0;    // [ldb] int32: the caller's column of the codeword now in column c
  size_t dest = 0;    // [ldb] int32: the map of the compaction in progress
  size_t ctl = 0;     // kLayCompactCtl int32 words
  size_t total = 0;
};
inline LayeredCompactBytes pass_compact_bytes(int32_t max_batch) {
  LayeredCompactBytes b;
  b.orig = b.dest = (size_t)4 * (size_t)pass_ldb(max_batch);
  b.ctl = (size_t)4 * kLayCompactCtl;
  b.total = b.orig + b.dest + b.ctl;
  return b;
}
// wave items of the row move: the n_v rows of P and the n_c rows of each of M1, M2, PS (wide: and PO)
inline int64_t pass_compact_rows(int32_t n_v, int32_t n_c, bool wide = false) {
  return (int64_t)n_v + pass_state_arrays(wide) * (int64_t)n_c;
}

// ---- fixed point, per-layer path (include/ibldpc.h "Layered min-sum, fixed point"; checked by
// tests/asan/layered_fixed_plan_check.cpp) ------------------------------------------------------------------------
// A lane owns 4 consecutive codewords: P[n_v][ldb] int8 (one dword per row and lane) and one 32-bit state word per
// check and codeword S[n_c][ldb] (a lane's four words one 16-byte load), ldb a multiple of kLayFixTile. A wave
// item is (check of the layer, tile of kLayFixTile codewords); the plan (LayeredPassPlan), the masks of finished
// and unsatisfied codewords and the packed hard decisions stay per kLayTile codewords, the mask arrays padded to
// whole tiles of kLayFixTile (the padding words all ones: finished).
constexpr int kLayFixCw = 4;                              // codewords per lane
constexpr int kLayFixTile = kLayFixCw * kLayTile;         // codewords per wave item
constexpr int kLayFixApp = 127, kLayFixQMax = 63, kLayFixAlphaOne = 16;

inline int32_t fix_tiles(int32_t B) { return pass_tiles(B, kLayFixTile); }
inline int64_t fix_ldb(int32_t B) { return pass_ldb(B, kLayFixTile); }
// words of each mask array: the kLayTile tiles of whole tiles of kLayFixTile
inline int64_t fix_mask_words(int32_t B) { return (int64_t)fix_tiles(B) * kLayFixCw; }
inline int64_t fix_items(int32_t n_checks, int32_t B) { return pass_items(n_checks, B, kLayFixTile); }
inline int64_t fix_grid(int32_t n_checks, int32_t B) { return pass_grid(n_checks, B, kLayFixTile); }

struct LayeredFixBytes {
  size_t P = 0;       // [n_v][ldb] int8
  size_t state = 0;   // [n_c][ldb] 32-bit words; wide: two such arrays, one after the other
  size_t mask = 0;    // each of finished, unsatisfied
  size_t counter = 0;
  size_t bits = 0;    // one 64-bit word per variable and tile of kLayTile
  size_t total = 0;   // P + state + 2 mask + counter + bits
};
inline LayeredFixBytes fix_bytes(int32_t n_v, int32_t n_c, int32_t max_batch, bool wide = false) {
  LayeredFixBytes b;
  const size_t ldb = (size_t)fix_ldb(max_batch);
  b.P = (size_t)n_v * ldb;
  b.state = (size_t)(wide ? 8 : 4) * (size_t)n_c * ldb;
  b.mask = (size_t)8 * (size_t)fix_mask_words(max_batch);
  b.counter = 4;
  b.bits = (size_t)8 * (size_t)n_v * (size_t)pass_tiles(max_batch);
  b.total = b.P + b.state + 2 * b.mask + b.counter + b.bits;
  return b;
}
// ibl_layered_create_fixed's ranges: alpha16 in [0, 16], beta_q in [0, 63], q_max in [1, 63]
constexpr bool fix_params_ok(int32_t alpha16, int32_t beta_q, int32_t q_max) {
  return alpha16 >= 0 && alpha16 <= kLayFixAlphaOne && beta_q >= 0 && beta_q <= kLayFixQMax && q_max >= 1 &&
         q_max <= kLayFixQMax;
}
// the state word of a check: corrected magnitudes (6 bits each), first argmin position, sign bits of R (edge k at bit k)
constexpr uint32_t fix_state_word(uint32_t m1, uint32_t m2, uint32_t pos, uint32_t signs) {
  return (m2 << 26) | (m1 << 20) | (pos << 16) | signs;
}
// The two state words of a check of a wide handle (degrees up to kLayWideMaxD), in the arrays S0 and S1 [n_c][ldb]:
//   word 0 = corrected m2 << 11 | corrected m1 << 5 | first argmin position (5 bits);
//   word 1 = the sign bits of R, edge k at bit k (all 32 bits at degree 32).
struct FixWideWords {
  uint32_t w0, w1;
};
constexpr FixWideWords fix_state_words_wide(uint32_t m1, uint32_t m2, uint32_t pos, uint32_t signs) {
  return FixWideWords{(m2 << 11) | (m1 << 5) | pos, signs};
}
constexpr uint32_t fix_wide_m1(uint32_t w0) { return (w0 >> 5) & 63u; }
constexpr uint32_t fix_wide_m2(uint32_t w0) { return (w0 >> 11) & 63u; }
constexpr uint32_t fix_wide_pos(uint32_t w0) { return w0 & 31u; }
// the low D bits set, D in [1, 32] (1u << 32 is undefined)
constexpr uint32_t fix_wide_mask(int D) { return 0xFFFFFFFFu >> (32 - D); }

// ---- fixed point, fused on chip (include/ibldpc.h "Layered min-sum, fixed point", the fused kernel; checked by
// tests/asan/layered_fixed_fused_plan_check.cpp) -----------------------------------------------------------------
// One wave owns one codeword, as in the fp32 fused kernel, and the device plan is that kernel's (plan_layered:
// task, idx). The wave's slice of LDS is P[ldn] int8, ldn = N rounded up to 4 so that the state words behind it are
// aligned, then S[n_c] (fix_state_word) or, wide, S[n_c] and S1[n_c] (fix_state_words_wide). Codewords travel
// through a [max_batch][ldn] int8 scratch buffer, rows of whole dwords; the staging kernels move 64 x 64 tiles
// (64 variables x 64 codewords) between it and the caller's [N][B] arrays.
// Codewords (= waves) of a workgroup: the cap a handle is created with, and the most the kernels are built for
// (their launch bounds: 1,024 threads, which caps the registers at 128 a lane). Small workgroups measured fastest
// (DESIGN.md "Layered min-sum: fixed point, fused"): 8, 4, 2 and 1 tie on a large batch, all ahead of 16, and 4 or
// fewer spread a small batch over more CUs.
constexpr int kLayFixFusedMaxCw = 4;
constexpr int kLayFixFusedBoundCw = 16;

inline int32_t fixfused_ldn(int32_t n_v) { return (int32_t)(((int64_t)n_v + 3) / 4 * 4); }
inline size_t fixfused_cw_bytes(int32_t n_v, int32_t n_c, bool wide = false) {
  return (size_t)fixfused_ldn(n_v) + (size_t)(wide ? 8 : 4) * (size_t)n_c;
}
// Codewords a workgroup keeps on chip: 0 = the code does not fit. cap: in [1, kLayFixFusedBoundCw]
inline int32_t fixfused_cw_per_group(int32_t n_v, int32_t n_c, bool wide = false, int32_t cap = kLayFixFusedMaxCw) {
  return (int32_t)std::min<size_t>((size_t)cap, (size_t)kLayLds / fixfused_cw_bytes(n_v, n_c, wide));
}
// bytes of the scratch buffer of a handle of max_batch
inline size_t fixfused_buf_bytes(int32_t n_v, int32_t max_batch) {
  return (size_t)max_batch * (size_t)fixfused_ldn(n_v);
}
// workgroups of a staging launch for a batch of B: tiles over the ldn scratch columns (variables) x the codewords
inline int64_t fixfused_stage_tiles(int32_t n_v, int32_t B) {
  return (((int64_t)fixfused_ldn(n_v) + 63) / 64) * (((int64_t)B + 63) / 64);
}

}  // namespace ibl
