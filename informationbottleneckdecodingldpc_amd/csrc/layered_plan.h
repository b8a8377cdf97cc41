// Host-side planning of the layered (row-serial) min-sum decoder: pure C++17, no HIP (like plan.h).
//
// Built twice: into libibldpc.so (capi.hip includes this header) and, with AddressSanitizer and
// UndefinedBehaviorSanitizer, into the CPU-only checker tests/asan/layered_plan_check.cpp
// (tests/test_cpu_layered.py).
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
#include <vector>

namespace ibl {

constexpr int kLayMinD = 2, kLayMaxD = 16;      // check degrees of the layered kernel's bodies
constexpr int kLayLds = 160 * 1024;             // LDS bytes of a workgroup (gfx950)
constexpr int kLayMaxCw = 8;                    // codewords (= waves) per workgroup at most
constexpr int kLayStateBytes = 12;              // per check and codeword: m1', m2', argmin position | sign bits

// 0 = valid; -1 = malformed (EINVAL: cover, disjointness, shared variable, bad index), -2 = a check degree
// outside [2, 16] (EUNSUPPORTED). *err names the first offending check.
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
    if (d < kLayMinD || d > kLayMaxD)
      return *err = "check " + std::to_string(c) + " has degree " + std::to_string(d) +
                    ": layered decoding supports check degrees 2..16", -2;
  }
  return 0;
}

// LDS bytes one codeword occupies: its APP LLRs P (fp32 per variable) and the compressed check state.
inline size_t layered_cw_bytes(int32_t n_v, int32_t n_c) {
  return (size_t)4 * (size_t)n_v + (size_t)kLayStateBytes * (size_t)n_c;
}
// Codewords a workgroup keeps on chip (one wave each): 0 = the code does not fit.
inline int32_t layered_cw_per_group(int32_t n_v, int32_t n_c) {
  const size_t per = layered_cw_bytes(n_v, n_c);
  return (int32_t)std::min<size_t>((size_t)kLayMaxCw, (size_t)kLayLds / per);
}

struct LayeredPlan {
  std::vector<int32_t> task;       // per task {first idx, count (1..64), degree, first state slot}
  std::vector<int32_t> idx;        // variable of edge k of lane i of a task at [first + 64 k + i]; padding 0
  std::vector<int32_t> slot_of;    // check -> state slot (task order)
  std::vector<int32_t> layer_task; // n_layers + 1: first task of each layer
  int32_t n_tasks = 0, cw_per_group = 0;
  size_t cw_bytes = 0;
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
  pl->cw_bytes = layered_cw_bytes(n_v, n_c);
  pl->cw_per_group = layered_cw_per_group(n_v, n_c);
}

}  // namespace ibl
