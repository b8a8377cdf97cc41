// CPU-only checker of the layered decoder's host plan (validate_layers, plan_layered of
// informationbottleneckdecodingldpc_amd/csrc/layered_plan.h), built by tests/test_cpu_layered.py with
// -fsanitize=address,undefined -fno-sanitize-recover=all.
//
//   layered_plan_check <graph.bin>
// graph.bin: int32 n_v, n_c, indptr[n_c + 1], cols[E] (canonical CSR of H), n_layers, layer_ptr[n_layers + 1],
// layer_checks[layer_ptr[n_layers]]. Prints one JSON line {valid, error, n_layers, n_tasks, idx_len,
// cw_per_group, cw_bytes, failures}; exit status 0 = the layers were judged and, when valid, every invariant of
// the plan held.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "layered_plan.h"

using namespace ibl;

static int g_fail = 0;
#define CHECK(cond, what)                                              \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::fprintf(stderr, "invariant failed: %s (%s)\n", what, #cond); \
      ++g_fail;                                                        \
    }                                                                  \
  } while (0)

static bool read_i32(FILE* f, std::vector<int32_t>* v, size_t n) {
  v->resize(n);
  return n == 0 || std::fread(v->data(), 4, n, f) == n;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: layered_plan_check graph.bin\n");
    return 2;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<int32_t> hdr, indptr, cols, nl, lptr, lchk;
  if (!read_i32(f, &hdr, 2)) return 2;
  const int32_t n_v = hdr[0], n_c = hdr[1];
  if (n_v <= 0 || n_c <= 0) return 2;
  if (!read_i32(f, &indptr, (size_t)n_c + 1) || indptr[n_c] < 0) return 2;
  if (!read_i32(f, &cols, (size_t)indptr[n_c])) return 2;
  if (!read_i32(f, &nl, 1) || nl[0] < 0) return 2;
  const int32_t n_layers = nl[0];
  if (!read_i32(f, &lptr, (size_t)n_layers + 1) || lptr[n_layers] < 0) return 2;
  if (!read_i32(f, &lchk, (size_t)lptr[n_layers])) return 2;
  std::fclose(f);
  lchk.push_back(0);   // never read: keeps data() non-null for an empty list

  std::string err;
  const int rc = validate_layers(n_v, n_c, indptr.data(), cols.data(), n_layers, lptr.data(), lchk.data(), &err);
  LayeredPlan pl;
  if (rc == 0) {
    plan_layered(n_v, n_c, indptr.data(), cols.data(), n_layers, lptr.data(), lchk.data(), &pl);
    CHECK(pl.task.size() == (size_t)4 * pl.n_tasks && pl.layer_task.size() == (size_t)n_layers + 1, "table sizes");
    CHECK(pl.cw_bytes == (size_t)4 * n_v + (size_t)12 * n_c, "bytes per codeword");
    CHECK(pl.cw_per_group >= 0 && pl.cw_per_group <= kLayMaxCw &&
              (size_t)pl.cw_per_group * pl.cw_bytes <= (size_t)kLayLds, "codewords per workgroup fit the LDS");
    CHECK(pl.cw_per_group == kLayMaxCw || (size_t)(pl.cw_per_group + 1) * pl.cw_bytes > (size_t)kLayLds,
          "as many codewords as fit");
    std::vector<int32_t> layer_of((size_t)n_c, -1);
    for (int32_t l = 0; l < n_layers; ++l)
      for (int32_t i = lptr[l]; i < lptr[l + 1]; ++i) layer_of[lchk[i]] = l;
    std::vector<int32_t> check_of_slot((size_t)n_c, -1);
    for (int32_t c = 0; c < n_c; ++c) {
      const int32_t s = pl.slot_of[c];
      CHECK(s >= 0 && s < n_c && check_of_slot[s] < 0, "state slots are a permutation of the checks");
      if (s >= 0 && s < n_c) check_of_slot[s] = c;
    }
    int32_t slot = 0;
    size_t first = 0;
    for (int32_t l = 0; l < n_layers; ++l) {
      CHECK(pl.layer_task[l] <= pl.layer_task[l + 1], "layer task ranges ascend");
      int32_t prev_d = kLayMaxD + 1, in_layer = 0;
      for (int32_t t = pl.layer_task[l]; t < pl.layer_task[l + 1]; ++t) {
        const int32_t* r = &pl.task[(size_t)4 * t];
        const int32_t cnt = r[1], d = r[2];
        CHECK((size_t)r[0] == first && r[3] == slot, "tasks are contiguous");
        CHECK(cnt >= 1 && cnt <= 64 && d >= kLayMinD && d <= kLayMaxD && d <= prev_d, "task shape");
        CHECK(first + (size_t)64 * d <= pl.idx.size(), "index rows within the table");
        if (cnt < 1 || cnt > 64 || d < kLayMinD || d > kLayMaxD || first + (size_t)64 * d > pl.idx.size()) break;
        for (int32_t lane = 0; lane < 64; ++lane) {
          const int32_t c = lane < cnt ? check_of_slot[(size_t)slot + lane] : -1;
          if (lane < cnt) {
            CHECK(c >= 0 && layer_of[c] == l && indptr[c + 1] - indptr[c] == d, "a task's checks: its layer, its degree");
            if (c < 0) continue;
          }
          for (int32_t k = 0; k < d; ++k) {
            const int32_t v = pl.idx[first + (size_t)64 * k + lane];
            CHECK(v >= 0 && v < n_v, "variable index in range (padding included)");
            if (lane < cnt) CHECK(v == cols[(size_t)indptr[c] + k], "edge k of a check in ascending column order");
          }
        }
        prev_d = d;
        slot += cnt;
        in_layer += cnt;
        first += (size_t)64 * d;
      }
      CHECK(in_layer == lptr[l + 1] - lptr[l], "a layer's tasks hold the layer's checks");
    }
    CHECK(slot == n_c && first == pl.idx.size(), "every check planned once");
  }
  std::string esc;
  for (char ch : err) esc += (ch == '"' || ch == '\\') ? '?' : ch;
  std::printf("{\"valid\": %d, \"error\": \"%s\", \"n_layers\": %d, \"n_tasks\": %d, \"idx_len\": %zu, "
              "\"cw_per_group\": %d, \"cw_bytes\": %zu, \"failures\": %d}\n",
              rc, esc.c_str(), n_layers, pl.n_tasks, pl.idx.size(), pl.cw_per_group, pl.cw_bytes, g_fail);
  return g_fail ? 1 : 0;
}
