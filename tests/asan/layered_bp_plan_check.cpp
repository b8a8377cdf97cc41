// CPU-only checker of the layered BP decoder's host plan (laybp_unsupported_check, laybp_cw_bytes,
// laybp_cw_per_group, plan_layered_bp, laybp_pass_bytes of informationbottleneckdecodingldpc_amd/csrc/layered_plan.h,
// with plan_layered_passes for the per-layer records), built by tests/test_cpu_layered_bp.py with
// -fsanitize=address,undefined -fno-sanitize-recover=all.
//
//   layered_bp_plan_check <graph.bin> <max_batch>
// graph.bin: the format of layered_plan_check.cpp — int32 n_v, n_c, indptr[n_c + 1], cols[E] (canonical CSR of H),
// n_layers, layer_ptr[n_layers + 1], layer_checks[layer_ptr[n_layers]]. Walks every access of the fused kernel's
// tasks (variable index rows against idx, message words against the wave's R[E]) and every row of every item of the
// per-layer launches of a batch of max_batch (against the scratch sizes), the way the kernels index, and prints one
// JSON line {valid, error, unsupported (first check without a degree body, or -1), n_e, n_tasks, cw_bytes,
// cw_per_group, bytes_P, bytes_R, bytes_total, failures}; exit status 0 = the layers were judged and, when the code
// is valid and supported, every invariant held.
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
  if (argc != 3) {
    std::fprintf(stderr, "usage: layered_bp_plan_check graph.bin max_batch\n");
    return 2;
  }
  const long mb = std::strtol(argv[2], nullptr, 10);
  if (mb < 1 || mb > 0x7fffffffl) return 2;
  const int32_t B = (int32_t)mb;
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
  int32_t unsupported = -1;
  LayeredBpPlan pl;
  LayeredBpBytes by;
  const int64_t E = indptr[n_c];
  if (rc == 0) unsupported = laybp_unsupported_check(n_c, indptr.data());
  if (rc == 0 && unsupported >= 0) {
    const int32_t d = indptr[unsupported + 1] - indptr[unsupported];
    CHECK(d < kLayMinD || d > kLayBpMaxD, "the named check has no degree body");
    for (int32_t c = 0; c < unsupported; ++c)
      CHECK(indptr[c + 1] - indptr[c] >= kLayMinD && indptr[c + 1] - indptr[c] <= kLayBpMaxD, "it is the first");
  }
  if (rc == 0 && unsupported < 0) {
    plan_layered_bp(n_v, n_c, indptr.data(), cols.data(), n_layers, lptr.data(), lchk.data(), &pl);
    // ---- fused kernel ----
    CHECK(pl.n_e == E, "the tasks hold every edge");
    CHECK(pl.cw_bytes == (size_t)4 * n_v + (size_t)4 * E && pl.cw_bytes == laybp_cw_bytes(n_v, E), "codeword bytes");
    const size_t fit = (size_t)kLayLds / pl.cw_bytes;
    CHECK(pl.cw_per_group == (int32_t)(fit < (size_t)kLayMaxCw ? fit : (size_t)kLayMaxCw), "fit rule");
    CHECK((size_t)pl.cw_per_group * pl.cw_bytes <= (size_t)kLayLds, "the group fits the LDS");
    CHECK(pl.task.size() == (size_t)4 * pl.n_tasks, "task table size");
    std::vector<int32_t> word_owner((size_t)E, -1), check_seen((size_t)n_c, 0);
    int64_t next_r = 0;
    for (int32_t t = 0; t < pl.n_tasks; ++t) {
      const int32_t first = pl.task[(size_t)4 * t], cnt = pl.task[(size_t)4 * t + 1], d = pl.task[(size_t)4 * t + 2],
                    r0 = pl.task[(size_t)4 * t + 3];
      CHECK(cnt >= 1 && cnt <= 64 && d >= kLayMinD && d <= kLayBpMaxD, "task shape");
      CHECK(r0 == next_r, "the tasks' message ranges tile R in task order");
      CHECK(first >= 0 && (size_t)first + (size_t)64 * d <= pl.idx.size(), "index rows within idx");
      next_r += (int64_t)cnt * d;
      if (cnt < 1 || cnt > 64 || d < kLayMinD || d > kLayBpMaxD || r0 < 0) continue;
      std::vector<int32_t> owner;   // variables of this task: a layer's checks share none
      for (int32_t lane = 0; lane < cnt; ++lane) {
        for (int32_t k = 0; k < d; ++k) {
          const int64_t w = (int64_t)r0 + (int64_t)cnt * k + lane;   // as laybp_cn addresses R
          CHECK(w >= 0 && w < E, "message word within R");
          if (w >= 0 && w < E) {
            CHECK(word_owner[(size_t)w] < 0, "no two edges share a message word");
            word_owner[(size_t)w] = t;
          }
          const size_t at = (size_t)first + (size_t)64 * k + (size_t)lane;
          if (at < pl.idx.size()) {
            const int32_t v = pl.idx[at];
            CHECK(v >= 0 && v < n_v, "variable index within P");
            owner.push_back(v);
          }
        }
      }
      std::vector<int32_t> sorted = owner;
      std::sort(sorted.begin(), sorted.end());
      CHECK(std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end(), "no two lanes of a task share a variable");
    }
    CHECK(next_r == E, "R is exactly E words");
    for (int64_t w = 0; w < E; ++w) CHECK(word_owner[(size_t)w] >= 0, "every message word is used");
    // every check appears in the tasks with its own columns in ascending order
    {
      LayeredPlan ms;
      plan_layered(n_v, n_c, indptr.data(), cols.data(), n_layers, lptr.data(), lchk.data(), &ms);
      CHECK(ms.n_tasks == pl.n_tasks && ms.idx == pl.idx, "tasks and indices are the min-sum plan's");
      for (int32_t c = 0; c < n_c && ms.slot_of.size() == (size_t)n_c; ++c) {
        const int32_t slot = ms.slot_of[c];
        CHECK(slot >= 0 && slot < n_c, "check has a slot");
        if (slot >= 0 && slot < n_c) ++check_seen[(size_t)slot];
      }
      for (int32_t s = 0; s < n_c; ++s) CHECK(check_seen[(size_t)s] == 1, "every check in one task lane");
    }
    // ---- per-layer path ----
    LayeredPassPlan pp;
    plan_layered_passes(n_c, indptr.data(), n_layers, lptr.data(), lchk.data(), &pp);
    by = laybp_pass_bytes(n_v, E, B);
    const int32_t ntiles = pass_tiles(B);
    const size_t ldb = (size_t)pass_ldb(B);
    CHECK(by.P == (size_t)4 * n_v * ldb && by.R == (size_t)4 * (size_t)E * ldb, "row array bytes");
    CHECK(by.mask == (size_t)8 * ntiles && by.counter == 4 && by.bits == (size_t)8 * n_v * ntiles, "mask, counter, bits");
    CHECK(by.total == by.P + by.R + 2 * by.mask + by.counter + by.bits, "total bytes");
    const size_t P_words = by.P / 4, R_words = by.R / 4;
    std::vector<int32_t> row_owner((size_t)E, 0);
    for (int32_t l = 0; l < n_layers; ++l) {
      const int32_t n = lptr[l + 1] - lptr[l];
      const int64_t items = pass_items(n, B), grid = pass_grid(n, B);
      for (int64_t item = 0; item < grid * kLayPassWaves; ++item) {
        if (item >= items) continue;
        const int32_t tile = (int32_t)(item % ntiles), slot = pp.layer_slot[l] + (int32_t)(item / ntiles);
        if (slot < 0 || slot >= n_c) {
          CHECK(false, "item -> slot of the code");
          continue;
        }
        const int32_t e0 = pp.rec[(size_t)2 * slot], d = pp.rec[(size_t)2 * slot + 1];
        CHECK(d >= kLayMinD && d <= kLayBpMaxD, "record degree has a body");
        const size_t tcol = (size_t)tile * kLayTile, last = kLayTile - 1;
        for (int32_t k = 0; k < d; ++k) {
          CHECK((int64_t)e0 + k < E, "edge within the CSR");
          if ((int64_t)e0 + k >= E) continue;
          CHECK((size_t)(e0 + k) * ldb + tcol + last < R_words, "R row within the scratch");   // as laybp_cn_rows
          CHECK((size_t)cols[(size_t)e0 + k] * ldb + tcol + last < P_words, "P row within the scratch");
          if (tile == 0) ++row_owner[(size_t)e0 + k];
        }
      }
    }
    for (int64_t e = 0; e < E; ++e) CHECK(row_owner[(size_t)e] == 1, "every R row written by one item per iteration");
  }
  std::string esc;
  for (char ch : err) esc += (ch == '"' || ch == '\\') ? '?' : ch;
  std::printf("{\"valid\": %d, \"error\": \"%s\", \"unsupported\": %d, \"n_e\": %lld, \"n_tasks\": %d, \"cw_bytes\": %zu, "
              "\"cw_per_group\": %d, \"bytes_P\": %zu, \"bytes_R\": %zu, \"bytes_total\": %zu, \"failures\": %d}\n",
              rc, esc.c_str(), unsupported, (long long)E, pl.n_tasks, pl.cw_bytes, pl.cw_per_group, by.P, by.R, by.total,
              g_fail);
  return g_fail ? 1 : 0;
}
