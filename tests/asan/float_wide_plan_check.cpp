// CPU-only checker of the float decoders' host planning (informationbottleneckdecodingldpc_amd/csrc/plan.h) on codes
// with checks of degree 17..32 (wide handles), built by tests/test_cpu_float_wide.py with
// -fsanitize=address,undefined -fno-sanitize-recover=all.
//
//   float_wide_plan_check <graph.bin>
// graph.bin: int32 n_v, n_c, indptr[n_c + 1], cols[E] (canonical CSR of H, as plan_check.cpp). Runs what float_create
// derives on the host — the check work order and its small-batch tasks, the degree-2 fold plan, the fused kernel's
// task tables with the padded variable slot indices — and walks them the way the wide check items index (edge j of
// lane i of a task at first + j * count + i for every j below the degree, not only below 16; a small-batch lane's
// rows st .. st + d - 1; the fold's positions inside a check of any degree). Prints one JSON line; exit status 0 =
// every invariant held.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "plan.h"

using namespace ibl;

static int g_fail = 0;
#define CHECK(cond, what)                                              \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::fprintf(stderr, "invariant failed: %s (%s)\n", what, #cond); \
      ++g_fail;                                                        \
    }                                                                  \
  } while (0)

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: float_wide_plan_check graph.bin\n");
    return 2;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[2];
  if (std::fread(hdr, 4, 2, f) != 2) return 2;
  const int32_t n_v = hdr[0], n_c = hdr[1];
  if (n_v <= 0 || n_c <= 0) return 2;
  std::vector<int32_t> indptr((size_t)n_c + 1);
  if (std::fread(indptr.data(), 4, indptr.size(), f) != indptr.size() || indptr[n_c] <= 0) return 2;
  std::vector<int32_t> cols((size_t)indptr[n_c]);
  if (std::fread(cols.data(), 4, cols.size(), f) != cols.size()) return 2;
  std::fclose(f);
  const int64_t E = indptr[n_c];

  HostGraph g;
  g.n_v = n_v;
  g.n_c = n_c;
  g.n_e = E;
  g.h_cn_start.resize(n_c);
  g.h_cn_deg.resize(n_c);
  g.h_vn_start.resize(n_v);
  g.h_vn_deg.resize(n_v);
  g.h_tgt_vn.resize(E);
  g.h_cols = cols;
  std::vector<int32_t> tgt_cn(E);
  std::string err;
  if (!map_node_connections(n_v, n_c, indptr.data(), cols.data(), g.h_cn_start.data(), g.h_cn_deg.data(),
                            tgt_cn.data(), g.h_vn_start.data(), g.h_vn_deg.data(), g.h_tgt_vn.data(), &err)) {
    std::fprintf(stderr, "map_node_connections: %s\n", err.c_str());
    return 1;
  }
  int32_t dcm = 0, dvm = 0;
  for (int32_t d : g.h_cn_deg) dcm = std::max(dcm, d);
  for (int32_t d : g.h_vn_deg) dvm = std::max(dvm, d);

  // small-batch check tasks: lane i of a task reads and targets rows st .. st + d - 1 of its check
  int32_t heavy = 0;
  const std::vector<int32_t> info = work_order(g.h_cn_start, g.h_cn_deg, &heavy);
  const std::vector<int32_t> tasks = order_tasks(info);
  std::vector<char> row_seen((size_t)E, 0);
  int64_t small_rows = 0;
  int32_t wide_tasks = 0;
  for (size_t t = 0; t < tasks.size() / 4; ++t) {
    const int32_t p0 = tasks[4 * t], cnt = tasks[4 * t + 1], d = tasks[4 * t + 2], st1 = tasks[4 * t + 3];
    CHECK(cnt >= 1 && cnt <= 64 && d >= 1 && d <= dcm, "small-batch task record");
    wide_tasks += d > kMaxD;
    for (int32_t lane = 0; lane < cnt; ++lane) {
      const int32_t st = st1 != 0 ? st1 - 1 + lane * d : info[4 * (size_t)(p0 + lane) + 1];
      CHECK(info[4 * (size_t)(p0 + lane) + 2] == d, "task degree is its nodes' degree");
      for (int32_t j = 0; j < d; ++j) {
        const int64_t r = (int64_t)st + j;
        CHECK(r >= 0 && r < E, "small-batch row in range");
        if (r >= 0 && r < E) {
          CHECK(!row_seen[(size_t)r], "small-batch row owned once");
          row_seen[(size_t)r] = 1;
          CHECK(tgt_cn[(size_t)r] >= 0 && tgt_cn[(size_t)r] < E, "target row in range");
          ++small_rows;
        }
      }
    }
  }
  CHECK(small_rows == E, "small-batch tasks cover every edge");

  // fold plan: positions inside the check (any degree), destination rows, variables
  std::vector<int32_t> rec, rest;
  const int32_t n_folded = plan_fold(g, &rec, &rest);
  CHECK(rec.size() == (size_t)n_c * kFoldRec, "fold records");
  CHECK((int64_t)rest.size() + n_folded == n_v, "folded + rest = variables");
  int32_t fold_above16 = 0, n_rec = 0;
  for (int32_t c = 0; c < n_c; ++c) {
    const int32_t* r = &rec[(size_t)kFoldRec * c];
    for (int k = 0; k < 2; ++k) {
      if (r[k] < 0) continue;
      ++n_rec;
      CHECK(r[k] < g.h_cn_deg[c], "fold position below the check's degree");
      fold_above16 += r[k] >= kMaxD;
      CHECK(r[2 + k] >= 0 && r[2 + k] < E, "fold destination row in range");
      CHECK(r[4 + k] >= 0 && r[4 + k] < n_v && g.h_vn_deg[r[4 + k]] == 2, "fold variable has degree 2");
      if (r[k] < g.h_cn_deg[c]) CHECK(cols[(size_t)g.h_cn_start[c] + r[k]] == r[4 + k], "fold position holds the variable");
    }
    if (r[0] >= 0 && r[1] >= 0) CHECK(r[0] != r[1], "two folds of a check at distinct positions");
  }
  CHECK(n_rec == 2 * n_folded, "every folded variable has a record in both of its checks");

  // fused task tables (both variable orders), as fused_setup builds them when the code fits
  int64_t fused_slots = 0;
  int32_t fused_wide_tasks = 0;
  const bool fits = E < 65536 && (size_t)(E + n_v) * 16 <= 160u * 1024u;
  for (int order = 0; fits && order < 2; ++order) {
    FusedTasks ft;
    build_fused_tasks(g, &ft, order == 1, 8);
    std::vector<char> slot_seen((size_t)E, 0);
    int64_t next = 0;
    int32_t last_d = 1 << 30;
    for (size_t t = 0; t < ft.cn_task.size() / 4; ++t) {
      const int32_t first = ft.cn_task[4 * t], cnt = ft.cn_task[4 * t + 1], d = ft.cn_task[4 * t + 2];
      CHECK(first == next && cnt >= 1 && cnt <= 64 && d >= 1 && d <= dcm && d <= last_d, "fused check task record");
      last_d = d;
      if (order == 0) fused_wide_tasks += d > kMaxD;
      for (int32_t lane = 0; lane < cnt; ++lane)
        for (int32_t j = 0; j < d; ++j) {
          const int64_t s = (int64_t)first + (int64_t)j * cnt + lane;
          CHECK(s >= 0 && s < E, "fused check slot in range");
          if (s >= 0 && s < E) {
            CHECK(!slot_seen[(size_t)s], "fused check slot owned once");
            slot_seen[(size_t)s] = 1;
          }
        }
      next += (int64_t)cnt * d;
    }
    CHECK(next == E, "fused check tasks cover every slot");
    pad_vn_slots(&ft);
    std::vector<int32_t> uses((size_t)E, 0);
    size_t pos = 0;
    for (size_t t = 0; t < ft.vn_task.size() / 4; ++t) {
      const int32_t p0 = ft.vn_task[4 * t], cnt = ft.vn_task[4 * t + 1], d = ft.vn_task[4 * t + 2], sf = ft.vn_task[4 * t + 3];
      CHECK(p0 == (int32_t)pos && cnt >= 1 && cnt <= 64 && d >= 1 && d <= dvm, "fused variable task record");
      CHECK(sf >= 0 && (size_t)sf + (size_t)64 * d <= ft.vn_slot.size(), "padded slot rows in range");
      for (int32_t k = 0; k < d; ++k)
        for (int32_t lane = 0; lane < 64; ++lane) {
          const size_t i = (size_t)sf + (size_t)64 * k + lane;
          if (i >= ft.vn_slot.size()) continue;
          const int32_t s = ft.vn_slot[i];
          CHECK(s >= 0 && s < E && s < 65536, "variable slot index fits 16 bits and the message array");
          if (lane < cnt && s >= 0 && s < E) ++uses[(size_t)s];
        }
      pos += cnt;
    }
    CHECK(pos == (size_t)n_v && ft.vn_node.size() == (size_t)n_v, "fused variable tasks cover every variable");
    for (int64_t s = 0; s < E; ++s) CHECK(uses[(size_t)s] == 1, "every slot is one variable edge");
    fused_slots = (int64_t)ft.vn_slot.size();
  }

  std::printf("{\"n_v\": %d, \"n_c\": %d, \"E\": %lld, \"dcm\": %d, \"dvm\": %d, \"wide\": %d, \"small_tasks\": %zu, "
              "\"small_wide_tasks\": %d, \"folded\": %d, \"fold_positions_above_16\": %d, \"fits_fused\": %d, "
              "\"fused_wide_tasks\": %d, \"fused_vn_slots\": %lld, \"failures\": %d}\n",
              n_v, n_c, (long long)E, dcm, dvm, dcm > kMaxD ? 1 : 0, tasks.size() / 4, wide_tasks, n_folded,
              fold_above16, fits ? 1 : 0, fused_wide_tasks, (long long)fused_slots, g_fail);
  return g_fail ? 1 : 0;
}
