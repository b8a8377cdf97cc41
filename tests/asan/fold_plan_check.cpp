// CPU-only checker of the IB fast path's degree-2 variable fold plan (plan_ib_fold and the keyed work orders of
// informationbottleneckdecodingldpc_amd/csrc/plan.h), built by tests/test_cpu_fold_plan.py with
// -fsanitize=address,undefined -fno-sanitize-recover=all.
//
//   fold_plan_check <graph.bin>
// graph.bin: int32 n_v, n_c, indptr[n_c + 1], cols[E] (canonical CSR of H). Checks the plan's invariants and
// prints one JSON line {n_v, n_c, n_e, folded, rest, classes: [c0, c1, c2, c3], by_degree: {"D": [c0, c1, c2, c3],
// ...} (the class counts of every check degree present), failures}. Exit status 0 = every invariant held.
#include <array>
#include <cstdio>
#include <cstdlib>
#include <map>
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
    std::fprintf(stderr, "usage: fold_plan_check graph.bin\n");
    return 2;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[2];
  if (std::fread(hdr, 4, 2, f) != 2) return 2;
  const int32_t n_v = hdr[0], n_c = hdr[1];
  if (n_v <= 0 || n_c <= 0) return 2;
  std::vector<int32_t> indptr((size_t)n_c + 1);
  if (std::fread(indptr.data(), 4, indptr.size(), f) != indptr.size()) return 2;
  const int64_t E = indptr[n_c];
  std::vector<int32_t> cols((size_t)E);
  if (std::fread(cols.data(), 4, cols.size(), f) != cols.size()) return 2;
  std::fclose(f);

  HostGraph g;
  g.n_v = n_v; g.n_c = n_c; g.n_e = E;
  g.h_cn_start.resize(n_c); g.h_cn_deg.resize(n_c); g.h_vn_start.resize(n_v); g.h_vn_deg.resize(n_v);
  g.h_tgt_vn.resize((size_t)E);
  g.h_cols = cols;
  std::vector<int32_t> tgt_cn((size_t)E);
  std::string err;
  if (!map_node_connections(n_v, n_c, indptr.data(), cols.data(), g.h_cn_start.data(), g.h_cn_deg.data(),
                            tgt_cn.data(), g.h_vn_start.data(), g.h_vn_deg.data(), g.h_tgt_vn.data(), &err)) {
    std::fprintf(stderr, "map_node_connections: %s\n", err.c_str());
    return 2;
  }

  std::vector<int32_t> rec, rest;
  const int32_t n = plan_ib_fold(g, &rec, &rest);
  CHECK(rec.size() == (size_t)n_c * kIbFoldRec, "record size");
  std::vector<int32_t> chk_of((size_t)E);
  for (int32_t c = 0; c < n_c; ++c)
    for (int32_t k = 0; k < g.h_cn_deg[c]; ++k) chk_of[(size_t)g.h_cn_start[c] + k] = c;
  // per check: the folded positions are within the last two, name degree-2 variables, and the variable's other
  // edge is folded in its own check with this edge as ITS other edge
  std::vector<int32_t> times((size_t)n_v, 0);
  long classes[4] = {0, 0, 0, 0};
  std::map<int32_t, std::array<long, 4>> by_degree;
  for (int32_t c = 0; c < n_c; ++c) {
    const int32_t* r = &rec[(size_t)kIbFoldRec * c];
    const int32_t d = g.h_cn_deg[c], st = g.h_cn_start[c];
    CHECK(r[0] >= 0 && r[0] <= 3, "class range");
    if (r[0] < 0 || r[0] > 3) continue;
    ++classes[r[0]];
    ++by_degree.try_emplace(d, std::array<long, 4>{0, 0, 0, 0}).first->second[r[0]];
    if (r[0]) CHECK(d >= 3, "a folding check has degree >= 3");
    for (int a = 0; a < 2; ++a) {
      if (d >= 2) CHECK(r[1 + a] == cols[(size_t)st + d - 2 + a], "channel row = the input's variable");
      if (!((r[0] >> a) & 1)) {
        CHECK(r[3 + a] == -1, "unfolded slot has no destination");
        continue;
      }
      const int32_t e = st + d - 2 + a, v = r[1 + a], o = r[3 + a];
      CHECK(v >= 0 && v < n_v && g.h_vn_deg[v] == 2, "folded variable has degree 2");
      CHECK(o >= 0 && o < E && o != e, "other edge in range");
      if (v < 0 || v >= n_v || o < 0 || o >= E) continue;
      ++times[v];
      CHECK(cols[(size_t)o] == v, "other edge belongs to the same variable");
      const int32_t c2 = chk_of[(size_t)o], d2 = g.h_cn_deg[c2], k2 = o - g.h_cn_start[c2];
      CHECK(k2 >= d2 - 2 && d2 >= 3, "other edge within the last two inputs of its check");
      if (k2 < d2 - 2 || k2 >= d2) continue;
      const int32_t* r2 = &rec[(size_t)kIbFoldRec * c2];
      const int a2 = k2 - (d2 - 2);
      CHECK(((r2[0] >> a2) & 1) && r2[3 + a2] == e, "the other edges are each other's");
    }
  }
  // folded in both checks or in neither; rest and folded partition the variables
  std::vector<char> in_rest((size_t)n_v, 0);
  for (int32_t v : rest) {
    CHECK(v >= 0 && v < n_v && !in_rest[v], "rest list entries distinct and in range");
    if (v >= 0 && v < n_v) in_rest[v] = 1;
  }
  int32_t cnt = 0;
  for (int32_t v = 0; v < n_v; ++v) {
    CHECK(times[v] == 0 || times[v] == 2, "folded in both checks or in neither");
    CHECK((times[v] == 2) != (in_rest[v] != 0), "rest and folded partition the variables");
    cnt += times[v] == 2;
  }
  CHECK(cnt == n && (size_t)n + rest.size() == (size_t)n_v, "folded count");
  for (size_t i = 1; i < rest.size(); ++i) CHECK(rest[i] > rest[i - 1], "rest ascending");

  // keyed work orders: checks by (degree desc, class asc), the rest list by degree desc
  std::vector<int32_t> cls((size_t)n_c), all((size_t)n_c);
  for (int32_t c = 0; c < n_c; ++c) {
    cls[c] = rec[(size_t)kIbFoldRec * c];
    all[c] = c;
  }
  int32_t heavy = -1, h = 0;
  const std::vector<int32_t> ci = work_order_keyed(all, g.h_cn_start, g.h_cn_deg, &cls, &heavy);
  CHECK(ci.size() == (size_t)4 * n_c, "check order size");
  std::vector<char> seen((size_t)n_c, 0);
  for (int32_t p = 0; p < n_c && ci.size() == (size_t)4 * n_c; ++p) {
    const int32_t c = ci[4 * p];
    CHECK(c >= 0 && c < n_c && !seen[c], "check order is a permutation");
    if (c < 0 || c >= n_c) continue;
    seen[c] = 1;
    CHECK(ci[4 * p + 1] == g.h_cn_start[c] && ci[4 * p + 2] == g.h_cn_deg[c] && ci[4 * p + 3] == cls[c], "check record");
    if (p) {
      const bool ok = ci[4 * p + 2] < ci[4 * (p - 1) + 2] ||
                      (ci[4 * p + 2] == ci[4 * (p - 1) + 2] && ci[4 * p + 3] >= ci[4 * (p - 1) + 3]);
      CHECK(ok, "heaviest first, class second");
    }
    h += g.h_cn_deg[c] > kLightD;
  }
  CHECK(h == heavy, "heavy checks");
  heavy = -1;
  h = 0;
  const std::vector<int32_t> vi = work_order_keyed(rest, g.h_vn_start, g.h_vn_deg, nullptr, &heavy);
  CHECK(vi.size() == 4 * rest.size(), "rest order size");
  std::vector<char> vseen((size_t)n_v, 0);
  for (size_t p = 0; p < rest.size() && vi.size() == 4 * rest.size(); ++p) {
    const int32_t v = vi[4 * p];
    CHECK(v >= 0 && v < n_v && in_rest[v] && !vseen[v], "rest order is a permutation of the rest list");
    if (v < 0 || v >= n_v) continue;
    vseen[v] = 1;
    CHECK(vi[4 * p + 1] == g.h_vn_start[v] && vi[4 * p + 2] == g.h_vn_deg[v] && vi[4 * p + 3] == 0, "rest record");
    if (p) CHECK(vi[4 * p + 2] <= vi[4 * (p - 1) + 2], "rest heaviest first");
    h += g.h_vn_deg[v] > kLightD;
  }
  CHECK(h == heavy, "heavy variables of the rest");

  std::printf("{\"n_v\": %d, \"n_c\": %d, \"n_e\": %lld, \"folded\": %d, \"rest\": %zu, "
              "\"classes\": [%ld, %ld, %ld, %ld], \"by_degree\": {",
              n_v, n_c, (long long)E, n, rest.size(), classes[0], classes[1], classes[2], classes[3]);
  const char* sep = "";
  for (const auto& kv : by_degree) {
    std::printf("%s\"%d\": [%ld, %ld, %ld, %ld]", sep, kv.first, kv.second[0], kv.second[1], kv.second[2],
                kv.second[3]);
    sep = ", ";
  }
  std::printf("}, \"failures\": %d}\n", g_fail);
  return g_fail ? 1 : 0;
}
