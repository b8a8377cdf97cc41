// CPU-only checker of the wide layered decoder's host plan (check degrees up to kLayWideMaxD = 32:
// layered_is_wide, the wide forms of layered_cw_bytes / layered_cw_per_group / plan_layered / pass_bytes /
// pass_compact_rows / fix_bytes and fix_state_words_wide of informationbottleneckdecodingldpc_amd/csrc/layered_plan.h),
// built by tests/test_cpu_layered_wide.py with -fsanitize=address,undefined -fno-sanitize-recover=all.
//
//   layered_wide_plan_check <graph.bin> <max_batch>
// graph.bin: the format of layered_plan_check.cpp. Walks the fused plan's tasks and every item of every per-layer
// launch of a batch of max_batch the way the lay_*_wide / layfix_*_wide kernels index, fp32 and fixed point, and
// prints one JSON line; exit status 0 = the layers were judged and, when valid, every invariant held. A narrow code
// (no check above degree 16) must get exactly the sizes the narrow functions always gave.
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
    std::fprintf(stderr, "usage: layered_wide_plan_check graph.bin max_batch\n");
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

  // the wide fixed-point words, whatever the graph: every m1, m2 in 0..63, pos in 0..31, sign masks with bit 31
  CHECK(kLayMaxD == 16 && kLayWideMaxD == 32 && kLayFixQMax == 63, "field widths hold the ranges");
  for (uint32_t m1 = 0; m1 <= 63; ++m1)
    for (uint32_t m2 = 0; m2 <= 63; ++m2)
      for (uint32_t pos = 0; pos <= 31; ++pos)
        for (uint32_t sg : {0u, 1u, 0x80000000u, 0xffffffffu, 0xaaaaaaaau, 0x55555555u, 0x80000001u}) {
          const FixWideWords w = fix_state_words_wide(m1, m2, pos, sg);
          CHECK(fix_wide_m1(w.w0) == m1 && fix_wide_m2(w.w0) == m2 && fix_wide_pos(w.w0) == pos && w.w1 == sg &&
                    (w.w0 >> 17) == 0u, "wide state words round-trip");
        }
  for (int d = 1; d <= 32; ++d) {
    const uint64_t want = (1ull << d) - 1ull;
    CHECK((uint64_t)fix_wide_mask(d) == want, "the low D bits");
  }

  std::string err;
  const int rc = validate_layers(n_v, n_c, indptr.data(), cols.data(), n_layers, lptr.data(), lchk.data(), &err);
  int wide = 0, max_d = 0, n_tasks = 0, cw_per_group = 0;
  size_t cw_bytes = 0;
  LayeredPassBytes pb;
  LayeredFixBytes fb;
  int64_t compact_rows = 0;
  if (rc == 0) {
    for (int32_t c = 0; c < n_c; ++c) max_d = std::max(max_d, indptr[c + 1] - indptr[c]);
    wide = layered_is_wide(n_c, indptr.data()) ? 1 : 0;
    CHECK(wide == (max_d > kLayMaxD ? 1 : 0) && max_d <= kLayWideMaxD, "wide iff some degree is above 16");
    const bool w = wide != 0;

    // ---- fused plan
    LayeredPlan pl;
    plan_layered(n_v, n_c, indptr.data(), cols.data(), n_layers, lptr.data(), lchk.data(), &pl);
    n_tasks = pl.n_tasks; cw_per_group = pl.cw_per_group; cw_bytes = pl.cw_bytes;
    CHECK(pl.wide == w, "the plan knows");
    CHECK(pl.cw_bytes == (size_t)4 * n_v + (size_t)(w ? 16 : 12) * n_c, "bytes per codeword");
    CHECK(pl.cw_bytes == layered_cw_bytes(n_v, n_c, w) && pl.cw_per_group == layered_cw_per_group(n_v, n_c, w),
          "the plan uses the handle's fit rule");
    CHECK(layered_cw_bytes(n_v, n_c) == (size_t)4 * n_v + (size_t)12 * n_c &&
              layered_cw_bytes(n_v, n_c, false) == layered_cw_bytes(n_v, n_c), "narrow bytes are what they were");
    CHECK(pl.cw_per_group >= 0 && pl.cw_per_group <= kLayMaxCw &&
              (size_t)pl.cw_per_group * pl.cw_bytes <= (size_t)kLayLds, "codewords per workgroup fit the LDS");
    CHECK(pl.cw_per_group == kLayMaxCw || (size_t)(pl.cw_per_group + 1) * pl.cw_bytes > (size_t)kLayLds,
          "as many codewords as fit");
    // the wave's LDS slice: P, M1, M2, PS and (wide) PO, each within cw_bytes
    CHECK((size_t)4 * ((size_t)n_v + (size_t)(w ? 4 : 3) * n_c) == pl.cw_bytes, "the state arrays fill the slice");
    CHECK(pl.task.size() == (size_t)4 * pl.n_tasks && pl.layer_task.size() == (size_t)n_layers + 1, "table sizes");
    std::vector<int32_t> check_of_slot((size_t)n_c, -1);
    for (int32_t c = 0; c < n_c; ++c) {
      const int32_t s = pl.slot_of[c];
      CHECK(s >= 0 && s < n_c && check_of_slot[s] < 0, "state slots are a permutation of the checks");
      if (s >= 0 && s < n_c) check_of_slot[s] = c;
    }
    int32_t slot = 0;
    size_t first = 0;
    for (int32_t t = 0; t < pl.n_tasks; ++t) {
      const int32_t* r = &pl.task[(size_t)4 * t];
      const int32_t cnt = r[1], d = r[2];
      CHECK((size_t)r[0] == first && r[3] == slot, "tasks are contiguous");
      CHECK(cnt >= 1 && cnt <= 64 && d >= kLayMinD && d <= kLayWideMaxD, "task shape");
      CHECK(first + (size_t)64 * d <= pl.idx.size() && slot + cnt <= n_c, "index rows and slots within the tables");
      if (cnt < 1 || cnt > 64 || d < kLayMinD || d > kLayWideMaxD || first + (size_t)64 * d > pl.idx.size() ||
          slot + cnt > n_c)
        break;
      for (int32_t lane = 0; lane < 64; ++lane) {
        const int32_t c = lane < cnt ? check_of_slot[(size_t)slot + lane] : -1;
        if (lane < cnt) {
          CHECK(c >= 0 && indptr[c + 1] - indptr[c] == d, "a task's checks have its degree");
          if (c < 0) continue;
        }
        for (int32_t k = 0; k < d; ++k) {
          const int32_t v = pl.idx[first + (size_t)64 * k + lane];
          CHECK(v >= 0 && v < n_v, "variable index in range (padding included)");
          if (lane < cnt) CHECK(v == cols[(size_t)indptr[c] + k], "edge k of a check in ascending column order");
        }
      }
      slot += cnt;
      first += (size_t)64 * d;
    }
    CHECK(slot == n_c && first == pl.idx.size(), "every check planned once");

    // ---- per-layer path, fp32
    LayeredPassPlan pp;
    plan_layered_passes(n_c, indptr.data(), n_layers, lptr.data(), lchk.data(), &pp);
    pb = pass_bytes(n_v, n_c, B, w);
    const LayeredPassBytes nb = pass_bytes(n_v, n_c, B);
    const int32_t ntiles = pass_tiles(B);
    const size_t ldb = (size_t)pass_ldb(B);
    CHECK(nb.total == nb.P + 3 * nb.state + 2 * nb.mask + nb.counter + nb.bits, "narrow total is what it was");
    CHECK(pb.P == nb.P && pb.state == nb.state && pb.mask == nb.mask && pb.bits == nb.bits, "the arrays keep their sizes");
    CHECK(pb.state == (size_t)4 * n_c * ldb && pb.total == nb.total + (w ? pb.state : 0), "wide adds one state array");
    compact_rows = pass_compact_rows(n_v, n_c, w);
    CHECK(pass_compact_rows(n_v, n_c) == (int64_t)n_v + 3 * (int64_t)n_c &&
              compact_rows == (int64_t)n_v + (w ? 4 : 3) * (int64_t)n_c, "rows of the compaction move");
    // the row move's items: every item names one row of one array, inside it
    for (int64_t item : {(int64_t)0, (int64_t)n_v - 1, (int64_t)n_v, compact_rows - 1}) {
      if (item < n_v) continue;
      const int64_t r = item - n_v;
      const int which = (int)(r / n_c);
      CHECK(which >= 0 && which < pass_state_arrays(w) && (size_t)(r % n_c) * ldb + ldb <= pb.state / 4,
            "a state row of the move within its array");
    }
    const size_t fix_ldb_ = (size_t)fix_ldb(B);
    fb = fix_bytes(n_v, n_c, B, w);
    const LayeredFixBytes fn = fix_bytes(n_v, n_c, B);
    CHECK(fn.state == (size_t)4 * n_c * fix_ldb_ && fn.total == fn.P + fn.state + 2 * fn.mask + fn.counter + fn.bits,
          "narrow fixed sizes are what they were");
    CHECK(fb.P == fn.P && fb.mask == fn.mask && fb.bits == fn.bits && fb.state == (w ? 2 : 1) * fn.state &&
              fb.total == fn.total + (w ? fn.state : 0), "wide fixed: a second state array");
    const size_t S_words = fb.state / (w ? 8 : 4);   // words of each state array
    const int32_t ntiles4 = fix_tiles(B);
    for (int32_t l = 0; l < n_layers; ++l) {
      const int32_t n = lptr[l + 1] - lptr[l];
      // fp32: lay_layer_wide — uniform row base + tile base, lane within the tile
      for (int64_t item = 0; item < pass_items(n, B); ++item) {
        const int32_t tile = (int32_t)(item % ntiles), s = pp.layer_slot[l] + (int32_t)(item / ntiles);
        CHECK(s >= lptr[l] && s < lptr[l + 1], "item -> slot of the layer");
        if (s < 0 || s >= n_c) continue;
        const int32_t e0 = pp.rec[(size_t)2 * s], d = pp.rec[(size_t)2 * s + 1];
        CHECK(d >= kLayMinD && d <= kLayWideMaxD && e0 >= 0 && (size_t)e0 + d <= cols.size(), "check record");
        const size_t tcol = (size_t)tile * kLayTile, srow = (size_t)s * ldb + tcol;
        CHECK(srow + (kLayTile - 1) < pb.state / 4, "a wave's state words within each state array");
        for (int32_t k = 0; k < d; ++k)
          CHECK((size_t)cols[(size_t)e0 + k] * ldb + tcol + (kLayTile - 1) < pb.P / 4, "a wave's P words within P");
      }
      // fixed point: layfix_layer_wide — a lane's dword of a P row, its four words of each state array
      for (int64_t item = 0; item < fix_items(n, B); ++item) {
        const int32_t tile = (int32_t)(item % ntiles4), s = pp.layer_slot[l] + (int32_t)(item / ntiles4);
        if (s < 0 || s >= n_c) continue;
        const int32_t e0 = pp.rec[(size_t)2 * s], d = pp.rec[(size_t)2 * s + 1];
        const size_t tcol = (size_t)tile * kLayFixTile, srow = (size_t)s * fix_ldb_ + tcol;
        for (size_t lane : {(size_t)0, (size_t)63}) {
          CHECK((srow + 4 * lane) % 4 == 0 && srow + 4 * lane + 3 < S_words,
                "a lane's four state words: 16-byte aligned, within each array");
          for (int32_t k = 0; k < d; ++k) {
            const size_t at = (size_t)cols[(size_t)e0 + k] * fix_ldb_ + tcol + 4 * lane;
            CHECK(at % 4 == 0 && at + 3 < fb.P, "a lane's dword of a P row: aligned, within the scratch");
          }
        }
      }
    }
    // stage-in zeroes the state rows under row < n_c: the last row of every array lies inside it
    CHECK((size_t)(n_c - 1) * ldb + ldb == pb.state / 4 && (size_t)(n_c - 1) * fix_ldb_ + fix_ldb_ == S_words,
          "state rows fill their arrays");
  }
  std::string esc;
  for (char ch : err) esc += (ch == '"' || ch == '\\') ? '?' : ch;
  std::printf("{\"valid\": %d, \"error\": \"%s\", \"wide\": %d, \"max_degree\": %d, \"n_tasks\": %d, "
              "\"cw_per_group\": %d, \"cw_bytes\": %zu, \"pass_state\": %zu, \"pass_total\": %zu, "
              "\"compact_rows\": %lld, \"fix_state\": %zu, \"fix_total\": %zu, \"failures\": %d}\n",
              rc, esc.c_str(), wide, max_d, n_tasks, cw_per_group, cw_bytes, pb.state, pb.total,
              (long long)compact_rows, fb.state, fb.total, g_fail);
  return g_fail ? 1 : 0;
}
