// CPU-only checker of the fixed-point fused layered kernel's host geometry (fixfused_ldn / fixfused_cw_bytes /
// fixfused_cw_per_group / fixfused_buf_bytes / fixfused_stage_tiles of
// informationbottleneckdecodingldpc_amd/csrc/layered_plan.h, over plan_layered's tasks), built by
// tests/test_cpu_layered_fixed_fused.py with -fsanitize=address,undefined -fno-sanitize-recover=all.
//
//   layered_fixed_fused_plan_check <graph.bin> <max_batch>
// graph.bin: the format of layered_plan_check.cpp. Walks the byte and word offsets the layfix_fused* kernels form —
// a wave's slice of LDS, its row of the staging buffer, every task's index rows and state slots, every dword of
// every staging tile of a batch of max_batch — against a model of the arrays (an LDS image of the workgroup and the
// staging buffer are allocated at their planned sizes and written at every offset, so an offset past them is an
// AddressSanitizer report) and prints one JSON line {valid, error, wide, n_tasks, ldn, cw_bytes, uncapped,
// cw_per_group, lds_bytes, buf_bytes, stage_tiles, ngroups, failures}; exit status 0 = the layers were judged and,
// when valid, every invariant held. A code that does not fit (cw_per_group 0) is reported with the sizes alone.
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
    std::fprintf(stderr, "usage: layered_fixed_fused_plan_check graph.bin max_batch\n");
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

  // the fit rule on sizes alone, whatever the graph
  CHECK(kLayFixFusedMaxCw >= 1 && kLayFixFusedMaxCw <= kLayFixFusedBoundCw && kLayFixFusedBoundCw <= 16,
        "at most 1,024 threads");
  CHECK(fixfused_ldn(1) == 4 && fixfused_ldn(4) == 4 && fixfused_ldn(5) == 8 && fixfused_ldn(5399) == 5400 &&
            fixfused_ldn(0x7ffffffc) == 0x7ffffffc,
        "ldn rounds up to 4");
  CHECK(fixfused_cw_bytes(1944, 972) == 5832 && fixfused_cw_per_group(1944, 972) == kLayFixFusedMaxCw &&
            fixfused_cw_per_group(1944, 972, false, 16) == 16 &&
            fixfused_cw_per_group(1944, 972, false, 8) == 8 && kLayLds / 5832 == 28, "WLAN N = 1944");
  CHECK(fixfused_cw_bytes(16200, 9000) == 52200 && fixfused_cw_per_group(16200, 9000) == 3, "N = 16200");
  CHECK(fixfused_cw_bytes(64800, 32400) == 194400 && fixfused_cw_per_group(64800, 32400) == 0, "N = 64800 does not fit");
  CHECK(fixfused_cw_bytes(11160, 1080, true) == 19800 && fixfused_cw_per_group(11160, 1080, true, 16) == 8, "wide");

  std::string err;
  const int rc = validate_layers(n_v, n_c, indptr.data(), cols.data(), n_layers, lptr.data(), lchk.data(), &err);
  bool wide = false;
  int32_t ldn = 0, cw = 0, uncapped = 0, n_tasks = 0, ngroups = 0;
  size_t cw_bytes = 0, lds = 0, buf_bytes = 0;
  int64_t tiles = 0;
  if (rc == 0) {
    wide = layered_is_wide(n_c, indptr.data());
    ldn = fixfused_ldn(n_v);
    cw_bytes = fixfused_cw_bytes(n_v, n_c, wide);
    cw = fixfused_cw_per_group(n_v, n_c, wide);
    uncapped = (int32_t)((size_t)kLayLds / cw_bytes);
    buf_bytes = fixfused_buf_bytes(n_v, B);
    tiles = fixfused_stage_tiles(n_v, B);
    CHECK(ldn >= n_v && ldn < n_v + 4 && ldn % 4 == 0, "ldn");
    CHECK(cw_bytes == (size_t)ldn + (size_t)(wide ? 8 : 4) * n_c && cw_bytes % 4 == 0, "cw_bytes");
    CHECK(cw == std::min<int32_t>(kLayFixFusedMaxCw, uncapped), "cw_per_group");
    CHECK(buf_bytes == (size_t)B * (size_t)ldn, "staging buffer bytes");
    for (int32_t cap = 1; cap <= kLayFixFusedBoundCw; ++cap)
      CHECK(fixfused_cw_per_group(n_v, n_c, wide, cap) == std::min<int32_t>(cap, uncapped), "a lower cap");
  }
  if (rc == 0 && cw >= 1) {
    lds = (size_t)cw * cw_bytes;
    CHECK(lds <= (size_t)kLayLds, "the workgroup's slices fit the LDS");
    ngroups = (B + cw - 1) / cw;
    CHECK((int64_t)ngroups * cw >= B && (int64_t)(ngroups - 1) * cw < B, "groups cover the batch");
    LayeredPlan pl;
    plan_layered(n_v, n_c, indptr.data(), cols.data(), n_layers, lptr.data(), lchk.data(), &pl);
    n_tasks = pl.n_tasks;
    std::vector<unsigned char> image(lds, 0);   // the workgroup's LDS
    std::vector<unsigned char> buf(buf_bytes, 0);
    // a wave's slice and its codeword row, as layfix_fused_body addresses them: first and last wave, the batch's
    // first and last codeword
    for (int32_t wave : {0, cw - 1}) {
      const size_t base = (size_t)wave * cw_bytes;
      CHECK((base + (size_t)ldn) % 4 == 0, "state words are aligned");
      for (int lane = 0; lane < 64; ++lane)
        for (int32_t v = 4 * lane; v < ldn; v += 256) {
          CHECK(v + 3 < ldn, "a row dword lies inside the row");
          for (int i = 0; i < 4; ++i) image[base + (size_t)v + i] = 1;
          for (int32_t b : {0, B - 1})
            for (int i = 0; i < 4; ++i) buf[(size_t)b * (size_t)ldn + (size_t)v + i] = 1;
        }
      for (int32_t c = 0; c < n_c; ++c)
        for (int w = 0; w < (wide ? 2 : 1); ++w) {
          const size_t at = base + (size_t)ldn + 4 * ((size_t)w * n_c + (size_t)c);
          CHECK(at + 4 <= base + cw_bytes, "a state word lies inside the slice");
          for (int i = 0; i < 4; ++i) image[at + i] = 2;
        }
      size_t p_bytes = 0;
      for (size_t i = 0; i < (size_t)ldn; ++i) p_bytes += image[base + i] == 1;
      CHECK(p_bytes == (size_t)ldn, "the row load covers P and the state words do not reach into it");
    }
    // every task: index rows inside idx, variables inside P, slots inside the state, each check once
    std::vector<int32_t> seen((size_t)n_c, 0);
    std::vector<int32_t> owner((size_t)n_v, -1);
    int32_t layer = 0;
    for (int32_t t = 0; t < pl.n_tasks; ++t) {
      while (layer + 1 <= n_layers && t >= pl.layer_task[(size_t)layer + 1]) {
        ++layer;
        std::fill(owner.begin(), owner.end(), -1);
      }
      const int32_t first = pl.task[4 * (size_t)t], cnt = pl.task[4 * (size_t)t + 1], d = pl.task[4 * (size_t)t + 2],
                    s0 = pl.task[4 * (size_t)t + 3];
      CHECK(cnt >= 1 && cnt <= 64 && d >= kLayMinD && d <= (wide ? kLayWideMaxD : kLayMaxD), "task shape");
      CHECK(first >= 0 && (size_t)first + (size_t)64 * d <= pl.idx.size(), "index rows inside idx");
      for (int32_t lane = 0; lane < cnt; ++lane) {
        const int32_t slot = s0 + lane;
        CHECK(slot >= 0 && slot < n_c, "slot inside the state");
        if (slot >= 0 && slot < n_c) ++seen[(size_t)slot];
        for (int32_t k = 0; k < d; ++k) {
          const int32_t v = pl.idx[(size_t)first + (size_t)64 * k + lane];
          CHECK(v >= 0 && v < n_v, "variable inside P");
          if (v < 0 || v >= n_v) continue;
          // the byte accesses rest on this: no two checks of a layer share a byte of P
          CHECK(owner[(size_t)v] < 0 || owner[(size_t)v] == slot, "a layer's checks share no variable");
          owner[(size_t)v] = slot;
          image[(size_t)(cw - 1) * cw_bytes + (size_t)v] = 3;
        }
      }
    }
    for (int32_t c = 0; c < n_c; ++c) CHECK(seen[(size_t)c] == 1, "every slot is updated once per iteration");
    // the staging tiles: every dword of every codeword row, once
    const int64_t tiles_x = ((int64_t)B + 63) / 64;
    CHECK(tiles == tiles_x * (((int64_t)ldn + 63) / 64) && tiles <= 0x7fffffffll, "staging grid");
    std::fill(buf.begin(), buf.end(), 0);
    for (int64_t blk = 0; blk < tiles; ++blk) {
      const size_t r0 = (size_t)(blk / tiles_x) * 64, c0 = (size_t)(blk % tiles_x) * 64;
      for (int id = 0; id < 1024; ++id) {
        const int q = id & 15, j = id >> 4;
        const size_t c = c0 + j, r = r0 + 4 * q;
        if (c < (size_t)B && r < (size_t)ldn)
          for (int i = 0; i < 4; ++i) ++buf[c * (size_t)ldn + r + i];
      }
    }
    size_t once = 0;
    for (unsigned char x : buf) once += x == 1;
    CHECK(once == buf_bytes, "the tiles' dwords cover the staging buffer exactly once");
  }
  std::string esc;
  for (char ch : err) esc += (ch == '"' || ch == '\\') ? '?' : ch;
  std::printf("{\"valid\": %d, \"error\": \"%s\", \"wide\": %d, \"n_tasks\": %d, \"ldn\": %d, \"cw_bytes\": %zu, "
              "\"uncapped\": %d, \"cw_per_group\": %d, \"lds_bytes\": %zu, \"buf_bytes\": %zu, \"stage_tiles\": %lld, "
              "\"ngroups\": %d, \"failures\": %d}\n",
              rc, esc.c_str(), wide ? 1 : 0, n_tasks, ldn, cw_bytes, uncapped, cw, lds, buf_bytes, (long long)tiles,
              ngroups, g_fail);
  return g_fail ? 1 : 0;
}
