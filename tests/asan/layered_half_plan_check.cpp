// CPU-only checker of the host plan of the layered BP decoder with half-precision state (layhp_cw_bytes,
// layhp_cw_per_group, plan_layered_bp_half, half_tiles, half_ldb, half_mask_words, half_done_word, layhp_pass_bytes of
// informationbottleneckdecodingldpc_amd/csrc/layered_plan.h, with plan_layered_passes for the per-layer records),
// built by tests/test_cpu_layered_half.py with -fsanitize=address,undefined -fno-sanitize-recover=all.
//
//   layered_half_plan_check <graph.bin> <max_batch>
// graph.bin: the format of layered_plan_check.cpp — int32 n_v, n_c, indptr[n_c + 1], cols[E] (canonical CSR of H),
// n_layers, layer_ptr[n_layers + 1], layer_checks[layer_ptr[n_layers]]. Walks every access of the fused kernel's
// tasks (2-byte words of the wave's P16[N] | R16[E] slice) and every row dword of every item of the per-layer launches
// of a batch of max_batch, the pack's 128-byte reads and the mask words, the way the kernels index, and prints one
// JSON line {valid, error, unsupported, n_e, n_tasks, cw_bytes, cw_per_group, ldb, mask_words, pad_words_all_ones,
// bytes_P, bytes_R, bytes_mask, bytes_total, failures}; exit status 0 = the layers were judged and, when the code is
// valid and supported, every invariant held.
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
    std::fprintf(stderr, "usage: layered_half_plan_check graph.bin max_batch\n");
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
  int32_t unsupported = -1, pad_ones = 0;
  LayeredBpPlan pl;
  LayeredBpBytes by;
  const int64_t E = indptr[n_c];
  int64_t ldb = 0, mask_words = 0;
  if (rc == 0) unsupported = laybp_unsupported_check(n_c, indptr.data());
  if (rc == 0 && unsupported >= 0) {
    const int32_t d = indptr[unsupported + 1] - indptr[unsupported];
    CHECK(d < kLayMinD || d > kLayBpMaxD, "the named check has no degree body");
    for (int32_t c = 0; c < unsupported; ++c)
      CHECK(indptr[c + 1] - indptr[c] >= kLayMinD && indptr[c + 1] - indptr[c] <= kLayBpMaxD, "it is the first");
  }
  if (rc == 0 && unsupported < 0) {
    plan_layered_bp_half(n_v, n_c, indptr.data(), cols.data(), n_layers, lptr.data(), lchk.data(), &pl);
    // ---- fused kernel ----
    LayeredBpPlan fp;
    plan_layered_bp(n_v, n_c, indptr.data(), cols.data(), n_layers, lptr.data(), lchk.data(), &fp);
    CHECK(pl.task == fp.task && pl.idx == fp.idx && pl.n_tasks == fp.n_tasks, "the task layout is the fp32 plan's");
    CHECK(pl.n_e == E, "the tasks hold every edge");
    const size_t raw = (size_t)2 * n_v + (size_t)2 * E;
    CHECK(pl.cw_bytes == (raw + 3) / 4 * 4 && pl.cw_bytes == layhp_cw_bytes(n_v, E), "codeword bytes");
    CHECK(pl.cw_bytes % 4 == 0 && pl.cw_bytes >= raw && pl.cw_bytes < raw + 4, "rounded up to a dword, no further");
    const size_t fit = (size_t)kLayLds / pl.cw_bytes;
    CHECK(pl.cw_per_group == (int32_t)(fit < (size_t)kLayMaxCw ? fit : (size_t)kLayMaxCw), "fit rule");
    CHECK(pl.cw_per_group == layhp_cw_per_group(n_v, E), "fit rule, by name");
    CHECK((size_t)pl.cw_per_group * pl.cw_bytes <= (size_t)kLayLds, "the group fits the LDS");
    CHECK(pl.cw_per_group >= laybp_cw_per_group(n_v, E), "never fewer codewords than the fp32 state");
    // the wave's slice as layhp_fused addresses it: halves [0, n_v) are P, [n_v, cw_bytes / 2) are R and what the
    // kernel zeroes
    const int64_t slice_halves = (int64_t)pl.cw_bytes / 2;
    CHECK(slice_halves - n_v >= E && slice_halves - n_v <= E + 1, "the zeroed range is R, or R and one half of padding");
    std::vector<int32_t> word_owner((size_t)E, -1);
    for (int32_t t = 0; t < pl.n_tasks; ++t) {
      const int32_t first = pl.task[(size_t)4 * t], cnt = pl.task[(size_t)4 * t + 1], d = pl.task[(size_t)4 * t + 2],
                    r0 = pl.task[(size_t)4 * t + 3];
      CHECK(cnt >= 1 && cnt <= 64 && d >= kLayMinD && d <= kLayBpMaxD, "task shape");
      CHECK(first >= 0 && (size_t)first + (size_t)64 * d <= pl.idx.size(), "index rows within idx");
      if (cnt < 1 || cnt > 64 || d < kLayMinD || d > kLayBpMaxD || r0 < 0) continue;
      for (int32_t lane = 0; lane < cnt; ++lane) {
        for (int32_t k = 0; k < d; ++k) {
          const int64_t w = (int64_t)r0 + (int64_t)cnt * k + lane;   // as layhp_cn addresses R
          CHECK(w >= 0 && w < E && n_v + w < slice_halves, "message half within the slice");
          if (w >= 0 && w < E) {
            CHECK(word_owner[(size_t)w] < 0, "no two edges share a message half");
            word_owner[(size_t)w] = t;
          }
          const size_t at = (size_t)first + (size_t)64 * k + (size_t)lane;
          if (at < pl.idx.size()) CHECK(pl.idx[at] >= 0 && pl.idx[at] < n_v, "variable index within P");
        }
      }
    }
    for (int64_t w = 0; w < E; ++w) CHECK(word_owner[(size_t)w] >= 0, "every message half is used");
    // ---- per-layer path ----
    LayeredPassPlan pp;
    plan_layered_passes(n_c, indptr.data(), n_layers, lptr.data(), lchk.data(), &pp);
    by = layhp_pass_bytes(n_v, E, B);
    const int32_t ntiles = pass_tiles(B), ntiles2 = half_tiles(B);
    ldb = half_ldb(B);
    mask_words = half_mask_words(B);
    CHECK(kLayHalfTile == 128 && kLayHalfCw == 2, "a lane owns two codewords, a wave 128");
    CHECK(ldb % kLayHalfTile == 0 && ldb >= B && ldb < (int64_t)B + kLayHalfTile, "ldb: B rounded up to 128");
    CHECK(ldb == (int64_t)ntiles2 * kLayHalfTile, "ldb is whole tiles");
    CHECK(mask_words == 2 * (int64_t)ntiles2 && mask_words >= ntiles && mask_words <= (int64_t)ntiles + 1,
          "mask words: whole tiles of 128");
    CHECK(by.P == (size_t)2 * n_v * (size_t)ldb && by.R == (size_t)2 * (size_t)E * (size_t)ldb, "row array bytes");
    CHECK(by.mask == (size_t)8 * (size_t)mask_words && by.counter == 4 && by.bits == (size_t)8 * n_v * ntiles,
          "mask, counter, bits");
    CHECK(by.total == by.P + by.R + 2 * by.mask + by.counter + by.bits, "total bytes");
    // the mask words as the stage-in writes them
    for (int64_t w = 0; w < mask_words; ++w) {
      const uint64_t m = half_done_word((int32_t)w, B);
      for (int b = 0; b < kLayTile; ++b)
        CHECK(((m >> b) & 1ull) == (uint64_t)(w * kLayTile + b >= B ? 1 : 0), "finished from the start iff past the batch");
      if (w >= ntiles) {
        CHECK(m == ~0ull, "a padding word is all ones");
        ++pad_ones;
      }
    }
    CHECK(pad_ones == (int32_t)(mask_words - ntiles), "every padding word counted");
    const size_t P_halves = by.P / 2, R_halves = by.R / 2;
    std::vector<int32_t> row_owner((size_t)E, 0);
    for (int32_t l = 0; l < n_layers; ++l) {
      const int32_t n = lptr[l + 1] - lptr[l];
      const int64_t items = half_items(n, B), grid = half_grid(n, B);
      CHECK(grid * kLayPassWaves >= items, "the grid covers the items");
      for (int64_t item = 0; item < items; ++item) {
        const int32_t tile = (int32_t)(item % ntiles2), slot = pp.layer_slot[l] + (int32_t)(item / ntiles2);
        if (slot < 0 || slot >= n_c) {
          CHECK(false, "item -> slot of the code");
          continue;
        }
        CHECK(2 * (int64_t)tile + 1 < mask_words, "the tile's two mask words exist");
        const int32_t e0 = pp.rec[(size_t)2 * slot], d = pp.rec[(size_t)2 * slot + 1];
        CHECK(d >= kLayMinD && d <= kLayBpMaxD, "record degree has a body");
        const size_t tcol = (size_t)tile * kLayHalfTile, last = 2 * 63 + 1;   // lane 63's dword: halves 126, 127
        for (int32_t k = 0; k < d; ++k) {
          CHECK((int64_t)e0 + k < E, "edge within the CSR");
          if ((int64_t)e0 + k >= E) continue;
          CHECK((size_t)(e0 + k) * (size_t)ldb + tcol + last < R_halves, "R row within the scratch");
          CHECK((size_t)cols[(size_t)e0 + k] * (size_t)ldb + tcol + last < P_halves, "P row within the scratch");
          CHECK((((size_t)(e0 + k) * (size_t)ldb + tcol) & 1u) == 0, "row dwords are aligned");
          if (tile == 0) ++row_owner[(size_t)e0 + k];
        }
      }
    }
    for (int64_t e = 0; e < E; ++e) CHECK(row_owner[(size_t)e] == 1, "every R row written by one item per iteration");
    // the pack: lane = variable, 64 halves (128 bytes, 16-byte aligned) of a tile of 64
    for (int32_t tile = 0; tile < ntiles; ++tile) {
      const size_t at = (size_t)(n_v - 1) * (size_t)ldb + (size_t)tile * kLayTile;
      CHECK(at + kLayTile <= P_halves && (2 * at) % 16 == 0, "the pack's reads within P and aligned");
    }
  }
  std::string esc;
  for (char ch : err) esc += (ch == '"' || ch == '\\') ? '?' : ch;
  std::printf("{\"valid\": %d, \"error\": \"%s\", \"unsupported\": %d, \"n_e\": %lld, \"n_tasks\": %d, \"cw_bytes\": %zu, "
              "\"cw_per_group\": %d, \"ldb\": %lld, \"mask_words\": %lld, \"pad_words_all_ones\": %d, \"bytes_P\": %zu, "
              "\"bytes_R\": %zu, \"bytes_mask\": %zu, \"bytes_total\": %zu, \"failures\": %d}\n",
              rc, esc.c_str(), unsupported, (long long)E, pl.n_tasks, pl.cw_bytes, pl.cw_per_group, (long long)ldb,
              (long long)mask_words, pad_ones, by.P, by.R, by.mask, by.total, g_fail);
  return g_fail ? 1 : 0;
}
