// CPU-only checker of the fixed-point layered decoder's host geometry (fix_tiles / fix_ldb / fix_mask_words /
// fix_items / fix_grid / fix_bytes / fix_params_ok / fix_state_word of
// informationbottleneckdecodingldpc_amd/csrc/layered_plan.h), built by tests/test_cpu_layered_fixed.py with
// -fsanitize=address,undefined -fno-sanitize-recover=all.
//
//   layered_fixed_plan_check <graph.bin> <max_batch>
// graph.bin: the format of layered_plan_check.cpp. Walks every item of every launch of a batch of max_batch the way
// the layfix_* kernels index (byte and word offsets against the scratch sizes, the 16-byte accesses' alignment) and
// prints one JSON line {valid, error, n_layers, ntiles, ntiles4, ldb, mask_words, layer_grids, bytes_P, bytes_state,
// bytes_mask, bytes_bits, bytes_total, failures}; exit status 0 = the layers were judged and, when valid, every
// invariant held.
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
    std::fprintf(stderr, "usage: layered_fixed_plan_check graph.bin max_batch\n");
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

  // parameter ranges and the state word, whatever the graph
  CHECK(fix_params_ok(0, 0, 1) && fix_params_ok(16, 63, 63) && fix_params_ok(13, 0, 31), "parameters in range");
  CHECK(!fix_params_ok(-1, 0, 31) && !fix_params_ok(17, 0, 31) && !fix_params_ok(13, -1, 31) &&
            !fix_params_ok(13, 64, 31) && !fix_params_ok(13, 0, 0) && !fix_params_ok(13, 0, 64), "parameters out of range");
  for (uint32_t m1 : {0u, 1u, 63u})
    for (uint32_t m2 : {0u, 31u, 63u})
      for (uint32_t pos : {0u, 7u, 15u})
        for (uint32_t sg : {0u, 0x5555u, 0xffffu}) {
          const uint32_t w = fix_state_word(m1, m2, pos, sg);
          CHECK(((w >> 20) & 63u) == m1 && (w >> 26) == m2 && ((w >> 16) & 15u) == pos && (w & 0xffffu) == sg,
                "state word fields do not overlap");
        }
  CHECK(kLayMaxD <= 16 && kLayFixQMax == 63 && kLayFixTile == 4 * kLayTile, "field widths hold the ranges");

  std::string err;
  const int rc = validate_layers(n_v, n_c, indptr.data(), cols.data(), n_layers, lptr.data(), lchk.data(), &err);
  LayeredPassPlan pl;
  LayeredFixBytes by;
  int32_t ntiles = 0, ntiles4 = 0;
  int64_t ldb = 0, mask_words = 0;
  std::string grids;
  if (rc == 0) {
    plan_layered_passes(n_c, indptr.data(), n_layers, lptr.data(), lchk.data(), &pl);
    by = fix_bytes(n_v, n_c, B);
    ntiles = pass_tiles(B);
    ntiles4 = fix_tiles(B);
    ldb = fix_ldb(B);
    mask_words = fix_mask_words(B);
    CHECK(ntiles4 >= 1 && (int64_t)(ntiles4 - 1) * kLayFixTile < B && B <= (int64_t)ntiles4 * kLayFixTile,
          "tiles of 256 cover the batch");
    CHECK(ldb == (int64_t)ntiles4 * kLayFixTile && ldb % 16 == 0, "row stride");
    CHECK(mask_words == (int64_t)ntiles4 * kLayFixCw && mask_words >= ntiles, "mask words cover the tiles of 64");
    CHECK(by.P == (size_t)n_v * (size_t)ldb && by.state == (size_t)4 * n_c * (size_t)ldb, "row array bytes");
    CHECK(by.mask == (size_t)8 * mask_words && by.counter == 4, "mask and counter bytes");
    CHECK(by.bits == (size_t)8 * n_v * ntiles, "packed hard-decision bytes");
    CHECK(by.total == by.P + by.state + 2 * by.mask + by.counter + by.bits, "total bytes");
    // the mask words layfix_stage_in writes: running codewords clear, padding set, nothing past the arrays
    int64_t running = 0;
    for (int32_t tile = 0; tile < ntiles4; ++tile)
      for (int32_t lane = 0; lane < kLayFixCw; ++lane) {
        const int64_t t64 = (int64_t)kLayFixCw * tile + lane;
        CHECK(t64 < mask_words, "mask word within the arrays");
        const int64_t left = (int64_t)B - t64 * kLayTile;
        const uint64_t m = left >= kLayTile ? 0ull : left <= 0 ? ~0ull : ~0ull << left;
        for (int b = 0; b < kLayTile; ++b) {
          const bool pad = t64 * kLayTile + b >= B;
          CHECK((((m >> b) & 1ull) != 0) == pad, "padding codewords are finished from the start");
          running += pad ? 0 : 1;
        }
      }
    CHECK(running == B, "every codeword of the batch starts running");
    // every wave of every layer's launch, as layfix_layer indexes
    const size_t S_words = by.state / 4;
    for (int32_t l = 0; l < n_layers; ++l) {
      const int32_t n = lptr[l + 1] - lptr[l];
      const int64_t items = fix_items(n, B), grid = fix_grid(n, B);
      CHECK(items == (int64_t)n * ntiles4, "layer items");
      CHECK(grid * kLayPassWaves >= items && grid * kLayPassWaves < items + kLayPassWaves,
            "layer grid is the least that covers the items");
      grids += (l ? ", " : "") + std::to_string(grid);
      for (int64_t item = 0; item < items; ++item) {
        const int32_t tile = (int32_t)(item % ntiles4), slot = pl.layer_slot[l] + (int32_t)(item / ntiles4);
        CHECK(slot >= lptr[l] && slot < lptr[l + 1], "item -> slot of the layer");
        if (slot < 0 || slot >= n_c) continue;
        const int32_t e0 = pl.rec[(size_t)2 * slot], d = pl.rec[(size_t)2 * slot + 1];
        for (int lane : {0, 63}) {
          const size_t col = (size_t)tile * kLayFixTile + (size_t)kLayFixCw * lane;
          const size_t srow = (size_t)slot * (size_t)ldb + col;
          CHECK(srow % 4 == 0 && srow + 3 < S_words, "a lane's four state words: aligned, within the scratch");
          for (int32_t k = 0; k < d; ++k) {
            const size_t at = (size_t)cols[(size_t)e0 + k] * (size_t)ldb + col;
            CHECK(at % 4 == 0 && at + 3 < by.P, "a lane's dword of a P row: aligned, within the scratch");
          }
        }
      }
    }
    // layfix_pack: lane = variable, 64 bytes of its row per tile of 64, one word of the bits table
    for (int32_t tile = 0; tile < ntiles; ++tile)
      for (int32_t v : {0, n_v - 1}) {
        const size_t at = (size_t)v * (size_t)ldb + (size_t)tile * kLayTile;
        CHECK(at % 16 == 0 && at + kLayTile - 1 < by.P, "a variable's 64 bytes: aligned, within the scratch");
        CHECK((size_t)tile * (size_t)n_v + (size_t)v < by.bits / 8, "packed word within the table");
      }
  }
  std::string esc;
  for (char ch : err) esc += (ch == '"' || ch == '\\') ? '?' : ch;
  std::printf("{\"valid\": %d, \"error\": \"%s\", \"n_layers\": %d, \"ntiles\": %d, \"ntiles4\": %d, \"ldb\": %lld, "
              "\"mask_words\": %lld, \"layer_grids\": [%s], \"bytes_P\": %zu, \"bytes_state\": %zu, \"bytes_mask\": %zu, "
              "\"bytes_bits\": %zu, \"bytes_total\": %zu, \"failures\": %d}\n",
              rc, esc.c_str(), n_layers, ntiles, ntiles4, (long long)ldb, (long long)mask_words, grids.c_str(), by.P,
              by.state, by.mask, by.bits, by.total, g_fail);
  return g_fail ? 1 : 0;
}
