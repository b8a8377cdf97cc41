// CPU-only checker of the composite final step's host side (ib_composite_degree, ib_composite_pass and
// ib_composite_image of informationbottleneckdecodingldpc_amd/csrc/plan.h), built by tests/test_cpu_ib_composite.py
// with -fsanitize=address,undefined -fno-sanitize-recover=all.
//
//   composite_image_check image <tables.bin>
// tables.bin: int32 T, CM, match, p, D, cn_len, mc_len, then cn[cn_len], mc[mc_len] (the reference-layout CN vector
// and check matching vector). Prints one JSON line {"img": [512 dwords]}: the composite image of check pass p for
// degree D, dword h of entry (t, m) at 256 h + 16 t + m.
//
//   composite_image_check plan <graph.bin> <cn_tables>
// graph.bin: int32 n_v, n_c, indptr[n_c + 1] (the checks' degrees are all the rule reads). Prints one JSON line
// {"cm", "degree", "table_lds", "counts": {"D": checks}}: the composite's degree for a check pass of cn_tables
// tables, 0 = none.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "plan.h"

using namespace ibl;

static bool read_i32(FILE* f, std::vector<int32_t>* v, size_t n) {
  v->resize(n);
  return n == 0 || std::fread(v->data(), 4, n, f) == n;
}

static int image(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return 2;
  std::vector<int32_t> hdr, cn, mc;
  if (!read_i32(f, &hdr, 7)) return 2;
  const int T = hdr[0], CM = hdr[1], match = hdr[2], p = hdr[3], D = hdr[4];
  if (T < 2 || T > 16 || D < 5 || D > CM || CM > 8 || p < 0 || hdr[5] < 0 || hdr[6] < 0) return 2;
  if (!read_i32(f, &cn, (size_t)hdr[5]) || !read_i32(f, &mc, (size_t)hdr[6])) return 2;
  std::fclose(f);
  // the vectors hold what pass p reads (ibl_ib_create checks the same before it builds an image)
  const int64_t need_cn = ib_cn_raw_index(T, T, CM, p, D - 3, T - 1, T - 1) + 1;
  const int64_t need_mc = match ? (int64_t)(p + 1) * T * CM : 0;
  if ((int64_t)cn.size() < need_cn || (int64_t)mc.size() < need_mc) return 2;
  for (int32_t x : cn)
    if (x < 0 || x >= T) return 2;
  for (int32_t x : mc)
    if (x < 0 || x >= T) return 2;
  std::vector<uint32_t> img(512);
  ib_composite_pass(cn.data(), mc.data(), match != 0, T, CM, p, D, img.data());
  std::printf("{\"img\": [");
  for (size_t i = 0; i < img.size(); ++i) std::printf("%s%u", i ? ", " : "", img[i]);
  std::printf("]}\n");
  return 0;
}

static int plan(const char* path, int cn_tables) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return 2;
  std::vector<int32_t> hdr, indptr;
  if (!read_i32(f, &hdr, 2) || hdr[0] <= 0 || hdr[1] <= 0) return 2;
  if (!read_i32(f, &indptr, (size_t)hdr[1] + 1)) return 2;
  std::fclose(f);
  std::vector<int32_t> deg((size_t)hdr[1]);
  int cm = 0;
  std::map<int32_t, long> counts;
  for (int32_t c = 0; c < hdr[1]; ++c) {
    deg[c] = indptr[c + 1] - indptr[c];
    cm = std::max(cm, (int)deg[c]);
    ++counts[deg[c]];
  }
  std::printf("{\"cm\": %d, \"degree\": %d, \"table_lds\": %zu, \"counts\": {", cm,
              ib_composite_degree(deg, cm, cn_tables), ib_table_lds(cn_tables));
  const char* sep = "";
  for (const auto& kv : counts) {
    std::printf("%s\"%d\": %ld", sep, kv.first, kv.second);
    sep = ", ";
  }
  std::printf("}}\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "image")) return image(argv[2]);
  if (argc == 4 && !std::strcmp(argv[1], "plan")) return plan(argv[2], std::atoi(argv[3]));
  std::fprintf(stderr, "usage: composite_image_check image tables.bin | plan graph.bin cn_tables\n");
  return 2;
}
