// CPU-only checker of the host side of the variable chains' composite final step (ib_vn_slots,
// ib_vn_composite_degree and ib_vn_composite_pass of informationbottleneckdecodingldpc_amd/csrc/plan.h), built by
// tests/test_cpu_ib_vn_composite.py with -fsanitize=address,undefined -fno-sanitize-recover=all.
//
//   vn_composite_image_check image <tables.bin>
// tables.bin: int32 T, VM, match, k, D, vn_len, mv_len, then vn[vn_len], mv[mv_len] (the reference-layout VN vector
// and variable matching vector). Prints one JSON line {"img": [512 dwords]}: the composite image of variable pass k
// for degree D, dword h of entry (t, m) at 256 h + 16 t + m.
//
//   vn_composite_image_check plan <degrees.bin> <match>
// degrees.bin: int32 n, vm, deg[n]: the degrees of the variables a pass walks and the code's largest variable degree.
// Prints one JSON line {"degree", "tables", "nraw", "table_lds", "deg": [..], "fslot": [kMaxD + 1 slots]}: the table
// slots of that pass's image and the composite's degree for it, 0 = none.
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
  std::vector<int32_t> hdr, vn, mv;
  if (!read_i32(f, &hdr, 7)) return 2;
  const int T = hdr[0], VM = hdr[1], match = hdr[2], k = hdr[3], D = hdr[4];
  if (T < 2 || T > 16 || D < 5 || D > VM || VM > 8 || k < 0 || hdr[5] < 0 || hdr[6] < 0) return 2;
  if (!read_i32(f, &vn, (size_t)hdr[5]) || !read_i32(f, &mv, (size_t)hdr[6])) return 2;
  std::fclose(f);
  // the vectors hold what pass k reads (ibl_ib_create checks the same before it builds an image)
  const int64_t need_vn = ib_vn_raw_index(T, T, VM, k, D - 2, T - 1, T - 1) + 1;
  const int64_t need_mv = match ? (int64_t)(k + 1) * T * VM : 0;
  if ((int64_t)vn.size() < need_vn || (int64_t)mv.size() < need_mv) return 2;
  for (int32_t x : vn)
    if (x < 0 || x >= T) return 2;
  for (int32_t x : mv)
    if (x < 0 || x >= T) return 2;
  std::vector<uint32_t> img(512);
  ib_vn_composite_pass(vn.data(), mv.data(), match != 0, T, T, VM, k, D, img.data());
  std::printf("{\"img\": [");
  for (size_t i = 0; i < img.size(); ++i) std::printf("%s%u", i ? ", " : "", img[i]);
  std::printf("]}\n");
  return 0;
}

static int plan(const char* path, int match) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return 2;
  std::vector<int32_t> hdr, deg;
  if (!read_i32(f, &hdr, 2) || hdr[0] <= 0 || hdr[1] <= 0) return 2;
  if (!read_i32(f, &deg, (size_t)hdr[0])) return 2;
  std::fclose(f);
  for (int32_t d : deg)
    if (d < 1 || d > hdr[1]) return 2;
  const IbVnSlots sl = ib_vn_slots(deg, match != 0);
  const int nt = std::max(sl.nt, 1);
  std::printf("{\"degree\": %d, \"tables\": %d, \"nraw\": %d, \"table_lds\": %zu, \"deg\": [",
              ib_vn_composite_degree(deg, hdr[1], nt), sl.nt, sl.nraw, ib_table_lds(nt));
  for (size_t i = 0; i < sl.deg.size(); ++i) std::printf("%s%d", i ? ", " : "", sl.deg[i]);
  std::printf("], \"fslot\": [");
  for (int d = 0; d <= kMaxD; ++d) std::printf("%s%d", d ? ", " : "", sl.fslot[d]);
  std::printf("]}\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "image")) return image(argv[2]);
  if (argc == 4 && !std::strcmp(argv[1], "plan")) return plan(argv[2], std::atoi(argv[3]));
  std::fprintf(stderr, "usage: vn_composite_image_check image tables.bin | plan degrees.bin match\n");
  return 2;
}
