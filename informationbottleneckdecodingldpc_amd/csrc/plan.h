// Host-side planning of the decoders and the encoder: pure C++17, no HIP.
//
// Everything the C ABI derives on the host before a launch lives here — the edge index arrays
// (map_node_connections), the fast path's work orders and small-batch tasks, the float and IB paths' degree-2
// fold plans (the IB one under tests/asan/fold_plan_check.cpp), the fused kernels' task tables and the encoder's substitution / factorisation plan — so the
// same code is built twice: into libibldpc.so (the capi_*.hip units include this header) and, with AddressSanitizer
// and UndefinedBehaviorSanitizer, into the CPU-only checker tests/asan/plan_check.cpp
// (tests/test_cpu_host.py::test_host_planning_under_sanitizers).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

namespace ibl {

constexpr int kMaxD = 16;         // largest node degree with an unrolled fast-path body
constexpr int kLightD = 4;        // nodes up to this degree run with a 4-row item buffer
constexpr int kFoldRec = 8;       // ints per check of the float fold plan (FlArgs::fold)

// The host copy of a code graph (ibl_graph derives from it): CSR of H with its CSC-side arrays.
struct HostGraph {
  int32_t n_v = 0, n_c = 0;
  int64_t n_e = 0;
  std::vector<int32_t> h_cn_deg, h_vn_deg;
  std::vector<int32_t> h_cn_start, h_cols, h_vn_start, h_tgt_vn;
};

// Tanner-graph index construction (discrete_LDPC_decoder_irreg.py:121-170): canonical CSR in, the
// reference's start / degree / target arrays out. Returns false with *err set on malformed input.
inline bool map_node_connections(int32_t n_v, int32_t n_c, const int32_t* indptr, const int32_t* cols,
                                 int32_t* cn_start, int32_t* cn_deg, int32_t* tgt_cn, int32_t* vn_start,
                                 int32_t* vn_deg, int32_t* tgt_vn, std::string* err) {
  if (n_v <= 0 || n_c <= 0 || !indptr || !cols) return *err = "empty graph", false;
  if (indptr[0] != 0) return *err = "csr_indptr[0] must be 0", false;
  std::vector<int32_t> vdeg(n_v, 0);
  for (int32_t c = 0; c < n_c; ++c) {
    if (indptr[c + 1] < indptr[c]) return *err = "csr_indptr not monotone", false;
    for (int32_t e = indptr[c]; e < indptr[c + 1]; ++e) {
      if (cols[e] < 0 || cols[e] >= n_v) return *err = "column index out of range", false;
      if (e > indptr[c] && cols[e] <= cols[e - 1])
        return *err = "column indices must be strictly ascending within a row (canonical CSR)", false;
      vdeg[cols[e]]++;
    }
    cn_start[c] = indptr[c];
    cn_deg[c] = indptr[c + 1] - indptr[c];
  }
  int64_t acc = 0;
  for (int32_t v = 0; v < n_v; ++v) {
    vn_start[v] = (int32_t)acc;
    vn_deg[v] = vdeg[v];
    acc += vdeg[v];
  }
  // walking checks in ascending order fills each variable's edges in ascending row order
  std::vector<int64_t> fill(vn_start, vn_start + n_v);
  for (int32_t c = 0; c < n_c; ++c)
    for (int32_t e = indptr[c]; e < indptr[c + 1]; ++e) {
      const int64_t p = fill[cols[e]]++;
      tgt_cn[e] = (int32_t)p;
      tgt_vn[p] = e;
    }
  return true;
}

// Fast-path work order of one side: {node, first own-order edge, degree, 0} per position, heaviest first
// (stable); *heavy = positions of degree > kLightD.
inline std::vector<int32_t> work_order(const std::vector<int32_t>& start, const std::vector<int32_t>& deg,
                                       int32_t* heavy) {
  const int32_t n = (int32_t)deg.size();
  std::vector<int32_t> idx(n);
  for (int32_t i = 0; i < n; ++i) idx[i] = i;
  std::stable_sort(idx.begin(), idx.end(), [&](int32_t x, int32_t y) { return deg[x] > deg[y]; });
  std::vector<int32_t> info(idx.size() * 4);
  *heavy = 0;
  for (size_t p = 0; p < idx.size(); ++p) {
    const int32_t v = idx[p];
    info[4 * p] = v;
    info[4 * p + 1] = start[v];
    info[4 * p + 2] = deg[v];
    info[4 * p + 3] = 0;
    if (deg[v] > kLightD) ++*heavy;
  }
  return info;
}

// {first position, count, degree, contiguous}: runs of at most 64 positions of one degree in a work order;
// contiguous = st0 + 1 when the run's nodes are consecutive and their own-order edges follow each other
// (node p0 + k at edge st0 + k·d), else 0 (the IB small-batch kernels then skip the per-lane record load)
inline std::vector<int32_t> order_tasks(const std::vector<int32_t>& info) {
  std::vector<int32_t> t;
  const int32_t n = (int32_t)(info.size() / 4);
  for (int32_t p = 0; p < n;) {
    const int32_t d = info[4 * p + 2];
    int32_t c = 0;
    while (p + c < n && c < 64 && info[4 * (p + c) + 2] == d) ++c;
    bool contig = true;
    for (int32_t k = 1; k < c && contig; ++k)
      contig = info[4 * (p + k)] == info[4 * p] + k && info[4 * (p + k) + 1] == info[4 * p + 1] + k * d;
    t.insert(t.end(), {p, c, d, contig ? info[4 * p + 1] + 1 : 0});
    p += c;
  }
  return t;
}

// Degree-2 variable fold (FlArgs::fold, fl_cn_item): a degree-2 variable v on checks c1, c2 is folded when
// both checks have one of their two fold slots free (variables taken in ascending order); each check's record
// names v's edge position in the check, the check-order row of v's other edge and v. Returns the folded
// variables' count; `rec` gets n_c records, `rest` the variables the variable pass still updates.
inline int32_t plan_fold(const HostGraph& g, std::vector<int32_t>* rec, std::vector<int32_t>* rest) {
  const int32_t nc = g.n_c, nv = g.n_v;
  rec->assign((size_t)nc * kFoldRec, 0);
  std::vector<int32_t> used(nc, 0);
  for (int32_t c = 0; c < nc; ++c) (*rec)[(size_t)kFoldRec * c] = (*rec)[(size_t)kFoldRec * c + 1] = -1;
  // check of each check-order edge
  std::vector<int32_t> chk_of(g.h_cols.size());
  for (int32_t c = 0; c < nc; ++c)
    for (int32_t k = 0; k < g.h_cn_deg[c]; ++k) chk_of[(size_t)g.h_cn_start[c] + k] = c;
  std::vector<char> folded(nv, 0);
  int32_t n = 0;
  for (int32_t v = 0; v < nv; ++v) {
    if (g.h_vn_deg[v] != 2) continue;
    const int32_t e1 = g.h_tgt_vn[(size_t)g.h_vn_start[v]], e2 = g.h_tgt_vn[(size_t)g.h_vn_start[v] + 1];
    const int32_t c1 = chk_of[(size_t)e1], c2 = chk_of[(size_t)e2];
    if (used[c1] >= 2 || used[c2] >= 2) continue;
    auto put = [&](int32_t c, int32_t e, int32_t other) {
      int32_t* r = &(*rec)[(size_t)kFoldRec * c];
      const int k = used[c]++;
      r[k] = e - g.h_cn_start[c];
      r[2 + k] = other;
      r[4 + k] = v;
    };
    put(c1, e1, e2);
    put(c2, e2, e1);
    folded[v] = 1;
    ++n;
  }
  rest->clear();
  for (int32_t v = 0; v < nv; ++v)
    if (!folded[v]) rest->push_back(v);
  return n;
}

// Degree-2 variable fold of the IB fast path (ib_cn_fast<8, ., true>, IbFastArgs::fold). The check bodies are
// straight-line code per degree, so the fold sits at fixed positions: a degree-2 variable is folded only when
// in BOTH of its checks its edge is one of the last two inputs (CSR order) of a check of degree >= 3 — a
// position holds one variable, so "both or neither" needs no further pruning. Per check kIbFoldRec ints
// {class, var0, var1, dst0, dst1, 0, 0, 0}: class bit 0 / 1 = the input at position D-2 / D-1 is folded (not
// necessarily a suffix: DVB-S2's last check holds a degree-2 variable next to the degree-1 one), var = that
// input's variable (its channel row), dst = the check-order row of the variable's other edge (-1: not folded).
// Returns the folded count; `rest` gets the variables the variable pass still updates.
constexpr int kIbFoldRec = 8;
inline int32_t plan_ib_fold(const HostGraph& g, std::vector<int32_t>* rec, std::vector<int32_t>* rest) {
  const int32_t nc = g.n_c, nv = g.n_v;
  rec->assign((size_t)nc * kIbFoldRec, 0);
  std::vector<int32_t> chk_of(g.h_cols.size());
  for (int32_t c = 0; c < nc; ++c) {
    int32_t* r = &(*rec)[(size_t)kIbFoldRec * c];
    const int32_t d = g.h_cn_deg[c], st = g.h_cn_start[c];
    for (int32_t k = 0; k < d; ++k) chk_of[(size_t)st + k] = c;
    for (int a = 0; a < 2; ++a) {
      r[1 + a] = d >= 2 ? g.h_cols[(size_t)st + d - 2 + a] : 0;
      r[3 + a] = -1;
    }
  }
  auto tail_pos = [&](int32_t e) {   // 0 / 1: edge e is input D-2 / D-1 of a check of degree >= 3; else -1
    const int32_t c = chk_of[(size_t)e], d = g.h_cn_deg[c], k = e - g.h_cn_start[c];
    return d >= 3 && k >= d - 2 ? k - (d - 2) : -1;
  };
  rest->clear();
  int32_t n = 0;
  for (int32_t v = 0; v < nv; ++v) {
    int32_t a1 = -1, a2 = -1, e1 = 0, e2 = 0;
    if (g.h_vn_deg[v] == 2) {
      e1 = g.h_tgt_vn[(size_t)g.h_vn_start[v]];
      e2 = g.h_tgt_vn[(size_t)g.h_vn_start[v] + 1];
      a1 = tail_pos(e1);
      a2 = tail_pos(e2);
    }
    if (a1 < 0 || a2 < 0) {
      rest->push_back(v);
      continue;
    }
    int32_t* r1 = &(*rec)[(size_t)kIbFoldRec * chk_of[(size_t)e1]];
    int32_t* r2 = &(*rec)[(size_t)kIbFoldRec * chk_of[(size_t)e2]];
    r1[0] |= 1 << a1;
    r1[3 + a1] = e2;
    r2[0] |= 1 << a2;
    r2[3 + a2] = e1;
    ++n;
  }
  return n;
}

// Work order of a node subset (the variables the fold leaves to the variable pass) or with a secondary key (the
// checks' fold class, so a wave item's class is uniform and equal classes run together): heaviest first, then
// ascending key, stable; field 3 of a position = its key.
inline std::vector<int32_t> work_order_keyed(const std::vector<int32_t>& nodes, const std::vector<int32_t>& start,
                                             const std::vector<int32_t>& deg, const std::vector<int32_t>* key,
                                             int32_t* heavy) {
  std::vector<int32_t> idx(nodes);
  auto kof = [&](int32_t x) { return key ? (*key)[(size_t)x] : 0; };
  std::stable_sort(idx.begin(), idx.end(), [&](int32_t x, int32_t y) {
    return deg[x] != deg[y] ? deg[x] > deg[y] : kof(x) < kof(y);
  });
  std::vector<int32_t> info(idx.size() * 4);
  *heavy = 0;
  for (size_t p = 0; p < idx.size(); ++p) {
    const int32_t v = idx[p];
    info[4 * p] = v;
    info[4 * p + 1] = start[v];
    info[4 * p + 2] = deg[v];
    info[4 * p + 3] = kof(v);
    if (deg[v] > kLightD) ++*heavy;
  }
  return info;
}

// Composite final step of the IB check chains (ib_cn_fast, the bodies cn_group_fold_ct<.., CP = true>; under
// tests/asan/composite_image_check.cpp). For one check degree D* >= 5 the last two steps of outputs 0 .. D*-3,
// "... -> L(., x_{D-2}) -> F(., x_{D-1})" with L = chain table D*-4 and F = the degree's final table (matching
// composed), are one table C(t, m)[y] = F(L(t, m), y): 16 nibbles = two dwords per entry (t, m), nibble y & 7 of
// dword y >> 3. In the LDS it is one more super-region of the quad layout (common.h): the dword of half h of
// entry (t, m) replicated over the 32 banks at (t << 12) | (m << 8) | (h << 7) | 4 (lane & 31), so the last two
// ds_read_u8 of a chain become one ds_read_b32 and a v_bfe_u32. The tables are decoder constants: composed once
// at create.
constexpr size_t kIbCompBytes = 65536;   // one super-region: 256 entries x 2 halves x 128 B
constexpr size_t kIbLdsBytes = 160 * 1024;   // a CU's LDS (common.h kLdsBytes)
// LDS bytes of a pass's nt tables: quads of 4, super-regions of 2 quads (common.h lds_of_quads(regions_of(nt)))
constexpr size_t ib_table_lds(int nt) { return (size_t)((((nt + 3) >> 2) + 1) >> 1) * 65536; }
// D*: the check degree >= 5 with the most checks (ties: the larger), if the per-pass kernels are the degree <= 8
// ones (cm = the largest check degree) and the composite's super-region fits the LDS behind the check pass's
// cn_tables tables (raw, matching-composed finals, the fold's) and before the two work counters; else 0.
inline int32_t ib_composite_degree(const std::vector<int32_t>& cn_deg, int cm, int cn_tables) {
  if (cm > 8 || ib_table_lds(cn_tables) + kIbCompBytes + 64 > kIbLdsBytes) return 0;
  int64_t cnt[9] = {0};
  for (int32_t d : cn_deg)
    if (d >= 5 && d <= 8) ++cnt[d];
  int32_t best = 0;
  for (int32_t d = 5; d <= 8; ++d)
    if (cnt[d] > 0 && (best == 0 || cnt[d] >= cnt[best])) best = d;
  return best;
}
// img[256 h + 16 t + m] = dword h of C(t, m): two quads' worth of raw dwords, staged like a table image.
// L and F: 256 entries each, (t, m) at 16 t + m (an alphabet below 16 is padded with zeros).
inline void ib_composite_image(const uint8_t* L, const uint8_t* F, uint32_t* img) {
  for (int e = 0; e < 256; ++e)
    for (int h = 0; h < 2; ++h) {
      uint32_t w = 0;
      for (int y = 0; y < 8; ++y) w |= (uint32_t)(F[16 * (L[e] & 15) + 8 * h + y] & 15) << (4 * y);
      img[256 * h + e] = w;
    }
}

// Entry (t, m) of chain table l of check pass p in the reference-layout CN vector (pass 0: the first table is
// Tc x Tc, the others Tc x T; later passes: CM - 2 tables of T x T each).
inline int64_t ib_cn_raw_index(int Tc, int T, int CM, int p, int l, int t, int m) {
  const int64_t T2 = (int64_t)T * T;
  if (p == 0) return l == 0 ? (int64_t)t * Tc + m : (int64_t)Tc * Tc + (int64_t)(l - 1) * Tc * T + (int64_t)t * T + m;
  return (int64_t)Tc * Tc + (int64_t)(CM - 3) * Tc * T + (int64_t)(p - 1) * (CM - 2) * T2 + l * T2 + (int64_t)t * T + m;
}
// The composite image of check pass p for degree D (5 <= D <= CM) from the reference-layout vectors, the fast
// path's alphabets (Tc = T <= 16): L = chain table D - 4, F = chain table D - 3 with the matching row of degree D
// composed into it when matching is on - the tables the pass image holds at slots D - 4 and cn_fslot[D].
inline void ib_composite_pass(const int32_t* cn, const int32_t* mc, bool match, int T, int CM, int p, int D,
                              uint32_t* img) {
  uint8_t L[256] = {0}, F[256] = {0};
  const int64_t mrow = (int64_t)p * T * CM + (int64_t)(D - 1) * T;
  for (int t = 0; t < T; ++t)
    for (int m = 0; m < T; ++m) {
      const int32_t r = cn[ib_cn_raw_index(T, T, CM, p, D - 3, t, m)];
      L[16 * t + m] = (uint8_t)cn[ib_cn_raw_index(T, T, CM, p, D - 4, t, m)];
      F[16 * t + m] = (uint8_t)(match ? mc[mrow + r] : r);
    }
  ib_composite_image(L, F, img);
}

// Composite final step of the IB variable chains (ib_vn_fast<8>, the bodies vn_group_cp; under
// tests/asan/vn_composite_image_check.cpp). The chains of outputs 0 .. D-3 of a degree-D variable end in "... ->
// V_{D-3}(., x_{D-2}) -> final_D(., x_{D-1})", the check chains' shape, so for one variable degree D* in 5..8 the
// same composite table (layout, image and LDS place of ib_composite_image) takes those two steps as one.
//
// Table slots of a variable pass image for the variables a pass walks (`deg`: their degrees): the raw tables up to
// the largest degree walked and, with matching, one composed final table per walked degree >= 2, in ascending
// order behind them (without matching a degree's final table is raw table d - 2). The full image (every variable)
// and the rest image of a folding decoder (the variables the fold leaves to the variable pass) are both planned
// by this rule; the images differ where the fold takes every variable of a degree.
struct IbVnSlots {
  std::vector<int> deg;                  // the degrees walked, ascending
  int nraw = 0, nt = 0;                  // raw tables; all tables
  int32_t fslot[kMaxD + 1] = {0};        // per degree <= kMaxD: slot of its final table
};
inline IbVnSlots ib_vn_slots(const std::vector<int32_t>& deg, bool match) {
  IbVnSlots sl;
  sl.deg.assign(deg.begin(), deg.end());
  std::sort(sl.deg.begin(), sl.deg.end());
  sl.deg.erase(std::unique(sl.deg.begin(), sl.deg.end()), sl.deg.end());
  const int dmax = sl.deg.empty() ? 0 : sl.deg.back();
  sl.nt = sl.nraw = match ? std::max(dmax - 2, 0) : std::max(dmax - 1, 0);
  for (int d : sl.deg) {
    if (d < 2) continue;
    const int fs = match ? sl.nt++ : d - 2;
    if (d <= kMaxD) sl.fslot[d] = fs;
  }
  return sl;
}
// D*: the variable degree in 5..8 with the most nodes among the walked ones (ties: the larger), if the per-pass
// kernel is the degree <= 8 one (vm = the code's largest variable degree) and the composite's super-region fits the
// LDS behind the pass's vn_tables tables (ib_vn_slots(..).nt) and before the two work counters; else 0.
inline int32_t ib_vn_composite_degree(const std::vector<int32_t>& deg, int vm, int vn_tables) {
  return ib_composite_degree(deg, vm, vn_tables);   // the check side's rule on the walked variables' degrees
}
// Entry (t, m) of raw table l of variable pass k in the reference-layout VN vector (per pass: V_0 of Tc x T, then
// VM - 1 tables of T x T).
inline int64_t ib_vn_raw_index(int Tc, int T, int VM, int k, int l, int t, int m) {
  const int64_t T2 = (int64_t)T * T, off = (int64_t)k * ((int64_t)Tc * T + (int64_t)(VM - 1) * T2);
  return off + (l == 0 ? (int64_t)t * T + m : (int64_t)Tc * T + (int64_t)(l - 1) * T2 + (int64_t)t * T + m);
}
// The composite image of variable pass k for degree D (5 <= D <= VM), the fast path's alphabets (Tc = T <= 16):
// L = raw table D - 3, F = raw table D - 2 with the matching row of degree D composed into it when matching is on -
// the table the pass image holds at slot fslot[D].
inline void ib_vn_composite_pass(const int32_t* vn, const int32_t* mv, bool match, int Tc, int T, int VM, int k, int D,
                                 uint32_t* img) {
  uint8_t L[256] = {0}, F[256] = {0};
  const int64_t mrow = (int64_t)k * T * VM + (int64_t)(D - 1) * T;
  for (int t = 0; t < T; ++t)
    for (int m = 0; m < T; ++m) {
      const int32_t r = vn[ib_vn_raw_index(Tc, T, VM, k, D - 2, t, m)];
      L[16 * t + m] = (uint8_t)vn[ib_vn_raw_index(Tc, T, VM, k, D - 3, t, m)];
      F[16 * t + m] = (uint8_t)(match ? mv[mrow + r] : r);
    }
  ib_composite_image(L, F, img);
}

// Task tables of the fused kernels (FlFusedArgs, IbFusedArgs).
struct FusedTasks {
  std::vector<int32_t> cn_task, vn_task, vn_node, vn_slot;
};

// Check nodes sorted by degree (heaviest first, stable) and cut into tasks of up to 64 nodes of one
// degree; edge k of lane i of a check task gets slot first + k*count + i. Variable nodes likewise;
// vn_slot maps each variable edge (task-major, k*count + i) to the slot of the same edge. bank_order
// reorders the variables of each degree for conflict-free dword slot reads, scanning `vwin` candidates per
// lane (below).
inline void build_fused_tasks(const HostGraph& g, FusedTasks* ft, bool bank_order, size_t vwin) {
  const int64_t E = g.n_e;
  vwin = std::max<size_t>(1, vwin);
  const std::vector<int32_t>& tgt_vn = g.h_tgt_vn;
  auto starts = [](const std::vector<int32_t>& deg) {
    std::vector<int64_t> st(deg.size() + 1, 0);
    for (size_t i = 0; i < deg.size(); ++i) st[i + 1] = st[i] + deg[i];
    return st;
  };
  auto sorted = [](const std::vector<int32_t>& deg) {
    std::vector<int32_t> idx(deg.size());
    for (size_t i = 0; i < idx.size(); ++i) idx[i] = (int32_t)i;
    std::stable_sort(idx.begin(), idx.end(), [&](int32_t x, int32_t y) { return deg[x] > deg[y]; });
    return idx;
  };
  const std::vector<int64_t> cst = starts(g.h_cn_deg), vst = starts(g.h_vn_deg);
  std::vector<int32_t> slot_of((size_t)E);
  {
    const std::vector<int32_t> ord = sorted(g.h_cn_deg);
    int32_t slot = 0;
    for (size_t i = 0; i < ord.size();) {
      const int32_t d = g.h_cn_deg[ord[i]];
      int32_t cnt = 0;
      while (i + cnt < ord.size() && cnt < 64 && g.h_cn_deg[ord[i + cnt]] == d) ++cnt;
      ft->cn_task.insert(ft->cn_task.end(), {slot, cnt, d, 0});
      for (int32_t l = 0; l < cnt; ++l)
        for (int32_t k = 0; k < d; ++k) slot_of[(size_t)cst[ord[i + l]] + k] = slot + k * cnt + l;
      slot += cnt * d;
      i += cnt;
    }
  }
  {
    std::vector<int32_t> ord = sorted(g.h_vn_deg);
    // Variable order within each degree: the variable pass reads its edge slots in check-task order,
    // so lanes of one 32-lane group (one LDS cycle of a ds_read_b32) collide when their k-th slots share
    // a bank (slot mod 32). Greedily fill each 32-lane group with variables whose k-th slots hit banks
    // not yet used by the group at that k (scan window vwin): the fused IB kernel's dword slots then read
    // (almost) conflict-free. Any order gives the same results.
    for (size_t i0 = 0; bank_order && i0 < ord.size();) {
      const int32_t d = g.h_vn_deg[ord[i0]];
      size_t i1 = i0;
      while (i1 < ord.size() && g.h_vn_deg[ord[i1]] == d) ++i1;
      std::vector<int32_t> pool(ord.begin() + (long)i0, ord.begin() + (long)i1), res;
      res.reserve(pool.size());
      auto bank = [&](int32_t v, int k) { return (uint32_t)slot_of[(size_t)tgt_vn[(size_t)vst[v] + k]] & 31u; };
      while (!pool.empty()) {
        uint32_t used[kMaxD + 1] = {0};
        for (int lane = 0; lane < 32 && !pool.empty(); ++lane) {
          size_t best = 0;
          int bestc = 1 << 30;
          const size_t win = std::min<size_t>(pool.size(), vwin);
          for (size_t c = 0; c < win && bestc > 0; ++c) {
            int col = 0;
            for (int k = 0; k < d && k <= kMaxD; ++k) col += (used[k] >> bank(pool[c], k)) & 1u;
            if (col < bestc) { bestc = col; best = c; }
          }
          const int32_t v = pool[best];
          for (int k = 0; k < d && k <= kMaxD; ++k) used[k] |= 1u << bank(v, k);
          res.push_back(v);
          pool.erase(pool.begin() + (long)best);
        }
      }
      std::copy(res.begin(), res.end(), ord.begin() + (long)i0);
      i0 = i1;
    }
    int32_t sidx = 0;
    for (size_t i = 0; i < ord.size();) {
      const int32_t d = g.h_vn_deg[ord[i]];
      int32_t cnt = 0;
      while (i + cnt < ord.size() && cnt < 64 && g.h_vn_deg[ord[i + cnt]] == d) ++cnt;
      ft->vn_task.insert(ft->vn_task.end(), {(int32_t)i, cnt, d, sidx});
      ft->vn_slot.resize((size_t)sidx + (size_t)cnt * d);
      for (int32_t l = 0; l < cnt; ++l) {
        const int32_t v = ord[i + l];
        ft->vn_node.push_back(v);
        for (int32_t k = 0; k < d; ++k) ft->vn_slot[(size_t)sidx + k * cnt + l] = slot_of[(size_t)tgt_vn[(size_t)vst[v] + k]];
      }
      sidx += cnt * d;
      i += cnt;
    }
  }
}

// The fused float kernel keeps the variable-edge slot indices in LDS as u16, each variable task's rows at the
// full stride of 64 lanes (record field 3 = the task's first padded index): the D index loads of a task share
// one address and take their row offsets as immediates, whatever the task's node count.
inline void pad_vn_slots(FusedTasks* ft) {
  std::vector<int32_t> pslot;
  for (size_t t = 0; t < ft->vn_task.size() / 4; ++t) {
    const int32_t cnt = ft->vn_task[4 * t + 1], d = ft->vn_task[4 * t + 2], sf = ft->vn_task[4 * t + 3];
    ft->vn_task[4 * t + 3] = (int32_t)pslot.size();
    for (int32_t k = 0; k < d; ++k)
      for (int32_t i = 0; i < 64; ++i) pslot.push_back(i < cnt ? ft->vn_slot[sf + (size_t)k * cnt + i] : 0);
  }
  ft->vn_slot.swap(pslot);
}

// ------------------------------------------------------------------ encoder plan
struct Csr {
  std::vector<int32_t> ip{0}, ix;
  void push_row(const std::vector<int32_t>& cols) {
    ix.insert(ix.end(), cols.begin(), cols.end());
    ip.push_back((int32_t)ix.size());
  }
};

// 1 lower / -1 upper triangular with full diagonal, 0 otherwise (LDPC_encoder.py:342-360);
// rows given as sorted column lists of the square parity part
inline int tri_shape(const std::vector<std::vector<int32_t>>& rows) {
  const int n = (int)rows.size();
  int64_t nnz = 0, low = 0;
  for (int i = 0; i < n; ++i) {
    bool diag = false;
    for (int c : rows[i]) {
      ++nnz;
      if (c <= i) ++low;
      if (c == i) diag = true;
    }
    if (!diag) return 0;
  }
  if (low == nnz) return 1;
  if (low == n) return -1;
  return 0;
}

// The plan getLDPCEncoderParamters (LDPC_encoder.py:197-269) derives from H = [A | B]: B triangular with a
// full diagonal (possibly after reversing its rows) -> forward / backward substitution over P = B's strict
// part; else GF(2) factorisation with gf2factorize's first-candidate pivot rule (:287-340) -> L, the pivot
// row order and P = strict upper part of U[piv]. chain = P is bidiagonal in substitution order (the prefix-
// XOR scan kernel).
struct EncPlan {
  std::string algo;
  int method = 0, dir = 1, chain = 0;   // method 1 = factorisation (L substitution first)
  Csr A, L, P;
  std::vector<int32_t> order;           // row order applied before P (empty: identity)
};

// Returns 0, -1 (malformed H), -2 (the parity part is singular in GF(2)) or -3 (too large to factorise); *err
// says which.
inline int encoder_plan(int32_t N, int32_t M, const int32_t* indptr, const int32_t* cols, EncPlan* pl,
                        std::string* err) {
  const int32_t K = N - M;
  std::vector<std::vector<int32_t>> brows(M);
  for (int32_t r = 0; r < M; ++r) {
    std::vector<int32_t> ac;
    for (int32_t e = indptr[r]; e < indptr[r + 1]; ++e) {
      const int32_t c = cols[e];
      if (c < 0 || c >= N) return *err = "column index out of range", -1;
      if (c < K) ac.push_back(c); else brows[r].push_back(c - K);
    }
    pl->A.push_row(ac);
  }
  auto strict = [&](const std::vector<std::vector<int32_t>>& rows, int dir) {
    Csr T;
    for (int i = 0; i < (int)rows.size(); ++i) {
      std::vector<int32_t> c;
      for (int j : rows[i])
        if (dir > 0 ? j < i : j > i) c.push_back(j);
      T.push_row(c);
    }
    return T;
  };
  int shape = tri_shape(brows);
  if (shape != 0) {                                    // (LDPC_encoder.py:208-213)
    pl->algo = shape == 1 ? "Forward Substitution" : "Backward Substitution";
    pl->dir = shape;
    pl->P = strict(brows, shape);
  } else {
    std::vector<std::vector<int32_t>> rev(brows.rbegin(), brows.rend());
    const int rshape = tri_shape(rev);
    if (rshape != 0) {                                 // rows reversed (:214-226)
      pl->algo = rshape == 1 ? "Forward Substitution" : "Backward Substitution";
      pl->dir = rshape;
      for (int i = 0; i < M; ++i) pl->order.push_back(M - 1 - i);
      pl->P = strict(rev, rshape);
    } else {                                           // GF(2) factorisation (:227-246, gf2factorize :287-340)
      if (M > 16384) return *err = "GF(2) factorisation limited to 16384 parity bits", -3;
      pl->algo = "Matrix Inverse";
      pl->method = 1;
      const int words = (M + 63) / 64;
      std::vector<uint64_t> Y2((size_t)M * words, 0), Y1((size_t)M * words, 0);
      for (int i = 0; i < M; ++i) {
        for (int c : brows[i]) Y2[(size_t)i * words + (c >> 6)] |= 1ull << (c & 63);
        Y1[(size_t)i * words + (i >> 6)] |= 1ull << (i & 63);
      }
      std::vector<char> used(M, 0);
      std::vector<int32_t> piv(M, 0);
      for (int col = 0; col < M; ++col) {
        const uint64_t bit = 1ull << (col & 63);
        int pv = -1;
        for (int i = 0; i < M; ++i)
          if (!used[i] && (Y2[(size_t)i * words + (col >> 6)] & bit)) {
            if (pv < 0) { pv = i; continue; }
            for (int w = 0; w < words; ++w) Y2[(size_t)i * words + w] ^= Y2[(size_t)pv * words + w];
            Y1[(size_t)i * words + (pv >> 6)] |= 1ull << (pv & 63);
          }
        if (pv < 0) return *err = "the last N-K columns of H are singular in GF(2)", -2;
        used[pv] = 1;
        piv[col] = pv;
      }
      auto row_cols = [&](const std::vector<uint64_t>& Y, int i) {
        std::vector<int32_t> c;
        for (int w = 0; w < words; ++w)
          for (uint64_t v = Y[(size_t)i * words + w]; v; v &= v - 1) c.push_back(w * 64 + __builtin_ctzll(v));
        return c;
      };
      std::vector<std::vector<int32_t>> l(M), u(M);
      for (int i = 0; i < M; ++i) {
        l[i] = row_cols(Y1, i);
        u[i] = row_cols(Y2, piv[i]);
      }
      pl->L = strict(l, 1);
      pl->P = strict(u, -1);
      pl->dir = -1;
      pl->order = piv;
    }
  }
  // bidiagonal P in substitution order -> prefix-XOR scan
  bool chain = true;
  for (int i = 0; i < M && chain; ++i) {
    const int n = pl->P.ip[i + 1] - pl->P.ip[i];
    const int want = pl->dir > 0 ? i - 1 : i + 1;
    if (want < 0 || want >= M) chain = n == 0;
    else chain = n == 1 && pl->P.ix[pl->P.ip[i]] == want;
  }
  pl->chain = chain ? 1 : 0;
  return 0;
}

}  // namespace ibl
