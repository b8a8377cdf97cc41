// C ABI (include/ibldpc.h): the information-bottleneck decoder (ib_kernels.hip): table-image construction at
// create, and one decode schedule per path (fused on-chip, small batch, fast per-pass, generic).
//
// Schedules restate the reference's host loop without its per-iteration host sync:
//   decode_OpenCL (Discrete_LDPC_decoding/discrete_LDPC_decoder_irreg.py:245-341)
// Early stop: each check-node pass ORs "some check unsatisfied" into 64 flag words of its
// iteration; the launches of the next iteration read those words and exit at once when they
// are all zero, and a one-wave kernel turns the flags into the iteration index the output
// pass uses.  The host only enqueues.
#include <cstring>
#include <functional>

#include "host.h"

using namespace ibl;

struct ibl_ib {
  const ibl_graph* g = nullptr;
  int32_t Tc = 0, T = 0, imax = 0, CM = 0, VM = 0, match = 0, max_batch = 0, ldb = 0;
  bool fast = false;
  DevBuf<uint8_t> cin, vin, ch8;
  DevBuf<int32_t> flags, dL;
  // fast path
  DevBuf<uint32_t> cn_img, vn_img, dec_img;
  int cn_nt = 0, vn_nt = 0, dec_nt = 0;   // fast path: LDS table quads (4 tables each) per pass
  int32_t cn_fslot[kMaxD + 1] = {0}, vn_fslot[kMaxD + 1] = {0};
  KCfg kcn, kvn, kdec;
  KTimer timer;
  // degree-2 variable fold of the per-pass path (plan.h plan_ib_fold; ib_cn_fast<8, ., FOLD>): the host plan
  // (per-check records, class-sorted check work order, work order of the variables left to the variable pass),
  // uploaded with the second check inbox once a batch reaches the folding kernels (ib_fold_alloc); fold_slot =
  // LDS slot of the transposed degree-2 variable table in every check pass's image
  int32_t n_folded = 0, fold_slot = -1, n_rest = 0, rest_heavy = 0;
  bool fold_on = true;
  std::vector<int32_t> fold_rec, fold_cn_info, fold_vn_info;
  DevBuf<uint8_t> cin2;
  DevBuf<int32_t> fold, cn_info_f, vn_info_r;
  // composite final step of the check chains (plan.h ib_composite_degree / ib_composite_image): the check degree
  // that has one (0: none planned), its per-pass images (imax x 512 dwords, beside cn_img) and the switch of
  // ibl_ib_set_composite; a launch with the composite takes kIbCompBytes more LDS than kcn.lds
  int32_t comp_deg = 0;
  bool comp_on = true;
  DevBuf<uint32_t> cn_comp;
  // composite final step of the variable chains (plan.h ib_vn_composite_degree / ib_vn_composite_pass), per work
  // order of the variable pass: [0] every variable (fold off, or nothing folded), [1] the variables the fold leaves
  // (the rest list). Per view the variable degree that has one (0: none), its per-pass images ((imax - 1) x 512
  // dwords) and the LDS bytes of a launch with it. The rest view runs from an image of its own, the tables of the
  // degrees it walks alone (plan.h ib_vn_slots; DVB-S2 with matching: 8 tables, not 9), with its own final slots.
  int32_t vcomp_deg[2] = {0, 0};
  bool vcomp_on = true;
  DevBuf<uint32_t> vn_comp[2], vn_img_r;
  size_t vcomp_lds[2] = {0, 0};
  int vn_nt_r = 0;
  int32_t vn_fslot_r[kMaxD + 1] = {0};
  // fused on-chip path (IbFusedArgs, short codes): task tables, LDS bytes per workgroup, grid
  int32_t path = IBL_PATH_AUTO;
  bool fused_ok = false, f_half_ok = false;   // f_half_ok: the 4-codeword-group kernel is usable too
  bool f_each_ok = false;                     // the per-codeword-stop forms of the group sizes in use are usable
  int32_t f_ncw_forced = 0;                   // IBL_FUSED_NCW read once at create (A/B, tests), 0 = auto
  // small-batch per-pass kernels (ib_*_small) for B <= small_b (0: off); LDS bytes per launch kind
  int32_t small_b = 0;
  bool s_ok = false;                          // the small-batch kernels exist for this decoder and run without scratch
  size_t s_lds_cn = 0, s_lds_vn = 0, s_lds_dec = 0;
  ChainGraphs s_graphs;                       // small-batch pass chains (IBL_SMALL_GRAPH=0 at create: launch them)
  FusedTaskBufs ft;
  int32_t f_nreg = 0, f_dbuf = 0, f_cn_uni = 0, f_vn_uni = 0;
  size_t f_lds = 0;
  int f_grid = 0, f_block = 0;
  // generic path
  DevBuf<int32_t> cn_lut, vn_lut, mc, mv;
  int64_t cn_len = 0, vn_len = 0, mc_len = 0, mv_len = 0;
};

// ------------------------------------------------------------------ create: tables to device images
namespace {

using Table = std::vector<uint8_t>;  // 256 entries, (t, m) at t*16 + m

struct IbLuts {   // ibl_ib_create's table vectors in the reference layout
  const int32_t *cn, *vn, *mc, *mv;
  int64_t cn_len, vn_len, mc_len, mv_len;
};
struct IbSlots {   // one pass's LDS table slots (ib_plan_slots)
  std::vector<int> cdeg, vdeg;            // the degrees present
  int cn_nraw = 0, vn_nraw = 0;           // raw (reference) tables of a check / variable pass
  int cn_nt = 0, vn_nt = 0;               // all tables of a pass: raw, matching-composed finals, the fold's
  IbVnSlots vr;                           // the variable pass over the fold's rest list (planned with its composite)
};
struct IbImages {
  std::vector<uint32_t> cn_img, vn_img, dec_img, cn_comp, vn_comp[2], vn_img_r;
};

Table make_table(int T, const std::function<int(int, int)>& f) {
  Table tb(256, 0);
  for (int t = 0; t < T; ++t)
    for (int m = 0; m < T; ++m) tb[t * kTP + m] = (uint8_t)f(t, m);
  return tb;
}

// One pass's tables as quads (common.h): nreg x 256 dwords, dword (t*16+m) of quad R holds entry (t, m)
// of table 4R+j in byte j (slot_off); the kernels replicate each dword over the 32 banks. Unused slots
// of the last quad are 0.
void append_pass(std::vector<uint32_t>& img, const std::vector<Table>& tbs, int nreg) {
  for (int R = 0; R < nreg; ++R)
    for (int r = 0; r < 256; ++r) {
      uint32_t w = 0;
      for (int j = 0; j < 4; ++j) {
        const size_t k = (size_t)4 * R + j;
        if (k < tbs.size()) w |= (uint32_t)tbs[k][r] << (8 * j);
      }
      img.push_back(w);
    }
}

std::vector<int> present(const std::vector<int32_t>& deg) {
  std::vector<int> d(deg.begin(), deg.end());
  std::sort(d.begin(), d.end());
  d.erase(std::unique(d.begin(), d.end()), d.end());
  return d;
}

// LDS bytes of a fast CN / VN launch: table quads, the 2 work counters
size_t fast_lds(int nt) { return lds_of_quads(regions_of(nt)) + 64; }

// extra: LDS bytes of the launch beyond the tables' (the check pass's composite super-region)
int pick_cfg(int which, int maxd, int nt, int num_cus, KCfg* k, size_t extra = 0) {
  k->lds = fast_lds(nt) + extra;
  int best_waves = 0;
  // largest block first at equal occupancy: a CU's waves then share one work counter
  for (int block : {1024, 768, 640, 512, 384, 256}) {
    int bpc = 0;
    if (ib_fast_occupancy(which, maxd, block, k->lds, &bpc) != hipSuccess) continue;
    const int waves = bpc * block / 64;
    if (bpc > 0 && waves > best_waves) {
      best_waves = waves;
      k->block = block;
      k->grid = bpc * num_cus;
    }
  }
  return best_waves > 0 ? IBL_OK : fail(IBL_EHIP, "no occupancy for IB kernel (LDS too large?)");
}

int ib_validate(const ibl_graph* g, int32_t Tc, int32_t T, int32_t imax, const IbLuts& lu, int32_t match,
                int32_t max_batch) {
  if (Tc < 2 || T < 2 || Tc > 256 || T > 256) return fail(IBL_EUNSUPPORTED, "cardinalities must lie in [2, 256]");
  if (imax < 1) return fail(IBL_EINVAL, "imax must be >= 1");
  if (max_batch < 1) return fail(IBL_EINVAL, "max_batch must be >= 1");
  const int CM = g->dcm, VM = g->dvm;
  if (CM < 3) return fail(IBL_EUNSUPPORTED, "IB decoding needs a check-node degree >= 3");
  const int64_t need_cn = (int64_t)Tc * Tc + (int64_t)(CM - 3) * Tc * T + (int64_t)(imax - 1) * (CM - 2) * T * T;
  const int64_t need_vn = (int64_t)imax * ((int64_t)Tc * T + (int64_t)(VM - 1) * T * T);
  if (!lu.cn || lu.cn_len < need_cn) return fail(IBL_EINVAL, "CN LUT vector shorter than the reference layout");
  if (!lu.vn || lu.vn_len < need_vn) return fail(IBL_EINVAL, "VN LUT vector shorter than the reference layout");
  auto in_T = [T](const int32_t* p, int64_t n) { return std::all_of(p, p + n, [T](int32_t x) { return x >= 0 && x < T; }); };
  if (!in_T(lu.cn, lu.cn_len)) return fail(IBL_EINVAL, "CN LUT entries must lie in [0, T_dec)");
  if (!in_T(lu.vn, lu.vn_len)) return fail(IBL_EINVAL, "VN LUT entries must lie in [0, T_dec)");
  if (match) {
    if (!lu.mc || lu.mc_len < (int64_t)imax * CM * T || !lu.mv || lu.mv_len < (int64_t)imax * VM * T)
      return fail(IBL_EINVAL, "matching vectors shorter than (imax, d_max, T_dec)");
    if (!in_T(lu.mc, lu.mc_len) || !in_T(lu.mv, lu.mv_len))
      return fail(IBL_EINVAL, "matching entries must lie in [0, T_dec)");
  }
  return IBL_OK;
}

// Table slots of the pass images (each degree's final one: cn_fslot / vn_fslot), whether
// the code takes the fast path (h->fast), and the degree-2 variable fold's plan with its slot.
IbSlots ib_plan_slots(ibl_ib* h, int32_t flags) {
  const ibl_graph* g = h->g;
  const int CM = h->CM, VM = h->VM;
  IbSlots sl;
  sl.cdeg = present(g->h_cn_deg);
  sl.vdeg = present(g->h_vn_deg);
  const bool deg_ok = CM <= kMaxD && VM <= kMaxD;
  sl.cn_nt = sl.cn_nraw = h->match ? CM - 3 : CM - 2;
  sl.vn_nt = sl.vn_nraw = h->match ? std::max(VM - 2, 0) : VM - 1;
  if (h->match) {
    sl.cn_nt += (int)sl.cdeg.size();
    for (int d : sl.vdeg) sl.vn_nt += (d >= 2);
  }
  const int max_nt = (kLdsBytes / kSuper) * 8;   // whole super-regions of 2 quads: 16 tables
  int slot = sl.cn_nraw;
  for (int d : sl.cdeg) {
    const int fs = h->match ? slot++ : (d >= 3 ? d - 3 : 0);
    if (deg_ok) h->cn_fslot[d] = fs;
  }
  slot = sl.vn_nraw;
  for (int d : sl.vdeg) {
    if (d < 2) continue;
    const int fs = h->match ? slot++ : d - 2;
    if (deg_ok) h->vn_fslot[d] = fs;
  }
  const bool lds_ok = fast_lds(sl.cn_nt) <= (size_t)kLdsBytes && fast_lds(std::max(sl.vn_nt, 1)) <= (size_t)kLdsBytes;
  h->fast = !(flags & IBL_FLAG_FORCE_GENERIC) && h->Tc == h->T && h->T <= kTP && deg_ok && sl.cn_nt <= max_nt &&
            sl.vn_nt <= max_nt && VM <= max_nt && sl.cn_nt > 0 && lds_ok;
  if (h->fast && CM <= 8) {
    // Degree-2 variable fold: planned when the folding kernels exist for this code (the degree <= 8 bodies) and
    // the transposed degree-2 variable table fits the check pass's LDS — a free slot of its quads (DVB-S2: 6 of
    // 8 used), or one more quad if the LDS has room for it.
    std::vector<int32_t> rec, rest;
    const int32_t n = plan_ib_fold(*g, &rec, &rest);
    if (n > 0 && sl.cn_nt + 1 <= max_nt && fast_lds(sl.cn_nt + 1) <= (size_t)kLdsBytes) {
      h->n_folded = n;
      h->fold_slot = sl.cn_nt++;
      std::vector<int32_t> cls((size_t)g->n_c), all((size_t)g->n_c);
      for (int32_t c = 0; c < g->n_c; ++c) {
        cls[c] = rec[(size_t)kIbFoldRec * c];
        all[c] = c;
      }
      int32_t heavy = 0;
      h->fold_cn_info = work_order_keyed(all, g->h_cn_start, g->h_cn_deg, &cls, &heavy);
      h->fold_vn_info = work_order_keyed(rest, g->h_vn_start, g->h_vn_deg, nullptr, &h->rest_heavy);
      h->n_rest = (int32_t)rest.size();
      h->fold_rec.swap(rec);
    }
  }
  if (h->fast) h->comp_deg = ib_composite_degree(g->h_cn_deg, CM, sl.cn_nt);
  if (h->fast) {   // the variable pass's composite, for either list it may walk
    h->vcomp_deg[0] = ib_vn_composite_degree(g->h_vn_deg, VM, std::max(sl.vn_nt, 1));
    if (h->n_folded > 0) {
      std::vector<int32_t> rdeg((size_t)h->n_rest);
      for (int32_t p = 0; p < h->n_rest; ++p) rdeg[(size_t)p] = h->fold_vn_info[4 * (size_t)p + 2];
      sl.vr = ib_vn_slots(rdeg, h->match != 0);
      h->vcomp_deg[1] = ib_vn_composite_degree(rdeg, VM, std::max(sl.vr.nt, 1));
      std::memcpy(h->vn_fslot_r, sl.vr.fslot, sizeof(h->vn_fslot_r));
    }
  }
  return sl;
}

// The fast path's images from the reference-layout vectors, tables in the slots ib_plan_slots numbered.
IbImages ib_build_images(ibl_ib* h, const IbLuts& lu, const IbSlots& sl) {
  const int Tc = h->Tc, T = h->T, imax = h->imax, CM = h->CM, VM = h->VM;
  IbImages im;
  // ---------------- CN images: pass p = 0 (iteration 0 ops) .. imax-1
  const int64_t T2 = (int64_t)T * T;
  auto cn_raw = [&](int p, int l, int t, int m) -> int { return lu.cn[ib_cn_raw_index(Tc, T, CM, p, l, t, m)]; };
  auto vn_raw = [&](int k, int l, int t, int m) -> int {
    const int64_t off = (int64_t)k * ((int64_t)Tc * T + (int64_t)(VM - 1) * T2);
    const int64_t idx = off + (l == 0 ? (int64_t)t * T + m : (int64_t)Tc * T + (int64_t)(l - 1) * T2 + (int64_t)t * T + m);
    return lu.vn[idx];
  };
  for (int p = 0; p < imax; ++p) {
    std::vector<Table> tbs;
    for (int l = 0; l < sl.cn_nraw; ++l) tbs.push_back(make_table(T, [&](int t, int m) { return cn_raw(p, l, t, m); }));
    if (h->match)   // each degree's final table composed with its matching row: slot cn_fslot[d]
      for (int d : sl.cdeg) {
        const int64_t mrow = (int64_t)p * T * CM + (int64_t)(d - 1) * T;
        if (d == 2) tbs.push_back(make_table(T, [&](int t, int) { return lu.mc[mrow + t]; }));
        else tbs.push_back(make_table(T, [&](int t, int m) { return lu.mc[mrow + cn_raw(p, d - 3, t, m)]; }));
      }
    if (h->fold_slot >= 0) {
      // the update of a degree-2 variable, transposed: row = the check's output, column = the channel value;
      // the table (matching composed) the variable pass after check pass p looks up as (channel, message)
      const int64_t mrow = (int64_t)p * T * VM + (int64_t)T;
      tbs.resize((size_t)h->fold_slot, Table(256, 0));
      tbs.push_back(make_table(T, [&](int t, int m) {
        const int r = vn_raw(p, 0, m, t);
        return h->match ? lu.mv[mrow + r] : r;
      }));
    }
    append_pass(im.cn_img, tbs, regions_of(sl.cn_nt));
    if (h->comp_deg) {   // chain table D* - 4 into D*'s final table (slots D* - 4 and cn_fslot[D*] of this image)
      im.cn_comp.resize((size_t)(p + 1) * 512);
      ib_composite_pass(lu.cn, lu.mc, h->match != 0, T, CM, p, h->comp_deg, &im.cn_comp[(size_t)p * 512]);
    }
  }
  h->cn_nt = regions_of(sl.cn_nt);
  // ---------------- VN images: pass k = 0 .. imax-2 (extrinsic), decision images k = 0 .. imax-1
  for (int k = 0; k < std::max(imax - 1, 1); ++k) {
    std::vector<Table> tbs;
    for (int l = 0; l < sl.vn_nraw; ++l) tbs.push_back(make_table(T, [&](int t, int m) { return vn_raw(k, l, t, m); }));
    for (int d : sl.vdeg) {   // likewise: slot vn_fslot[d]
      if (!h->match || d < 2) continue;
      const int64_t mrow = (int64_t)k * T * VM + (int64_t)(d - 1) * T;
      tbs.push_back(make_table(T, [&](int t, int m) { return lu.mv[mrow + vn_raw(k, d - 2, t, m)]; }));
    }
    append_pass(im.vn_img, tbs, regions_of(std::max(sl.vn_nt, 1)));
    for (int v = 0; v < 2; ++v)   // raw table D* - 3 into D*'s final table, per work order
      if (h->vcomp_deg[v]) {
        im.vn_comp[v].resize((size_t)(k + 1) * 512);
        ib_vn_composite_pass(lu.vn, lu.mv, h->match != 0, Tc, T, VM, k, h->vcomp_deg[v], &im.vn_comp[v][(size_t)k * 512]);
      }
    if (h->vcomp_deg[1]) {   // the rest list's own image: the tables of the degrees it walks, slots vn_fslot_r
      std::vector<Table> rt;
      for (int l = 0; l < sl.vr.nraw; ++l) rt.push_back(make_table(T, [&](int t, int m) { return vn_raw(k, l, t, m); }));
      for (int d : sl.vr.deg) {
        if (!h->match || d < 2) continue;
        const int64_t mrow = (int64_t)k * T * VM + (int64_t)(d - 1) * T;
        rt.push_back(make_table(T, [&](int t, int m) { return lu.mv[mrow + vn_raw(k, d - 2, t, m)]; }));
      }
      append_pass(im.vn_img_r, rt, regions_of(std::max(sl.vr.nt, 1)));
    }
  }
  h->vn_nt = regions_of(std::max(sl.vn_nt, 1));
  h->vn_nt_r = regions_of(std::max(sl.vr.nt, 1));
  for (int k = 0; k < imax; ++k) {
    std::vector<Table> tbs;
    for (int l = 0; l < VM; ++l) tbs.push_back(make_table(T, [&](int t, int m) { return vn_raw(k, l, t, m); }));
    append_pass(im.dec_img, tbs, regions_of(VM));
  }
  h->dec_nt = regions_of(VM);
  return im;
}

// Fused IB decoder eligibility (fast path, messages + the largest pass's table
// quads within the CU's LDS, check degree >= 2, an occupancy of >= 1 block without scratch) and
// task tables. Leaves fused_ok false when the code does not fit.
int ib_fused_setup(ibl_ib* h) {
  const ibl_graph* g = h->g;
  if (!h->fast || g->n_e == 0 || g->dc_min < 2) return IBL_OK;
  const int nreg = std::max(h->cn_nt, std::max(h->vn_nt, h->dec_nt));
  // one table set: tables, raw images, slots; two sets (see TablePrefetch; a single quad's two sets share
  // one super-region) where they fit beside the slots; IBL_FUSED_DBUF=0 turns them off (A/B)
  const size_t lds1 = lds_of_quads(nreg) + (size_t)nreg * 1024 + (size_t)g->n_e * 4 + 16;
  const size_t lds2 = lds_of_quads(2 * nreg) + (size_t)g->n_e * 4 + 16;
  const bool dbuf = nreg <= 2 && lds2 <= (size_t)kLdsBytes && env_on("IBL_FUSED_DBUF");   // set offset: ib_fused
  const size_t lds = dbuf ? lds2 : lds1;
  if (lds > (size_t)kLdsBytes) return IBL_OK;
  int bpc = 0, block = 0;
  size_t priv = 0;
  if (ib_fused_occupancy(h->CM, h->VM, 8, lds, &bpc, &block, &priv) != hipSuccess || bpc < 1 || priv != 0) {
    (void)hipGetLastError();
    return IBL_OK;
  }
  {   // the half-group instantiation (4 codewords per workgroup, small batches) under the same bounds
    int bpc4 = 0, block4 = 0;
    size_t priv4 = 0;
    h->f_half_ok = ib_fused_occupancy(h->CM, h->VM, 4, lds, &bpc4, &block4, &priv4) == hipSuccess && bpc4 == bpc &&
                   block4 == block && priv4 == 0;
    (void)hipGetLastError();
  }
  {   // the per-codeword-stop forms (ibl_ib_decode_each) of the group sizes in use, under the same bounds: same LDS
      // (their two mask words are the spare ones behind the ticket counters), no scratch, the same geometry
    int bpe = 0, blocke = 0;
    size_t prive = 0;
    h->f_each_ok = ib_fused_occupancy(h->CM, h->VM, 8, lds, &bpe, &blocke, &prive, true) == hipSuccess && bpe == bpc &&
                   blocke == block && prive == 0;
    if (h->f_each_ok && h->f_half_ok)
      h->f_each_ok = ib_fused_occupancy(h->CM, h->VM, 4, lds, &bpe, &blocke, &prive, true) == hipSuccess &&
                     bpe == bpc && blocke == block && prive == 0;
    (void)hipGetLastError();
  }
  FusedTasks ft;
  build_fused_tasks(*g, &ft, env_on("IBL_FUSED_VORDER"), fused_vwin());
  if (int rc = h->ft.upload(ft)) return rc;
  // single-degree sides: task records follow from the task index (IbFusedArgs::cn_uni / vn_uni);
  // IBL_FUSED_UNIFORM=0 keeps the loaded records (A/B)
  if (env_on("IBL_FUSED_UNIFORM")) {
    auto uniform = [](const std::vector<int32_t>& task, int32_t n, bool vn) {
      if (task.empty()) return 0;
      const int32_t d = task[2];
      for (size_t t = 0; t < task.size() / 4; ++t) {
        const int32_t p = (int32_t)(64 * t), cnt = std::min<int32_t>(64, n - p);
        const int32_t* r = &task[4 * t];
        if (r[1] != cnt || r[2] != d || (vn ? (r[0] != p || r[3] != p * d) : r[0] != p * d)) return 0;
      }
      return (int)d;
    };
    h->f_cn_uni = uniform(ft.cn_task, g->n_c, false);
    h->f_vn_uni = uniform(ft.vn_task, g->n_v, true);
  }
  if (const char* ne = getenv("IBL_FUSED_NCW")) h->f_ncw_forced = atoi(ne);
  h->f_nreg = nreg;
  h->f_dbuf = dbuf ? 1 : 0;
  h->f_lds = lds;
  h->f_block = block;
  h->f_grid = bpc * g->num_cus;
  h->fused_ok = true;
  return IBL_OK;
}

// The fast path's device state: images, launch configurations, the no-scratch check, the fused and the
// small-batch kernels' set-up.
int ib_configure_fast(ibl_ib* h, const IbImages& im) {
  const ibl_graph* g = h->g;
  const int CM = h->CM, VM = h->VM;
  int rc;
  if ((rc = h->cn_img.upload(im.cn_img)) || (rc = h->vn_img.upload(im.vn_img)) || (rc = h->dec_img.upload(im.dec_img)))
    return rc;
  if ((rc = pick_cfg(0, CM, 4 * h->cn_nt, g->num_cus, &h->kcn)) ||
      (rc = pick_cfg(1, VM, 4 * h->vn_nt, g->num_cus, &h->kvn)) ||
      (rc = pick_cfg(2, VM, 4 * h->dec_nt, g->num_cus, &h->kdec)))
    return rc;
  if (h->comp_deg) {   // kept only if the launch with the composite's LDS has the check pass's geometry
    KCfg kc;
    if (pick_cfg(0, CM, 4 * h->cn_nt, g->num_cus, &kc, kIbCompBytes) != IBL_OK || kc.block != h->kcn.block ||
        kc.grid != h->kcn.grid)
      h->comp_deg = 0;
    else if ((rc = h->cn_comp.upload(im.cn_comp)))
      return rc;
  }
  for (int v = 0; v < 2; ++v) {   // likewise the variable pass's, per work order
    if (!h->vcomp_deg[v]) continue;
    KCfg kc;
    if (pick_cfg(1, VM, 4 * (v ? h->vn_nt_r : h->vn_nt), g->num_cus, &kc, kIbCompBytes) != IBL_OK ||
        kc.block != h->kvn.block || kc.grid != h->kvn.grid) {
      h->vcomp_deg[v] = 0;
      continue;
    }
    h->vcomp_lds[v] = kc.lds;
    if ((rc = h->vn_comp[v].upload(im.vn_comp[v])) || (v == 1 && (rc = h->vn_img_r.upload(im.vn_img_r)))) return rc;
  }
  size_t priv = 0;
  const char* kname = "";
  HIPCHK(ib_fast_private_bytes(CM, VM, &priv, &kname));
#if IBL_DIAG
  const bool allow_scratch = getenv("IBL_ALLOW_SCRATCH") != nullptr;   // diagnostic builds: the spill experiment
#else
  const bool allow_scratch = false;
#endif
  if (!allow_scratch && (rc = refuse_private(priv, std::string("fast-path kernel ") + kname + " has a ",
                                             "-byte private segment (register spill / scratch item): rebuild required")))
    return rc;
  if ((rc = ib_fused_setup(h))) return rc;
  // small-batch per-pass kernels: the fast path's tables; used for B <= small_b (IBL_SMALL_B at create overrides
  // the default, 0 turns them off)
  HIPCHK(ib_small_private_bytes(CM, VM, &priv, &kname));
  h->s_ok = priv == 0;
  small_batch_env(h->s_ok, kSmallBatchDefault, &h->small_b, &h->s_graphs);
  h->s_lds_cn = lds_of_quads(h->cn_nt);
  h->s_lds_vn = lds_of_quads(h->vn_nt);
  h->s_lds_dec = lds_of_quads(h->dec_nt);
  return IBL_OK;
}

int ib_upload_generic(ibl_ib* h, const IbLuts& lu) {
  int rc;
  h->cn_len = lu.cn_len; h->vn_len = lu.vn_len;
  if ((rc = h->cn_lut.upload(lu.cn, lu.cn_len)) || (rc = h->vn_lut.upload(lu.vn, lu.vn_len))) return rc;
  if (h->match) {
    h->mc_len = lu.mc_len; h->mv_len = lu.mv_len;
    if ((rc = h->mc.upload(lu.mc, lu.mc_len)) || (rc = h->mv.upload(lu.mv, lu.mv_len))) return rc;
  }
  return IBL_OK;
}

bool ib_fused_in_use(const ibl_ib* h) { return h->fused_ok && h->path != IBL_PATH_PASSES; }

// Codewords per workgroup of the fused IB kernel for a batch of B: 4-codeword half groups when even the
// doubled number of workgroups fits the grid (each half group then has a workgroup slot of its own);
// whole 8-codeword groups otherwise — with 2*ngroups > grid some workgroups would run two half groups in
// a row, and a half group takes more than half a group's time (per-phase latency). The
// environment IBL_FUSED_NCW=8 / 4, read once when the decoder is created, forces either (A/B, tests); 4
// needs the half-group kernel (f_half_ok).
int ib_fused_ncw(const ibl_ib* h, int B) {
  const int ngroups = (B + 7) / 8;
  const int forced = h->f_ncw_forced;
  if (!h->f_half_ok || forced == 8) return 8;
  return (forced == 4 || 2 * ngroups <= h->f_grid) ? 4 : 8;
}

// The IB fold's device state, allocated by the first decode that reaches the folding kernels (a batch above the
// small-batch threshold on the per-pass path with the fold on): second check inbox, per-check records, the
// class-sorted check work order and the work order of the variables the variable pass still updates. cin2 is
// set last: cin2 set <=> the fold's state is complete.
int ib_fold_alloc(ibl_ib* h) {
  if (h->n_folded == 0 || h->cin2) return IBL_OK;
  DevBuf<uint8_t> c2;
  DevBuf<int32_t> fold, cf, vr;
  int rc;
  if ((rc = c2.alloc_zero((size_t)h->g->n_e * h->ldb)) || (rc = fold.upload(h->fold_rec)) ||
      (rc = cf.upload(h->fold_cn_info)) || (rc = vr.upload(h->fold_vn_info)))
    return rc;
  h->fold = std::move(fold);
  h->cn_info_f = std::move(cf);
  h->vn_info_r = std::move(vr);
  h->cin2 = std::move(c2);
  return IBL_OK;
}

// ------------------------------------------------------------------ decode: one function per path

// What the check / variable launches of the small-batch and the fast per-pass schedule share: rows of ldbb bytes
void ib_pass_args(const ibl_ib* h, int B, int ldbb, IbFastArgs* cn, IbFastArgs* vn) {
  const ibl_graph* g = h->g;
  cn->ch8 = vn->ch8 = h->ch8;
  cn->info = g->cn_info; cn->tgt = g->tgt_cn; cn->out = h->vin;
  vn->info = g->vn_info; vn->tgt = g->tgt_vn; vn->out = h->cin; vn->in = h->vin;
  cn->n_nodes = g->n_c; vn->n_nodes = g->n_v;
  cn->ldb = vn->ldb = ldbb;
  cn->B = vn->B = B;
  cn->half = vn->half = h->T / 2;
  cn->match = vn->match = h->match;
  cn->nt = h->cn_nt; vn->nt = h->vn_nt;
  std::memcpy(cn->fslot, h->cn_fslot, sizeof(cn->fslot));
  std::memcpy(vn->fslot, h->vn_fslot, sizeof(vn->fslot));
}

// The fused kernel's arguments for a batch of B, but for the stop (unsat / dL, or iters); *grid: workgroups
IbFusedArgs ib_fused_args(const ibl_ib* h, uint32_t* chT, int32_t B, void* d_out, int32_t out_dtype, int* grid) {
  const ibl_graph* g = h->g;
  IbFusedArgs f{};
  f.cn_img = h->cn_img; f.vn_img = h->vn_img; f.dec_img = h->dec_img; f.chT = chT;
  f.cn_task = h->ft.cn_task; f.vn_task = h->ft.vn_task; f.vn_node = h->ft.vn_node; f.vn_slot = h->ft.vn_slot;
  f.out = d_out;
  std::memcpy(f.cn_fslot, h->cn_fslot, sizeof(f.cn_fslot));
  std::memcpy(f.vn_fslot, h->vn_fslot, sizeof(f.vn_fslot));
  f.cn_nt = h->cn_nt; f.vn_nt = h->vn_nt; f.dec_nt = h->dec_nt; f.nreg = h->f_nreg; f.dbuf = h->f_dbuf;
  f.n_cn_nodes = g->n_c; f.cn_uni = h->f_cn_uni; f.vn_uni = h->f_vn_uni;
  f.n_e = (int32_t)g->n_e; f.n_v = g->n_v; f.n_cn_tasks = h->ft.n_cn; f.n_vn_tasks = h->ft.n_vn;
  f.B = B; f.imax = h->imax; f.half = h->T / 2; f.match = h->match; f.out_dtype = out_dtype;
  f.aligned = out_aligned(B, d_out, 4, out_dtype == kU8 ? 1 : 4);
  f.ngroups = (B + 7) / 8;
  f.ncw = ib_fused_ncw(h, B);
  *grid = std::min(h->f_grid, f.ngroups * (8 / f.ncw));
  return f;
}

// Per-codeword stop (ibldpc.h "Per-codeword stop"): the staging launch and one launch of ib_fused<.., ncw | kIbEach>; no flag
// words, no finalize_iters, no second pass.
int ib_each_fused(ibl_ib* h, const void* d_ch, int32_t ch_dtype, int32_t B, void* d_out, int32_t out_dtype,
                  int32_t* d_iters, hipStream_t s) {
  uint32_t* chT = reinterpret_cast<uint32_t*>(h->ch8.get());
  HIPCHK(launch_ib_stage_t(d_ch, ch_dtype, h->g->n_v, B, h->ft.vn_node, chT, s));
  int grid = 0;
  IbFusedArgs f = ib_fused_args(h, chT, B, d_out, out_dtype, &grid);
  f.iters = d_iters;
  HIPCHK(h->timer.timed(0, s, [&] { return launch_ib_fused(f, h->CM, h->VM, grid, h->f_block, h->f_lds, s, true); }));
  return IBL_OK;
}

int ib_decode_fused(ibl_ib* h, const void* d_ch, int32_t ch_dtype, int32_t B, void* d_out, int32_t out_dtype,
                    bool early, int32_t* d_iters, hipStream_t s) {
  const ibl_graph* g = h->g;
  const int I = h->imax;
  // channel as [group][N] dwords of 8 nibbles (the fused kernel's layout), in the staging buffer
  uint32_t* chT = reinterpret_cast<uint32_t*>(h->ch8.get());
  HIPCHK(launch_ib_stage_t(d_ch, ch_dtype, g->n_v, B, h->ft.vn_node, chT, s));
  int grid = 0;
  IbFusedArgs f = ib_fused_args(h, chT, B, d_out, out_dtype, &grid);
  f.unsat = flag_row(h->flags, early, 0); f.dL = nullptr;
  auto launch = [&] { return launch_ib_fused(f, h->CM, h->VM, grid, h->f_block, h->f_lds, s); };
#if IBL_DIAG
  // diagnostic builds only: IBL_TRACE_FUSED=<file> records block 0's clock at every phase boundary of its
  // first group (with -DIBL_FUSED_TRACE=1 kernels, tools/variants.py ftrace)
  const char* ftrace = getenv("IBL_TRACE_FUSED");
  TraceBuf tr;
  int rc;
  if (ftrace) {
    if ((rc = tr.open((size_t)3 * (2 * I + 4), s))) return rc;
    f.trace = tr.d;
  }
#endif
  HIPCHK(h->timer.timed(0, s, launch));
#if IBL_DIAG
  if (ftrace && (rc = tr.save(s, ftrace, 0, tr.n))) return rc;
  f.trace = nullptr;
#endif
  HIPCHK(launch_finalize(h->flags, I, early ? 1 : 0, h->dL, d_iters, s));
  if (early) {   // pass 2: re-run the batch to the stop iteration (a no-op when it is imax-1)
    f.unsat = nullptr;
    f.dL = h->dL;
    HIPCHK(h->timer.timed(0, s, launch));
  }
  return IBL_OK;
}

// small batch: (task, word) items, lane = node (ib_*_small); the pass schedule of the fast path.
// Rows are packed to the batch's words (4 * nwords bytes, not the per-pass path's ldb / 2): a pass
// then touches E * 4 * nwords bytes of each inbox (B = 2 on DVB-S2: 0.9 MB, resident in the L2s and
// the MALL) instead of one 128-B line per edge (29 MB)
int ib_decode_small(ibl_ib* h, const void* d_ch, int32_t ch_dtype, int32_t B, void* d_out, int32_t out_dtype,
                    bool early, int32_t* d_iters, hipStream_t s) {
  const ibl_graph* g = h->g;
  const int I = h->imax;
  const int nwords = (B + 7) / 8, ldbb = 4 * nwords;
  HIPCHK(launch_ib_stage4(d_ch, ch_dtype, g->n_v, B, h->ch8, ldbb, s));
  auto grid_of = [&](int ntask, size_t lds) {
    const int per_cu = std::max(1, (int)(kLdsBytes / std::max<size_t>(lds, 1)));
    const int wpb = small_block(nwords) / 64;
    const int need = (ntask * nwords + wpb - 1) / wpb;
    return std::max(1, std::min(need, per_cu * g->num_cus));
  };
  IbFastArgs cn{}, vn{};
  ib_pass_args(h, B, ldbb, &cn, &vn);
  cn.task = g->cn_task; cn.n_tasks = g->n_cn_task;
  vn.task = g->vn_task; vn.n_tasks = g->n_vn_task;
  cn.nwords = vn.nwords = nwords;
  const int gcn = grid_of(g->n_cn_task, h->s_lds_cn), gvn = grid_of(g->n_vn_task, h->s_lds_vn);
  // the pass chain (decoder buffers only): CN pass 0 from the staged channel, then {VN j, CN j}
  auto chain = [&](hipStream_t st) -> hipError_t {
    IbFastArgs c0 = cn, v = vn;
    c0.in = nullptr; c0.gather = g->csr_cols; c0.img = h->cn_img; c0.gate = nullptr; c0.unsat = nullptr;
    hipError_t e = h->timer.timed(0, st, [&] { return launch_ib_cn_small(c0, h->CM, gcn, h->s_lds_cn, st); });
    if (e != hipSuccess) return e;
    IbFastArgs c = c0;
    c.gather = nullptr;
    c.in = h->cin;
    for (int j = 1; j < I; ++j) {
      const int32_t* gate = flag_row(h->flags, early && j >= 2, j - 1);
      v.img = h->vn_img + (size_t)(j - 1) * h->vn_nt * 256;
      v.gate = gate;
      if ((e = h->timer.timed(1, st, [&] { return launch_ib_vn_small(v, h->VM, gvn, h->s_lds_vn, st); })) != hipSuccess)
        return e;
      c.img = h->cn_img + (size_t)j * h->cn_nt * 256;
      c.gate = gate;
      c.unsat = flag_row(h->flags, early, j);
      if ((e = h->timer.timed(0, st, [&] { return launch_ib_cn_small(c, h->CM, gcn, h->s_lds_cn, st); })) != hipSuccess)
        return e;
    }
    return hipSuccess;
  };
  // replayed from a captured graph, unless per-launch timing is on (bench roofline) or graphs are off
  if (h->s_graphs.on && !h->timer.on) HIPCHK(h->s_graphs.run(B, early ? 1 : 0, s, chain));
  else HIPCHK(chain(s));
  HIPCHK(launch_finalize(h->flags, I, early ? 1 : 0, h->dL, d_iters, s));
  IbDecArgs dc{};
  dc.vin = h->vin; dc.ch8 = h->ch8; dc.img = h->dec_img; dc.iters = h->dL; dc.out = d_out; dc.out_dtype = out_dtype;
  dc.nt = h->dec_nt; dc.n_nodes = g->n_v; dc.ldb = ldbb; dc.B = B;
  dc.info = g->vn_info; dc.task = g->vn_task; dc.n_tasks = g->n_vn_task; dc.nwords = nwords;
  dc.aligned = out_aligned(B, d_out, 4, out_dtype == kU8 ? 1 : 4);
  HIPCHK(launch_ib_dec_small(dc, grid_of(g->n_vn_task, h->s_lds_dec), h->s_lds_dec, s));
  return IBL_OK;
}

int ib_decode_fast(ibl_ib* h, const void* d_ch, int32_t ch_dtype, int32_t B, void* d_out, int32_t out_dtype,
                   bool early, int32_t* d_iters, hipStream_t s) {
  const ibl_graph* g = h->g;
  const int I = h->imax;
  const int ccn = ib_fast_chunk(h->CM), cvn = ib_fast_chunk(h->VM);
  const int ldbb = h->ldb / 2;
  HIPCHK(launch_ib_stage4(d_ch, ch_dtype, g->n_v, B, h->ch8, ldbb, s));
  IbFastArgs cn{}, vn{};
  ib_pass_args(h, B, ldbb, &cn, &vn);
  cn.n_heavy = g->cn_heavy; vn.n_heavy = g->vn_heavy;
  // Degree-2 variable fold: check pass j < I-1 applies the folded variables' update itself and writes the
  // result into the inbox check pass j+1 reads, cb[(j + 1) & 1]; variable pass j writes the rest there. The
  // last check pass folds nothing (the decision reads every variable-inbox row); with early stop any pass
  // from 1 on may be the last, so those also write the folded edges' variable-inbox rows (fold_mode 2).
  const bool fold = h->fold_on && h->n_folded > 0 && I > 1;
  int rc;
  if (fold) {
    if ((rc = ib_fold_alloc(h))) return rc;
    vn.info = h->vn_info_r; vn.n_nodes = h->n_rest; vn.n_heavy = h->rest_heavy;
    cn.fold = h->fold; cn.fold_slot = h->fold_slot;
  }
  uint8_t* cb[2] = {h->cin, fold ? h->cin2 : h->cin};
  auto cn_fold = [&](int j) {   // check pass j's work order and fold mode
    const bool f = fold && j < I - 1;
    cn.info = f ? h->cn_info_f.get() : g->cn_info.get();
    cn.fold_mode = f ? ((early && j >= 1) ? 2 : 1) : 0;
    cn.fout = f ? cb[(j + 1) & 1] : nullptr;
  };
#if IBL_DIAG
  // diagnostic builds only (timing, outputs are not decodes): IBL_VN_PART=heavy / light runs the variable
  // pass over one item class only (the degree > kLightD items, or the rest)
  if (const char* vp = getenv("IBL_VN_PART")) {
    if (vp[0] == 'h') {
      vn.n_nodes = g->vn_heavy;
    } else if (vp[0] == 'l') {
      vn.info = g->vn_info + 4 * (size_t)g->vn_heavy;
      vn.n_nodes = g->n_v - g->vn_heavy;
      vn.n_heavy = 0;
    }
  }
#endif
  cn.nchunks = (B + ccn - 1) / ccn;
  vn.nchunks = (B + cvn - 1) / cvn;
  // pass 0: send + checknode_update_iter0, inputs gathered from the staged channel rows
  cn.in = nullptr; cn.gather = g->csr_cols; cn.img = h->cn_img; cn.gate = nullptr; cn.unsat = nullptr;
  cn_fold(0);
  // composite final step: check pass j runs it from its own image
  const int comp = h->comp_on ? h->comp_deg : 0;
  const uint32_t* cimg = comp ? h->cn_comp.get() : nullptr;
  auto launch_cn = [&]() {
    return launch_ib_cn_fast(cn, h->CM, h->kcn.grid, h->kcn.block, h->kcn.lds + (comp ? kIbCompBytes : 0), s, cimg, comp);
  };
  HIPCHK(h->timer.timed(0, s, launch_cn));
  cn.gather = nullptr;
  // likewise the variable passes, by the list they walk; over the rest list from that list's own image and slots
  const int view = fold ? 1 : 0;
  const int vcomp = h->vcomp_on ? h->vcomp_deg[view] : 0;
  const bool rest_img = vcomp && view == 1;
  if (rest_img) {
    vn.nt = h->vn_nt_r;
    std::memcpy(vn.fslot, h->vn_fslot_r, sizeof(vn.fslot));
  }
  const uint32_t* vimg = rest_img ? h->vn_img_r.get() : h->vn_img.get();
  const size_t vlds = vcomp ? h->vcomp_lds[view] : h->kvn.lds;
  uint64_t* trace = nullptr;
  size_t nwv = 0;
#if IBL_DIAG
  // diagnostic builds only: IBL_TRACE_WAVES=<prefix> records {start, end, items|cu} of every wave of the
  // middle iteration's VN and CN launches into <prefix>_vn.bin / <prefix>_cn.bin (uint64 triples)
  const char* trace_path = getenv("IBL_TRACE_WAVES");
  TraceBuf tr;
  nwv = (size_t)h->kvn.grid * (h->kvn.block / 64);
  const size_t nwc = (size_t)h->kcn.grid * (h->kcn.block / 64);
  if (trace_path && I > 1) {
    if ((rc = tr.open(3 * (nwv + nwc), s))) return rc;
    trace = tr.d;
  }
#endif
  for (int j = 1; j < I; ++j) {
    const int32_t* gate = flag_row(h->flags, early && j >= 2, j - 1);
    vn.img = vimg + (size_t)(j - 1) * vn.nt * 256;
    const uint32_t* vcimg = vcomp ? h->vn_comp[view] + (size_t)(j - 1) * 512 : nullptr;
    vn.gate = gate;
    vn.trace = (trace && j == I / 2) ? trace : nullptr;
    vn.out = cb[j & 1];
    HIPCHK(h->timer.timed(1, s, [&] {
      return launch_ib_vn_fast(vn, h->VM, h->kvn.grid, h->kvn.block, vlds, s, vcimg, vcomp);
    }));
    cn.img = h->cn_img + (size_t)j * h->cn_nt * 256;
    if (comp) cimg = h->cn_comp + (size_t)j * 512;
    cn.gate = gate;
    cn.unsat = flag_row(h->flags, early, j);
    cn.trace = (trace && j == I / 2) ? trace + 3 * nwv : nullptr;
    cn.in = cb[j & 1];
    cn_fold(j);
    HIPCHK(h->timer.timed(0, s, launch_cn));
  }
#if IBL_DIAG
  if (trace && ((rc = tr.save(s, std::string(trace_path) + "_vn.bin", 0, 3 * nwv)) ||
                (rc = tr.save(s, std::string(trace_path) + "_cn.bin", 3 * nwv, 3 * nwc))))
    return rc;
#endif
  HIPCHK(launch_finalize(h->flags, I, early ? 1 : 0, h->dL, d_iters, s));
  IbDecArgs dc{};
  dc.vin = h->vin; dc.ch8 = h->ch8; dc.start = g->vn_start; dc.deg = g->vn_deg; dc.img = h->dec_img;
  dc.iters = h->dL; dc.out = d_out; dc.out_dtype = out_dtype; dc.nt = h->dec_nt; dc.n_nodes = g->n_v;
  dc.nchunks = (B + kChunkDec - 1) / kChunkDec; dc.ldb = ldbb; dc.B = B;
  dc.aligned = out_aligned(B, d_out, 4, out_dtype == kU8 ? 1 : 4);
  HIPCHK(launch_ib_dec_fast(dc, h->kdec.grid, h->kdec.block, h->kdec.lds, s));
  return IBL_OK;
}

int ib_decode_generic(ibl_ib* h, const void* d_ch, int32_t ch_dtype, int32_t B, void* d_out, int32_t out_dtype,
                      bool early, int32_t* d_iters, hipStream_t s) {
  const ibl_graph* g = h->g;
  const int I = h->imax;
  HIPCHK(launch_ib_stage(d_ch, ch_dtype, g->n_v, B, h->ch8, h->ldb, s));
  IbGenArgs cn{}, vn{};
  cn.ch8 = vn.ch8 = h->ch8;
  cn.start = g->cn_start; cn.deg = g->cn_deg; cn.tgt = g->tgt_cn; cn.out = h->vin; cn.lut = h->cn_lut;
  cn.lut_len = h->cn_len; cn.mt = h->mc; cn.mt_len = h->mc_len;
  vn.start = g->vn_start; vn.deg = g->vn_deg; vn.tgt = g->tgt_vn; vn.out = h->cin; vn.in = h->vin; vn.lut = h->vn_lut;
  vn.lut_len = h->vn_len; vn.mt = h->mv; vn.mt_len = h->mv_len;
  cn.Tc = vn.Tc = h->Tc; cn.T = vn.T = h->T; cn.CM = vn.CM = h->CM; cn.VM = vn.VM = h->VM;
  cn.match = vn.match = h->match;
  cn.n_nodes = g->n_c; vn.n_nodes = g->n_v;
  cn.ldb = vn.ldb = h->ldb; cn.B = vn.B = B; cn.half = vn.half = h->T / 2;
  cn.pass = 0; cn.in = nullptr; cn.gather = g->csr_cols;
  HIPCHK(h->timer.timed(0, s, [&] { return launch_ib_cn_gen(cn, s); }));
  cn.in = h->cin; cn.gather = nullptr;
  for (int j = 1; j < I; ++j) {
    const int32_t* gate = flag_row(h->flags, early && j >= 2, j - 1);
    vn.pass = j - 1; vn.gate = gate;
    HIPCHK(h->timer.timed(1, s, [&] { return launch_ib_vn_gen(vn, s); }));
    cn.pass = j; cn.gate = gate; cn.unsat = flag_row(h->flags, early, j);
    HIPCHK(h->timer.timed(0, s, [&] { return launch_ib_cn_gen(cn, s); }));
  }
  HIPCHK(launch_finalize(h->flags, I, early ? 1 : 0, h->dL, d_iters, s));
  IbGenDecArgs dc{};
  dc.vin = h->vin; dc.ch8 = h->ch8; dc.start = g->vn_start; dc.deg = g->vn_deg; dc.lut = h->vn_lut;
  dc.lut_len = h->vn_len; dc.iters = h->dL; dc.out = d_out; dc.out_dtype = out_dtype; dc.Tc = h->Tc; dc.T = h->T;
  dc.VM = h->VM; dc.n_nodes = g->n_v; dc.ldb = h->ldb; dc.B = B;
  HIPCHK(launch_ib_dec_gen(dc, s));
  return IBL_OK;
}
}  // namespace

extern "C" {

int ibl_ib_create(const ibl_graph* g, int32_t Tc, int32_t T, int32_t imax, const int32_t* cn_lut, int64_t cn_len,
                  const int32_t* vn_lut, int64_t vn_len, const int32_t* match_cn, int64_t mc_len,
                  const int32_t* match_vn, int64_t mv_len, int32_t match, int32_t max_batch, int32_t flags,
                  ibl_ib** out) {
  if (!out) return fail(IBL_EINVAL, "out is NULL");
  *out = nullptr;
  if (!g) return fail(IBL_EINVAL, "graph is NULL");
  const IbLuts lu{cn_lut, vn_lut, match_cn, match_vn, cn_len, vn_len, mc_len, mv_len};
  int rc = ib_validate(g, Tc, T, imax, lu, match, max_batch);
  if (rc) return rc;
  HIPCHK(hipSetDevice(g->device));
  std::unique_ptr<ibl_ib> h(new ibl_ib());
  h->g = g;
  h->Tc = Tc; h->T = T; h->imax = imax; h->CM = g->dcm; h->VM = g->dvm; h->match = match ? 1 : 0;
  h->max_batch = max_batch;
  h->ldb = (max_batch + kRowPad - 1) / kRowPad * kRowPad;   // codewords; fast path rows = ldb/2 bytes
  const size_t inbox = (size_t)g->n_e * h->ldb;
  if ((rc = h->cin.alloc_zero(inbox)) || (rc = h->vin.alloc_zero(inbox)) ||
      (rc = h->ch8.alloc_zero((size_t)g->n_v * h->ldb)) || (rc = h->flags.alloc_zero((size_t)imax * kShards)) ||
      (rc = h->dL.alloc(1)))
    return rc;
  const IbSlots sl = ib_plan_slots(h.get(), flags);
  if (h->fast) rc = ib_configure_fast(h.get(), ib_build_images(h.get(), lu, sl));
  else rc = ib_upload_generic(h.get(), lu);
  if (rc) return rc;
  *out = h.release();
  return IBL_OK;
}

int ibl_ib_path(const ibl_ib* h) { return h && h->fast ? 1 : 0; }

int ibl_ib_set_small_batch(ibl_ib* h, int32_t max_b) {
  if (!h) return fail(IBL_EINVAL, "decoder is NULL");
  if (max_b < 0) return fail(IBL_EINVAL, "max_b must be >= 0");
  if (max_b > 0 && !(h->fast && h->s_lds_cn > 0))
    return fail(IBL_EUNSUPPORTED, "the small-batch kernels need the fast path (T_ch = T_dec <= 16, degrees <= 16)");
  if (max_b > 0 && !h->s_ok)   // create turned them off: this build's small-batch kernels need scratch
    return fail(IBL_EUNSUPPORTED, "the small-batch kernels of this build have a private segment: rebuild required");
  h->small_b = max_b;
  return IBL_OK;
}

int ibl_ib_small_batch(const ibl_ib* h, int32_t* max_b) {
  if (!h || !max_b) return fail(IBL_EINVAL, "NULL argument");
  *max_b = h->small_b;
  return IBL_OK;
}

int ibl_ib_set_path(ibl_ib* h, int32_t path) {
  if (!h) return fail(IBL_EINVAL, "decoder is NULL");
  if (int rc = check_path(path)) return rc;
  if (path == IBL_PATH_FUSED && !h->fused_ok)
    return fail(IBL_EUNSUPPORTED, "code does not fit the fused IB kernel (fast path, E * 4 B of messages plus the "
                                  "largest pass's tables within 160 KiB, check degrees >= 2)");
  h->path = path;
  return IBL_OK;
}

int ibl_ib_fused_ncw(const ibl_ib* h, int32_t B, int32_t* ncw) {
  if (!h || !ncw) return fail(IBL_EINVAL, "NULL argument");
  if (B < 1 || B > h->max_batch) return fail(IBL_EINVAL, "B must lie in [1, max_batch]");
  *ncw = ib_fused_in_use(h) ? ib_fused_ncw(h, B) : 0;
  return IBL_OK;
}

int ibl_ib_path_in_use(const ibl_ib* h, int32_t* fused) {
  if (!h || !fused) return fail(IBL_EINVAL, "NULL argument");
  *fused = ib_fused_in_use(h) ? 1 : 0;
  return IBL_OK;
}

int ibl_ib_folded(const ibl_ib* h, int32_t* n_folded) {
  if (!h || !n_folded) return fail(IBL_EINVAL, "NULL argument");
  *n_folded = h->n_folded;
  return IBL_OK;
}

int ibl_ib_set_fold(ibl_ib* h, int32_t on) {
  if (!h) return fail(IBL_EINVAL, "decoder is NULL");
  h->fold_on = on != 0;
  return IBL_OK;
}

int ibl_ib_composite(const ibl_ib* h, int32_t* degree) {
  if (!h || !degree) return fail(IBL_EINVAL, "NULL argument");
  *degree = h->comp_on ? h->comp_deg : 0;
  return IBL_OK;
}

int ibl_ib_set_composite(ibl_ib* h, int32_t on) {
  if (!h) return fail(IBL_EINVAL, "decoder is NULL");
  h->comp_on = on != 0;
  return IBL_OK;
}

int ibl_ib_vn_composite(const ibl_ib* h, int32_t* degree) {
  if (!h || !degree) return fail(IBL_EINVAL, "NULL argument");
  const int view = h->fold_on && h->n_folded > 0 && h->imax > 1 ? 1 : 0;   // the list ib_decode_fast walks
  *degree = h->vcomp_on ? h->vcomp_deg[view] : 0;
  return IBL_OK;
}

int ibl_ib_set_vn_composite(ibl_ib* h, int32_t on) {
  if (!h) return fail(IBL_EINVAL, "decoder is NULL");
  h->vcomp_on = on != 0;
  return IBL_OK;
}

int ibl_ib_timing(ibl_ib* h, int32_t enable) { return timing_enable(h, enable); }
int ibl_ib_timing_read(ibl_ib* h, double* cn_ms, int32_t* cn_n, double* vn_ms, int32_t* vn_n) {
  return timing_read(h, cn_ms, cn_n, vn_ms, vn_n);
}

void ibl_ib_destroy(ibl_ib* h) {
  if (h) (void)hipSetDevice(h->g->device);
  delete h;
}

// the argument checks ibl_ib_decode and ibl_ib_decode_each share
static int ib_decode_check(const ibl_ib* h, const void* d_ch, int32_t ch_dtype, int32_t B, const void* d_out,
                           int32_t out_dtype) {
  if (!h) return fail(IBL_EINVAL, "decoder is NULL");
  if (B < 1 || B > h->max_batch) return fail(IBL_EINVAL, "B must lie in [1, max_batch]");
  if (ch_dtype != kU8 && ch_dtype != kI32) return fail(IBL_EINVAL, "channel dtype must be IBL_U8 or IBL_I32");
  if (out_dtype != kU8 && out_dtype != kI32) return fail(IBL_EINVAL, "output dtype must be IBL_U8 or IBL_I32");
  if (!d_ch || !d_out) return fail(IBL_EINVAL, "NULL buffer");
  return IBL_OK;
}

// (the return type on its own line: tests/test_cpu_host.py lists the `int ..._decode...(` definitions of these files
// by name to hold them to "no read of the environment"; tests/test_cpu_stop_codeword.py holds this one to it)
int
ibl_ib_decode_each(ibl_ib* h, const void* d_ch, int32_t ch_dtype, int32_t B, void* d_out, int32_t out_dtype,
                   int32_t* d_iters, void* stream) {
  if (int rc = ib_decode_check(h, d_ch, ch_dtype, B, d_out, out_dtype)) return rc;
  if (!ib_fused_in_use(h))
    return fail(IBL_EUNSUPPORTED, "the per-codeword stop runs on the fused kernel only (path \"passes\", the generic "
                                  "path, or the code does not fit it)");
  if (!h->f_each_ok)
    return fail(IBL_EUNSUPPORTED, "the per-codeword-stop kernels of this build have a private segment or another "
                                  "occupancy than the fused kernel: rebuild required");
  HIPCHK(hipSetDevice(h->g->device));
  return ib_each_fused(h, d_ch, ch_dtype, B, d_out, out_dtype, d_iters, (hipStream_t)stream);
}

int ibl_ib_decode(ibl_ib* h, const void* d_ch, int32_t ch_dtype, int32_t B, void* d_out, int32_t out_dtype,
                  int32_t early_stop, int32_t* d_iters, void* stream) {
  if (int rc = ib_decode_check(h, d_ch, ch_dtype, B, d_out, out_dtype)) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipSetDevice(h->g->device));
  const bool early = early_stop != 0 && h->imax > 1;
  if (early) HIPCHK(hipMemsetAsync(h->flags, 0, sizeof(int32_t) * (size_t)h->imax * kShards, s));
  if (ib_fused_in_use(h)) return ib_decode_fused(h, d_ch, ch_dtype, B, d_out, out_dtype, early, d_iters, s);
  if (!h->fast) return ib_decode_generic(h, d_ch, ch_dtype, B, d_out, out_dtype, early, d_iters, s);
  if (B <= h->small_b) return ib_decode_small(h, d_ch, ch_dtype, B, d_out, out_dtype, early, d_iters, s);
  return ib_decode_fast(h, d_ch, ch_dtype, B, d_out, out_dtype, early, d_iters, s);
}

}  // extern "C"
