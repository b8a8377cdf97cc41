// C ABI (include/ibldpc.h): the float decoders (min-sum, belief propagation; float_kernels.hip).
//
// Schedules restate the reference's host loops without their per-iteration host sync:
//   decode_OpenCL_min_sum            (Continous_LDPC_Decoding/min_sum_decoder_irreg.py:221-287)
//   decode_OpenCL_belief_propagation (bp_decoder_irreg.py:221-286)
// Early stop: each check-node pass ORs "some check unsatisfied" into 64 flag words of its
// iteration; the launches of the next iteration read those words and exit at once when they
// are all zero, and a one-wave kernel turns the flags into the iteration index the output
// pass uses.  The host only enqueues.
#include <cmath>

#include "host.h"

using namespace ibl;

struct ibl_float {
  const ibl_graph* g = nullptr;
  int32_t kind = 0, imax = 0, prec = kF32, max_batch = 0, ldb = 0;
  double llr_max = 150.0;
  // corrected min-sum (ibl_float_create_corrected): `kind` stays the public IBL_MINSUM (staging rule, messages);
  // kkind is the check-body kind every launch, occupancy and private-segment query takes (0, 1 or 2)
  int32_t kkind = 0;
  double alpha = 1.0, beta = 0.0;
  bool wide = false;        // a check of degree 17..32: the check and fused kernels are the wide instantiations
  DevBuf<uint8_t> cin, vbuf0, vbuf1, chf;   // inboxes and staged channel, fp32 or fp64 elements
  DevBuf<int32_t> flags, dL;
  int grid_cn = 0, grid_vn = 0;
  // degree-2 variable fold of the per-pass path (fl_cn_item): per-check records, the variables the
  // variable pass still updates, the second check inbox (the check passes alternate between cin / cin2)
  DevBuf<uint8_t> cin2;
  DevBuf<int32_t> fold, vn_nodes;
  int32_t n_vn_nodes = 0, n_folded = 0;
  std::vector<int32_t> fold_rec, fold_rest;   // the fold's host plan; uploaded with cin2 once a batch can use it
  DevBuf<int32_t> bad;      // channel LLRs that violated the precondition since the last ibl_float_input_check
  int32_t small_b = 0;      // small-batch kernels (fl_*_small) for B <= small_b (0: off)
  bool s_ok = false;        // the small-batch kernels run without scratch (create's check)
  ChainGraphs s_graphs;     // small-batch pass chains (IBL_SMALL_GRAPH=0 at create: launch them one by one)
  KTimer timer;
  // fused on-chip path (FlFusedArgs): task tables, LDS bytes per workgroup, grid
  int32_t path = IBL_PATH_AUTO;
  bool fused_ok = false;
  FusedTaskBufs ft;
  size_t f_lds = 0;
  int f_grid = 0;
  int f_grid_each = 0;      // the per-codeword-stop form's grid (ibl_float_decode_each)
};

namespace {

// Task tables of the fused float kernel (FlFusedArgs). Check nodes sorted by degree (heaviest first,
// stable) and cut into tasks of up to 64 nodes of one degree; edge k of lane i of a check task gets
// slot first + k*count + i. Variable nodes likewise; vn_slot maps each variable edge (task-major,
// k*count + i) to the slot of the same edge. Leaves fused_ok false when the code does not fit.
int fused_setup(ibl_float* h) {
  const ibl_graph* g = h->g;
  const int64_t E = g->n_e;
  if (E >= 65536 || g->dc_min < 2 || E == 0 || (size_t)(E + g->n_v) * 16 > (size_t)kLdsBytes) return IBL_OK;
  FusedTasks ft;
  // 16-byte slots (ds_read_b128 / ds_write_b128): the natural order (stable by degree) keeps a quasi-cyclic
  // code's lanes on runs of consecutive slots, which conflict less than the dword-bank greedy order;
  // IBL_FUSED_VORDER=1 selects the greedy order (A/B)
  const char* voe = getenv("IBL_FUSED_VORDER");
  build_fused_tasks(*g, &ft, voe && voe[0] == '1', fused_vwin());
  pad_vn_slots(&ft);
  // messages and channel (16-byte slots), 4 words (two ticket counters, the per-codeword stop's two mask words),
  // the padded u16 indices (codes whose indices do not fit beside the messages take the per-pass path)
  const size_t lds = (size_t)(E + g->n_v) * 16 + 16 + ft.vn_slot.size() * 2;
  if (lds > (size_t)kLdsBytes) return IBL_OK;
  int bpc = 0, block = 0;
  if (fl_occupancy(kFlFused, kFlCheck, h->kkind, h->prec, g->dcm, g->dvm, lds, &bpc, &block) != hipSuccess || bpc < 1) {
    (void)hipGetLastError();
    return IBL_OK;
  }
  // the per-codeword-stop form: same LDS; its own register count decides its grid
  int bpe = 0;
  if (fl_occupancy(kFlFused, kFlCheck, h->kkind, h->prec, g->dcm, g->dvm, lds, &bpe, &block, true) != hipSuccess || bpe < 1) {
    (void)hipGetLastError();
    return IBL_OK;
  }
  if (int rc = h->ft.upload(ft)) return rc;
  h->f_lds = lds;
  h->f_grid = bpc * g->num_cus;
  h->f_grid_each = bpe * g->num_cus;
  h->fused_ok = true;
  return IBL_OK;
}

// Launch geometry of the fused float kernel for a batch of B: groups of 4 fp32 / 2 fp64 codewords, one per
// workgroup round (fl_fused's group loop); the decode and ibl_float_fused_geometry both take it from here.
void float_fused_geometry(const ibl_float* h, int B, int32_t* ngroups, int32_t* grid) {
  const int cwl = fl_cw_per_lane(h->prec);
  *ngroups = (B + cwl - 1) / cwl;
  *grid = std::min(*ngroups, h->f_grid);
}

// The fold's device state (second check inbox, per-check records, unfolded variable list) once a batch can reach
// the per-pass kernels (max_batch > small_b): decoders that only ever run the small-batch kernels — the
// reference's DVB-S2 driver decodes msg_at_time = 2 — do not hold a fourth E x ldb inbox. cin2 is set last:
// cin2 set <=> the fold's state is complete.
int fold_alloc(ibl_float* h) {
  if (h->n_folded == 0 || h->cin2 || h->max_batch <= h->small_b) return IBL_OK;
  DevBuf<uint8_t> c2;
  DevBuf<int32_t> fold, nodes;
  int rc;
  if ((rc = c2.alloc_zero((size_t)h->g->n_e * h->ldb * fl_elem_size(h->prec))) || (rc = fold.upload(h->fold_rec)) ||
      (rc = nodes.upload(h->fold_rest)))
    return rc;
  h->fold = std::move(fold);
  h->vn_nodes = std::move(nodes);
  h->cin2 = std::move(c2);
  return IBL_OK;
}

// the staging kernels count precondition violations (float_kernels.hip llr_bad): min-sum NaN; BP NaN and, for
// the fp64 decoder, |x| > 709.089 (just under ln(DBL_MAX / 2)), for the fp32 decoder +-inf
int stage_rule(const ibl_float* h) { return h->kind == IBL_BP ? (h->prec == kF64 ? 2 : 3) : 1; }

// The send, check, variable and decision arguments that the small-batch and the per-pass schedule share, for a
// batch of B in rows of ldb codewords. The schedules add their tasks or chunks and the fold, and set the buffers
// and gates of each pass.
struct FlPassArgs {
  FlArgs send{}, cn{}, vn{};
  FlDecArgs dec{};
};
FlPassArgs float_pass_args(const ibl_float* h, int B, int ldb, void* d_out, int32_t out_dtype) {
  const ibl_graph* g = h->g;
  FlPassArgs p;
  p.send.ch = p.cn.ch = p.vn.ch = p.dec.ch = h->chf;
  p.send.out = h->cin;
  p.send.start = p.vn.start = p.dec.start = g->vn_start;
  p.send.deg = p.vn.deg = p.dec.deg = g->vn_deg;
  p.send.tgt = p.vn.tgt = g->tgt_vn;
  p.cn.start = g->cn_start; p.cn.deg = g->cn_deg; p.cn.tgt = g->tgt_cn;
  p.cn.llr_max = p.vn.llr_max = h->llr_max;
  p.cn.cor_a = h->alpha; p.cn.cor_b = h->beta;
  p.cn.n_nodes = g->n_c;
  p.send.n_nodes = p.vn.n_nodes = p.dec.n_nodes = g->n_v;
  p.send.ldb = p.cn.ldb = p.vn.ldb = p.dec.ldb = ldb;
  p.send.B = p.cn.B = p.vn.B = p.dec.B = B;
  p.dec.vin0 = h->vbuf0; p.dec.vin1 = h->vbuf1; p.dec.iters = h->dL; p.dec.out = d_out; p.dec.out_dtype = out_dtype;
  return p;
}

// The fused kernel's arguments for a batch of B, but for the stop (unsat / dL, or iters); *grid: float_fused_geometry's
FlFusedArgs float_fused_args(const ibl_float* h, int32_t B, void* d_out, int32_t out_dtype, int* grid) {
  const ibl_graph* g = h->g;
  FlFusedArgs fa{};
  fa.ch = h->chf; fa.cn_task = h->ft.cn_task; fa.vn_task = h->ft.vn_task; fa.vn_node = h->ft.vn_node;
  fa.vn_slot = h->ft.vn_slot; fa.out = d_out;
  fa.llr_max = h->llr_max; fa.n_e = (int32_t)g->n_e; fa.n_v = g->n_v; fa.n_cn_tasks = h->ft.n_cn;
  fa.cor_a = h->alpha; fa.cor_b = h->beta;
  fa.n_vn_tasks = h->ft.n_vn; fa.n_vs = h->ft.n_vs; fa.ldb = h->ldb; fa.B = B; fa.imax = h->imax; fa.out_dtype = out_dtype;
  float_fused_geometry(h, B, &fa.ngroups, grid);
  fa.aligned = out_aligned(B, d_out, fl_cw_per_lane(h->prec), fl_elem_size(out_dtype));
  return fa;
}

// Per-codeword stop (ibldpc.h "Per-codeword stop"): the staging launch and one launch of fl_fused<kind | kFlEach, ..>; no flag
// words, no finalize_iters, no second pass.
int float_each_fused(ibl_float* h, const void* d_llr, int32_t llr_dtype, int32_t B, void* d_out, int32_t out_dtype,
                     int32_t* d_iters, hipStream_t s) {
  const ibl_graph* g = h->g;
  HIPCHK(launch_fl_stage_t(d_llr, llr_dtype, g->n_v, B, h->ft.vn_node, h->chf, h->prec, stage_rule(h), h->bad, s));
  int grid = 0;
  FlFusedArgs fa = float_fused_args(h, B, d_out, out_dtype, &grid);
  fa.iters = d_iters;
  grid = std::min(fa.ngroups, h->f_grid_each);
  HIPCHK(h->timer.timed(0, s, [&] {
    return launch_fl_fused(fa, h->kkind, h->prec, g->dcm, g->dvm, grid, h->f_lds, s, true);
  }));
  return IBL_OK;
}

int float_decode_fused(ibl_float* h, const void* d_llr, int32_t llr_dtype, int32_t B, void* d_out, int32_t out_dtype,
                       bool early, int32_t* d_iters, hipStream_t s) {
  const ibl_graph* g = h->g;
  const int I = h->imax;
  HIPCHK(launch_fl_stage_t(d_llr, llr_dtype, g->n_v, B, h->ft.vn_node, h->chf, h->prec, stage_rule(h), h->bad, s));
  int grid = 0;
  FlFusedArgs fa = float_fused_args(h, B, d_out, out_dtype, &grid);
  fa.unsat = flag_row(h->flags, early, 0); fa.dL = nullptr;
  auto launch = [&] { return launch_fl_fused(fa, h->kkind, h->prec, g->dcm, g->dvm, grid, h->f_lds, s); };
#if IBL_DIAG
  const char* ftrace = getenv("IBL_TRACE_FUSED");   // diagnostic builds: phase clocks of block 0's first group
  TraceBuf tr;
  int rc;
  if (ftrace) {
    if ((rc = tr.open((size_t)kFlTraceWords * (2 * I + 4), s))) return rc;
    fa.trace = tr.d;
  }
#endif
  HIPCHK(h->timer.timed(0, s, launch));
#if IBL_DIAG
  if (ftrace && (rc = tr.save(s, ftrace, 0, tr.n))) return rc;
  fa.trace = nullptr;
#endif
  HIPCHK(launch_finalize(h->flags, I, early ? 1 : 0, h->dL, d_iters, s));
  if (early) {   // batch-global stop before imax-1: re-run the batch to L (the kernel exits if L = imax-1)
    fa.unsat = nullptr;
    fa.dL = h->dL;
    HIPCHK(h->timer.timed(0, s, launch));
  }
  return IBL_OK;
}

// small batch: (task, word) items, lane = node (fl_*_small); the per-pass schedule without the fold.
// Rows packed to the batch (B rounded up to 4 codewords: fl_send's quads, 16-byte pieces) instead of
// the per-pass path's ldb, so a pass touches E x ldbs elements of each inbox, not one line per edge
int float_decode_small(ibl_float* h, const void* d_llr, int32_t llr_dtype, int32_t B, void* d_out, int32_t out_dtype,
                       bool early, int32_t* d_iters, hipStream_t s) {
  const ibl_graph* g = h->g;
  const int I = h->imax, cwl = fl_cw_per_lane(h->prec);
  const int nwords = (B + cwl - 1) / cwl, ldbs = (B + 3) / 4 * 4;
  HIPCHK(launch_fl_stage(d_llr, llr_dtype, g->n_v, B, h->chf, h->prec, ldbs, stage_rule(h), h->bad, s));
  auto grid_of = [&](int ntask) {
    const int need = (ntask * nwords + kFlSmallBlock / 64 - 1) / (kFlSmallBlock / 64);
    return std::max(1, std::min(need, 4 * g->num_cus));
  };
  FlPassArgs pa = float_pass_args(h, B, ldbs, d_out, out_dtype);
  const FlArgs& send = pa.send;
  FlArgs &cn = pa.cn, &vn = pa.vn;
  FlDecArgs& dc = pa.dec;
  cn.in = h->cin;
  vn.out = h->cin;
  cn.info = g->cn_info; cn.task = g->cn_task; cn.n_tasks = g->n_cn_task;
  vn.info = dc.info = g->vn_info; vn.task = dc.task = g->vn_task; vn.n_tasks = dc.n_tasks = g->n_vn_task;
  cn.nwords = vn.nwords = dc.nwords = nwords;
  const int gcn = grid_of(g->n_cn_task), gvn = grid_of(g->n_vn_task);
  // the pass chain (decoder buffers only): send, then {CN j, VN j} — replayed from a captured graph (ChainGraphs)
  auto chain = [&](hipStream_t st) -> hipError_t {
    hipError_t e = launch_fl_send(send, h->prec, st);
    if (e != hipSuccess) return e;
    FlArgs c = cn, v = vn;
    for (int j = 1; j < I; ++j) {
      void* vb = (j & 1) ? h->vbuf1 : h->vbuf0;
      c.out = vb;
      c.gate = flag_row(h->flags, early && j >= 3, j - 2);
      c.unsat = flag_row(h->flags, early, j - 1);
      if ((e = h->timer.timed(0, st, [&] { return launch_fl_pass(kFlSmall, kFlCheck, c, h->kkind, h->prec, g->dcm, gcn, st); })) != hipSuccess)
        return e;
      if (j == I - 1) break;   // the last variable pass feeds no output (as in float_decode_passes)
      v.in = vb;
      v.gate = flag_row(h->flags, early && j >= 2, j - 1);
      if ((e = h->timer.timed(1, st, [&] { return launch_fl_pass(kFlSmall, kFlVariable, v, 0, h->prec, g->dvm, gvn, st); })) != hipSuccess)
        return e;
    }
    return hipSuccess;
  };
  if (h->s_graphs.on && !h->timer.on) HIPCHK(h->s_graphs.run(B, early ? 1 : 0, s, chain));
  else HIPCHK(chain(s));
  HIPCHK(launch_finalize(h->flags, I, early ? 1 : 0, h->dL, d_iters, s));
  HIPCHK(launch_fl_dec(kFlSmall, dc, h->prec, gvn, s));
  return IBL_OK;
}

int float_decode_passes(ibl_float* h, const void* d_llr, int32_t llr_dtype, int32_t B, void* d_out, int32_t out_dtype,
                        bool early, int32_t* d_iters, hipStream_t s) {
  const ibl_graph* g = h->g;
  const int I = h->imax, cwl = fl_cw_per_lane(h->prec);
  const int nchunks = (B + fl_vn_chunk(h->prec) - 1) / fl_vn_chunk(h->prec);
  HIPCHK(launch_fl_stage(d_llr, llr_dtype, g->n_v, B, h->chf, h->prec, h->ldb, stage_rule(h), h->bad, s));
  FlPassArgs pa = float_pass_args(h, B, h->ldb, d_out, out_dtype);
  FlArgs &cn = pa.cn, &vn = pa.vn;
  FlDecArgs& dc = pa.dec;
  HIPCHK(launch_fl_send(pa.send, h->prec, s));
  // Check pass j reads check inbox cb[j & 1] (send fills cb[1]) and writes the variable inbox vbuf[j & 1];
  // variable pass j writes cb[(j + 1) & 1]. With the fold, check pass j also writes its folded variables'
  // messages into cb[(j + 1) & 1], and the variable pass skips them; the last check pass writes every
  // variable-inbox row (the decision reads them) and folds nothing. The last iteration's variable pass
  // only feeds a syndrome the reference never reads (its loop ends at imax, bp_decoder_irreg.py:240-268),
  // so it is not run.
  if (h->n_folded > 0 && !h->cin2) return fail(IBL_EHIP, "fold inbox missing (fold_alloc)");
  const bool fold = h->n_folded > 0;
  void* cb[2] = {fold ? h->cin2 : h->cin, h->cin};
  cn.fold = h->fold;
  if (fold) {   // the variable pass updates the variables that are not folded
    vn.nodes = h->vn_nodes.get();
    vn.n_nodes = h->n_vn_nodes;
  }
  cn.nchunks = vn.nchunks = dc.nchunks = nchunks;
  for (int j = 1; j < I; ++j) {
    void* vb = (j & 1) ? h->vbuf1 : h->vbuf0;
    const bool last = j == I - 1;
    cn.in = cb[j & 1];
    cn.out = vb;
    cn.fout = cb[(j + 1) & 1];
    cn.fold_mode = (fold && !last) ? (early ? 2 : 1) : 0;
    cn.gate = flag_row(h->flags, early && j >= 3, j - 2);
    cn.unsat = flag_row(h->flags, early, j - 1);
    HIPCHK(h->timer.timed(0, s, [&] { return launch_fl_pass(kFlPerPass, kFlCheck, cn, h->kkind, h->prec, g->dcm, h->grid_cn, s); }));
    if (last) break;
    vn.in = vb;
    vn.out = cb[(j + 1) & 1];
    vn.gate = flag_row(h->flags, early && j >= 2, j - 1);
    HIPCHK(h->timer.timed(1, s, [&] { return launch_fl_pass(kFlPerPass, kFlVariable, vn, 0, h->prec, g->dvm, h->grid_vn, s); }));
  }
  HIPCHK(launch_finalize(h->flags, I, early ? 1 : 0, h->dL, d_iters, s));
  dc.aligned = out_aligned(B, d_out, cwl, fl_elem_size(out_dtype));
  const size_t items = (size_t)g->n_v * nchunks;
  HIPCHK(launch_fl_dec(kFlPerPass, dc, h->prec, (int)std::min<size_t>((items + 3) / 4, 65536), s));
  return IBL_OK;
}

// The decoder behind ibl_float_create and ibl_float_create_corrected (parameters checked by the callers). kkind is
// the check-body kind of the kernels: `kind`, or 2 for corrected min-sum with (alpha, beta) != (1, 0).
int float_create(const ibl_graph* g, int32_t kind, int32_t kkind, double alpha, double beta, int32_t imax,
                 double llr_max, int32_t precision, int32_t max_batch, ibl_float** out) {
  if (g->dcm > kFlWideD)
    return fail(IBL_EUNSUPPORTED, "float decoders support check degrees <= 32 (the code has a check of degree " +
                                      std::to_string(g->dcm) + ")");
  if (g->dvm > kMaxD)
    return fail(IBL_EUNSUPPORTED, "float decoders support variable degrees <= 16 (the code has a variable of degree " +
                                      std::to_string(g->dvm) + ")");
  HIPCHK(hipSetDevice(g->device));
  std::unique_ptr<ibl_float> h(new ibl_float());
  h->wide = g->dcm > kMaxD;
  h->g = g; h->kind = kind; h->imax = imax; h->prec = precision; h->max_batch = max_batch; h->llr_max = llr_max;
  h->kkind = kkind; h->alpha = alpha; h->beta = beta;
  // rows padded to the wave item of the per-pass kernels (fp32 256 / fp64 128 codewords), not beyond: the
  // reference's DVB-S2 driver decodes msg_at_time = 2 in fp64
  const int pad = fl_vn_chunk(precision);
  h->ldb = (max_batch + pad - 1) / pad * pad;
  const size_t es = fl_elem_size(precision);
  const size_t inbox = (size_t)g->n_e * h->ldb * es;
  int rc;
  if ((rc = h->cin.alloc_zero(inbox)) || (rc = h->vbuf0.alloc_zero(inbox)) || (rc = h->vbuf1.alloc_zero(inbox)) ||
      (rc = h->chf.alloc((size_t)g->n_v * h->ldb * es)) || (rc = h->flags.alloc((size_t)imax * kShards)) ||
      (rc = h->dL.alloc(1)) || (rc = h->bad.alloc_zero(1)))
    return rc;
  int bpc = 0, block = 0;
  // at most 16 waves per CU: with a second block per CU its waves issue behind the first block's
  // (oldest-first) and the per-block work counters cannot rebalance across blocks
  if (fl_occupancy(kFlPerPass, kFlCheck, kkind, precision, g->dcm, g->dvm, 0, &bpc, &block) != hipSuccess || bpc < 1) bpc = 1;
  // (A/B knob, read once here: IBL_FL_WAVES = waves per CU the per-pass grids may fill, default 16)
  const char* fw = getenv("IBL_FL_WAVES");
  const int wcap = std::max(16, fw ? atoi(fw) : 16) * 64;
  h->grid_cn = std::min(bpc, wcap / block) * g->num_cus;
  if (fl_occupancy(kFlPerPass, kFlVariable, kkind, precision, g->dcm, g->dvm, 0, &bpc, &block) != hipSuccess || bpc < 1) bpc = 1;
  h->grid_vn = std::min(bpc, wcap / block) * g->num_cus;
  if ((rc = fused_setup(h.get()))) return rc;
  // degree-2 variable fold of the per-pass path (IBL_FL_FOLD=0 at create turns it off: A/B); its second check
  // inbox is allocated only once some batch can reach the per-pass kernels (max_batch > small_b, fold_alloc)
  if (env_on("IBL_FL_FOLD") && (h->n_folded = plan_fold(*g, &h->fold_rec, &h->fold_rest)) > 0)
    h->n_vn_nodes = (int32_t)h->fold_rest.size();
  else
    h->n_folded = 0;
  // same guard as the IB fast path: the float kernels are built to run without scratch
  size_t priv = 0;
  const char* kname = "";
  HIPCHK(fl_private_bytes(kFlPerPass, kkind, precision, g->dcm, g->dvm, h->fused_ok, &priv, &kname));
  if ((rc = refuse_private(priv, std::string("float kernel ") + kname + " has a ",
                           "-byte private segment (register spill): rebuild required")))
    return rc;
  // small-batch kernels (IBL_SMALL_B at create overrides the default; off if they would need scratch)
  HIPCHK(fl_private_bytes(kFlSmall, kkind, precision, g->dcm, g->dvm, false, &priv, &kname));
  h->s_ok = priv == 0;
  small_batch_env(h->s_ok, kFlSmallBatchDefault, &h->small_b, &h->s_graphs);
  if ((rc = fold_alloc(h.get()))) return rc;
  *out = h.release();
  return IBL_OK;
}
}  // namespace

extern "C" {

int ibl_float_set_path(ibl_float* h, int32_t path) {
  if (!h) return fail(IBL_EINVAL, "decoder is NULL");
  if (int rc = check_path(path)) return rc;
  if (path == IBL_PATH_FUSED && !h->fused_ok)
    return fail(IBL_EUNSUPPORTED, "code does not fit the fused kernel ((E + N) * 16 B > 160 KiB or a check degree < 2)");
  h->path = path;
  return IBL_OK;
}

int ibl_float_set_small_batch(ibl_float* h, int32_t max_b) {
  if (!h) return fail(IBL_EINVAL, "decoder is NULL");
  if (max_b < 0) return fail(IBL_EINVAL, "max_b must be >= 0");
  if (max_b > 0 && !h->s_ok)   // create turned them off: this build's small-batch kernels need scratch
    return fail(IBL_EUNSUPPORTED, "the small-batch kernels of this build have a private segment: rebuild required");
  HIPCHK(hipSetDevice(h->g->device));
  const int32_t old = h->small_b;
  h->small_b = max_b;
  int rc = fold_alloc(h);   // batches above the new threshold take the per-pass kernels, which fold
  if (rc) h->small_b = old;
  return rc;
}

int ibl_float_small_batch(const ibl_float* h, int32_t* max_b) {
  if (!h || !max_b) return fail(IBL_EINVAL, "NULL argument");
  *max_b = h->small_b;
  return IBL_OK;
}

int ibl_float_folded(const ibl_float* h, int32_t* n_folded) {
  if (!h || !n_folded) return fail(IBL_EINVAL, "NULL argument");
  *n_folded = h->n_folded;
  return IBL_OK;
}

int ibl_float_is_wide(const ibl_float* h, int32_t* wide) {
  if (!h || !wide) return fail(IBL_EINVAL, "NULL argument");
  *wide = h->wide ? 1 : 0;
  return IBL_OK;
}

int ibl_float_input_check(ibl_float* h, int32_t* violations, void* stream) {
  if (!h) return fail(IBL_EINVAL, "decoder is NULL");
  // The counter belongs to the decoder and collects every decode's staging, on any stream: synchronise the whole
  // device (not only `stream`) so no decode still in flight elsewhere adds to it between the read and the clear.
  (void)stream;
  HIPCHK(hipSetDevice(h->g->device));
  HIPCHK(hipDeviceSynchronize());
  int32_t n = 0;
  HIPCHK(hipMemcpy(&n, h->bad, sizeof(int32_t), hipMemcpyDeviceToHost));
  HIPCHK(hipMemset(h->bad, 0, sizeof(int32_t)));
  if (violations) *violations = n;
  if (n > 0)
    return fail(IBL_EINVAL, std::to_string(n) + (h->kind == IBL_BP
                                                     ? (h->prec == kF64 ? " channel LLR(s) NaN or |x| > 709.089 (BP precondition)"
                                                                          : " channel LLR(s) NaN or infinite (BP precondition)")
                                                     : " channel LLR(s) NaN (min-sum precondition)") +
                                ": those decodes' outputs are unspecified");
  return IBL_OK;
}

int ibl_float_fused_geometry(const ibl_float* h, int32_t B, int32_t* ngroups, int32_t* grid) {
  if (!h || !ngroups || !grid) return fail(IBL_EINVAL, "NULL argument");
  if (B < 1 || B > h->max_batch) return fail(IBL_EINVAL, "B must lie in [1, max_batch]");
  *ngroups = *grid = 0;
  if (h->fused_ok && h->path != IBL_PATH_PASSES) float_fused_geometry(h, B, ngroups, grid);
  return IBL_OK;
}

int ibl_float_path_in_use(const ibl_float* h, int32_t* fused) {
  if (!h || !fused) return fail(IBL_EINVAL, "NULL argument");
  *fused = (h->fused_ok && h->path != IBL_PATH_PASSES) ? 1 : 0;
  return IBL_OK;
}

int ibl_float_timing(ibl_float* h, int32_t enable) { return timing_enable(h, enable); }
int ibl_float_timing_read(ibl_float* h, double* cn_ms, int32_t* cn_n, double* vn_ms, int32_t* vn_n) {
  return timing_read(h, cn_ms, cn_n, vn_ms, vn_n);
}

int ibl_float_create(const ibl_graph* g, int32_t kind, int32_t imax, double llr_max, int32_t precision,
                     int32_t max_batch, ibl_float** out) {
  if (!out) return fail(IBL_EINVAL, "out is NULL");
  *out = nullptr;
  if (!g) return fail(IBL_EINVAL, "graph is NULL");
  if (kind != IBL_MINSUM && kind != IBL_BP) return fail(IBL_EINVAL, "kind must be IBL_MINSUM or IBL_BP");
  if (precision != kF32 && precision != kF64) return fail(IBL_EINVAL, "precision must be IBL_F32 or IBL_F64");
  if (imax < 1 || max_batch < 1) return fail(IBL_EINVAL, "imax and max_batch must be >= 1");
  return float_create(g, kind, kind, 1.0, 0.0, imax, llr_max, precision, max_batch, out);
}

int ibl_float_create_corrected(const ibl_graph* g, double alpha, double beta, int32_t imax, double llr_max,
                               int32_t precision, int32_t max_batch, ibl_float** out) {
  if (!out) return fail(IBL_EINVAL, "out is NULL");
  *out = nullptr;
  // parameter errors before the NULL graph (as ibl_layered_create_fixed): they need no device
  if (!std::isfinite(alpha) || !(alpha > 0.0) || alpha > 1.0) return fail(IBL_EINVAL, "alpha must be finite with 0 < alpha <= 1");
  if (!std::isfinite(beta) || beta < 0.0) return fail(IBL_EINVAL, "beta must be finite and >= 0");
  if (precision != kF32 && precision != kF64) return fail(IBL_EINVAL, "precision must be IBL_F32 or IBL_F64");
  // the domain holds for a = (F)alpha and b = (F)beta, the values the kernels compute with: an alpha that rounds
  // to 0 in fp32 would zero every check message, a beta that rounds to inf every nonzero one
  if (precision == kF32 && (!((float)alpha > 0.f) || !std::isfinite((float)beta)))
    return fail(IBL_EINVAL, !((float)alpha > 0.f) ? "alpha rounds to 0 in fp32: (float)alpha must be > 0"
                                                  : "beta rounds to infinity in fp32: (float)beta must be finite");
  beta += 0.0;   // -0.0 is 0: stored, used and reported as +0
  if (imax < 1 || max_batch < 1) return fail(IBL_EINVAL, "imax and max_batch must be >= 1");
  if (!g) return fail(IBL_EINVAL, "graph is NULL");
  // (1, 0) is plain min-sum: the decoder ibl_float_create(IBL_MINSUM) makes, with its kernels
  const bool plain = alpha == 1.0 && beta == 0.0;
  return float_create(g, IBL_MINSUM, plain ? 0 : 2, alpha, beta, imax, llr_max, precision, max_batch, out);
}

int ibl_float_correction(const ibl_float* h, double* alpha, double* beta) {
  if (!h || !alpha || !beta) return fail(IBL_EINVAL, "NULL argument");
  if (h->kind != IBL_MINSUM) return fail(IBL_EINVAL, "a BP decoder has no min-sum correction");
  *alpha = h->alpha;
  *beta = h->beta;
  return IBL_OK;
}

void ibl_float_destroy(ibl_float* h) {
  if (h) (void)hipSetDevice(h->g->device);
  delete h;
}

// the argument checks ibl_float_decode and ibl_float_decode_each share
static int float_decode_check(const ibl_float* h, const void* d_llr, int32_t llr_dtype, int32_t B, const void* d_out,
                              int32_t out_dtype) {
  if (!h) return fail(IBL_EINVAL, "decoder is NULL");
  if (B < 1 || B > h->max_batch) return fail(IBL_EINVAL, "B must lie in [1, max_batch]");
  if ((llr_dtype != kF32 && llr_dtype != kF64) || (out_dtype != kF32 && out_dtype != kF64))
    return fail(IBL_EINVAL, "LLR dtypes must be IBL_F32 or IBL_F64");
  if (!d_llr || !d_out) return fail(IBL_EINVAL, "NULL buffer");
  return IBL_OK;
}

// (the return type on its own line: tests/test_cpu_host.py lists the `int ..._decode...(` definitions of these files
// by name to hold them to "no read of the environment"; tests/test_cpu_stop_codeword.py holds this one to it)
int
ibl_float_decode_each(ibl_float* h, const void* d_llr, int32_t llr_dtype, int32_t B, void* d_out,
                      int32_t out_dtype, int32_t* d_iters, void* stream) {
  if (int rc = float_decode_check(h, d_llr, llr_dtype, B, d_out, out_dtype)) return rc;
  if (!(h->fused_ok && h->path != IBL_PATH_PASSES))
    return fail(IBL_EUNSUPPORTED, "the per-codeword stop runs on the fused kernel only (path \"passes\", or the code "
                                  "does not fit it)");
  HIPCHK(hipSetDevice(h->g->device));
  return float_each_fused(h, d_llr, llr_dtype, B, d_out, out_dtype, d_iters, (hipStream_t)stream);
}

int ibl_float_decode(ibl_float* h, const void* d_llr, int32_t llr_dtype, int32_t B, void* d_out, int32_t out_dtype,
                     int32_t early_stop, int32_t* d_iters, void* stream) {
  if (int rc = float_decode_check(h, d_llr, llr_dtype, B, d_out, out_dtype)) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipSetDevice(h->g->device));
  const bool early = early_stop != 0 && h->imax > 1;
  if (early) HIPCHK(hipMemsetAsync(h->flags, 0, sizeof(int32_t) * (size_t)h->imax * kShards, s));
  if (h->fused_ok && h->path != IBL_PATH_PASSES)
    return float_decode_fused(h, d_llr, llr_dtype, B, d_out, out_dtype, early, d_iters, s);
  if (B <= h->small_b) return float_decode_small(h, d_llr, llr_dtype, B, d_out, out_dtype, early, d_iters, s);
  return float_decode_passes(h, d_llr, llr_dtype, B, d_out, out_dtype, early, d_iters, s);
}

}  // extern "C"
