// C ABI (include/ibldpc.h): the layered normalised / offset min-sum decoder (layered_plan.h, layered_kernels.hip):
// the fused on-chip kernel for codes whose codeword state fits the LDS, the per-layer path over HBM otherwise, and
// the fixed-point arithmetic on the per-layer path (ibl_layered_create_fixed) and fused on chip
// (ibl_layered_create_fixed_fused); and the layered BP decoder (layered_bp_kernels.hip, ibl_layered_create_bp) on both
// paths, with fp32 or half-precision state (layered_half_kernels.hip, ibl_layered_create_bp_half).
#include <cmath>
#include <cstring>

#include "host.h"
#include "layered_plan.h"

using namespace ibl;

struct ibl_layered {
  const ibl_graph* g = nullptr;
  int32_t imax = 0, max_batch = 0, n_tasks = 0, cw_per_group = 0, bpc = 1;
  float alpha = 1.f, beta = 0.f, llr_max = 150.f;
  size_t cw_bytes = 0;
  DevBuf<int32_t> task, idx;
  DevBuf<float> buf;        // [max_batch][n_v] codeword rows
  // per-layer path over HBM (fused = 0): the plan's records, the layers' first slots and the scratch of
  // layered_plan.h pass_bytes(n_v, n_c, max_batch)
  int32_t fused = 1;
  std::vector<int32_t> layer_slot;
  DevBuf<int32_t> rec;
  DevBuf<float> P, M1, M2;
  DevBuf<uint32_t> PS;
  DevBuf<uint64_t> done, unsat, bits;
  DevBuf<int32_t> running;
  int32_t syn_packed = 1;   // syndrome form (IBL_LAY_SYNDROME=gather|packed at create; DESIGN.md for the numbers)
  // fixed point (ibl_layered_create_fixed; fused = 0): rec, layer_slot, the masks, the counter and bits as above,
  // the int8 APP rows and the state words of layered_plan.h fix_bytes(n_v, n_c, max_batch)
  int32_t fixed = 0, alpha16 = 16, beta_q = 0, q_max = 31;
  float scale = 2.f;
  DevBuf<int8_t> P8;
  DevBuf<uint32_t> S;
  // compaction of the running codewords (ibl_layered_set_compaction; fp32 per-layer path): every = 0 is off; the
  // state of layered_plan.h pass_compact_bytes(max_batch), allocated when first switched on
  int32_t compact_every = 0, compact_pct = 0;
  DevBuf<int32_t> orig, dest, ctl;
  int32_t last_B = 0, last_compact = 0;   // the last decode: its batch, and whether it ran with compaction
  // wide (a check of degree 17..32; layered_plan.h layered_is_wide): the *_wide kernels and one more state array,
  // PO [n_c][ldb] on the fp32 per-layer path, S1 [n_c][ldb] in fixed point (the fused kernel's PO is in LDS)
  int32_t wide = 0;
  DevBuf<uint32_t> PO, S1;
  // fixed point, fused on chip (ibl_layered_create_fixed_fused; fixed = 1, fused = 1): task, idx, n_tasks,
  // cw_per_group, cw_bytes and bpc as on the fp32 fused handle, and the [max_batch][ldn] int8 codeword rows of
  // layered_plan.h fixfused_buf_bytes(n_v, max_batch)
  DevBuf<int8_t> buf8;
  // layered BP (ibl_layered_create_bp; fixed = 0, wide = 0): fused = 1 uses task, idx, buf, n_tasks, cw_per_group,
  // cw_bytes (4 N + 4 E) and bpc as above; fused = 0 uses rec, layer_slot, P, the masks, the counter and bits, and R
  // [E][ldb], the check messages (layered_plan.h laybp_pass_bytes)
  int32_t bp = 0;
  DevBuf<float> R;
  // layered BP with half-precision state (ibl_layered_create_bp_half; bp = 1, half = 1): fused = 1 as the fp32 BP
  // handle with cw_bytes = 2 N + 2 E rounded up to 4; fused = 0 uses rec, layer_slot, the masks, the counter and bits,
  // and P16 [n_v][ldb], R16 [E][ldb] (layered_plan.h layhp_pass_bytes)
  int32_t half = 0;
  DevBuf<uint16_t> P16, R16;
};

namespace {
std::vector<int32_t> graph_indptr(const ibl_graph* g) {
  std::vector<int32_t> ip((size_t)g->n_c + 1, 0);
  for (int32_t c = 0; c < g->n_c; ++c) ip[(size_t)c + 1] = ip[c] + g->h_cn_deg[c];
  return ip;
}
void layered_geometry(const ibl_layered* h, int B, int32_t* ngroups, int32_t* grid) {
  *ngroups = (B + h->cw_per_group - 1) / h->cw_per_group;
  *grid = std::min(*ngroups, h->bpc * h->g->num_cus);
}

// The per-layer handle (layers already validated): plan, records and all scratch for max_batch.
int layered_create_passes(const ibl_graph* g, const std::vector<int32_t>& ip, int32_t n_layers,
                          const int32_t* layer_ptr, const int32_t* layer_checks, int32_t imax, float alpha, float beta,
                          float llr_max, int32_t max_batch, ibl_layered** out) {
  LayeredPassPlan pl;
  plan_layered_passes(g->n_c, ip.data(), n_layers, layer_ptr, layer_checks, &pl);
  const int64_t rows = std::max(g->n_v, g->n_c);
  if (pass_grid(pl.max_layer, max_batch) > 0x7fffffffll || pass_grid(pass_syn_runs(g->n_c), max_batch) > 0x7fffffffll ||
      (rows * pass_tiles(max_batch) + kLayPassWaves - 1) / kLayPassWaves > 0x7fffffffll)
    return fail(IBL_EINVAL, "max_batch is too large for the per-layer kernels' grids");
  HIPCHK(hipSetDevice(g->device));
  const bool wide = layered_is_wide(g->n_c, ip.data());
  size_t priv = 0, priv_wide = 0;
  HIPCHK(lay_pass_private_bytes(&priv));
  if (wide) HIPCHK(lay_wide_private_bytes(&priv_wide));
  int rc = refuse_private(std::max(priv, priv_wide), "a per-layer layered kernel has a ",
                          "-byte private segment (register spill): rebuild required");
  if (rc) return rc;
  std::unique_ptr<ibl_layered> h(new ibl_layered());
  h->g = g; h->imax = imax; h->max_batch = max_batch; h->alpha = alpha; h->beta = beta; h->llr_max = llr_max;
  h->fused = 0;
  h->wide = wide;
  h->layer_slot = pl.layer_slot;
  const LayeredPassBytes by = pass_bytes(g->n_v, g->n_c, max_batch, wide);
  if (wide && (rc = h->PO.alloc(by.state / 4))) return rc;
  if ((rc = h->rec.upload(pl.rec)) || (rc = h->P.alloc(by.P / 4)) || (rc = h->M1.alloc(by.state / 4)) ||
      (rc = h->M2.alloc(by.state / 4)) || (rc = h->PS.alloc(by.state / 4)) || (rc = h->done.alloc(by.mask / 8)) ||
      (rc = h->unsat.alloc(by.mask / 8)) || (rc = h->running.alloc(1)) || (rc = h->bits.alloc(by.bits / 8)))
    return rc;
  if (const char* v = getenv("IBL_LAY_SYNDROME")) {
    if (!strcmp(v, "gather")) h->syn_packed = 0;
    else if (strcmp(v, "packed")) return fail(IBL_EINVAL, "IBL_LAY_SYNDROME must be gather or packed");
  }
  *out = h.release();
  return IBL_OK;
}

int layered_decode_passes(ibl_layered* h, const float* d_llr, int32_t B, float* d_out, int32_t early_stop,
                          int32_t* d_iters, hipStream_t s) {
  const ibl_graph* g = h->g;
  LayPassArgs a{};
  a.P = h->P; a.M1 = h->M1; a.M2 = h->M2; a.PS = h->PS; a.done = h->done; a.unsat = h->unsat;
  a.running = h->running; a.bits = h->bits; a.rec = h->rec; a.cols = g->csr_cols; a.iters = d_iters;
  a.alpha = h->alpha; a.beta = h->beta; a.llr_max = h->llr_max;
  a.n_v = g->n_v; a.n_c = g->n_c; a.B = B; a.ntiles = pass_tiles(B);
  const int32_t every = h->compact_every;
  LayCompactArgs c{};
  c.orig = h->orig; c.dest = h->dest; c.ctl = h->ctl; c.out = d_out; c.min_free_pct = h->compact_pct;
  h->last_B = B;
  h->last_compact = every > 0;
  // h->PO is allocated on a wide handle only: with it the stage-in, the layers and the row move run in their wide
  // forms, in the same chain
  HIPCHK(launch_lay_stage_in(a, every ? &c : nullptr, h->PO, d_llr, h->imax, s));
  const int32_t n_layers = (int32_t)h->layer_slot.size() - 1;
  for (int32_t it = 1; it <= h->imax; ++it) {
    for (int32_t l = 0; l < n_layers; ++l) {
      const int32_t s0 = h->layer_slot[l], n = h->layer_slot[l + 1] - s0;
      HIPCHK(launch_lay_layer(a, h->PO, s0, n, s));
    }
    if (early_stop && it < h->imax) {
      HIPCHK(launch_lay_syndrome(a, h->syn_packed, s));
      if (every) HIPCHK(launch_lay_finalise_c(a, c, it, s));
      else HIPCHK(launch_lay_finalise(a, it, s));
      // the device decides whether the attempt moves anything (layered_plan.h compact_wanted)
      if (every && it % every == 0) HIPCHK(launch_lay_compact(a, c, h->PO, s));
    }
  }
  if (every) HIPCHK(launch_lay_stage_out_c(a, c, s));
  else HIPCHK(launch_lay_stage_out(a, d_out, s));
  return IBL_OK;
}

int layered_run_fixed(ibl_layered* h, const void* d_llr, int32_t llr_dtype, int32_t B, void* d_out, int32_t out_dtype,
                      int32_t early_stop, int32_t* d_iters, hipStream_t s) {
  const ibl_graph* g = h->g;
  LayFixArgs a{};
  a.P = h->P8; a.S = h->S; a.done = h->done; a.unsat = h->unsat; a.running = h->running; a.bits = h->bits;
  a.rec = h->rec; a.cols = g->csr_cols; a.iters = d_iters;
  a.alpha16 = h->alpha16; a.beta_q = h->beta_q; a.q_max = h->q_max; a.scale = h->scale;
  a.n_v = g->n_v; a.n_c = g->n_c; a.B = B; a.ntiles = pass_tiles(B); a.ntiles4 = fix_tiles(B);
  // h->S1 is allocated on a wide handle only
  HIPCHK(launch_layfix_stage_in(a, h->S1, d_llr, llr_dtype, h->imax, s));
  const int32_t n_layers = (int32_t)h->layer_slot.size() - 1;
  for (int32_t it = 1; it <= h->imax; ++it) {
    for (int32_t l = 0; l < n_layers; ++l) {
      const int32_t s0 = h->layer_slot[l], n = h->layer_slot[l + 1] - s0;
      HIPCHK(launch_layfix_layer(a, h->S1, s0, n, s));
    }
    if (early_stop && it < h->imax) HIPCHK(launch_layfix_stop(a, it, s));
  }
  HIPCHK(launch_layfix_stage_out(a, d_out, out_dtype, s));
  return IBL_OK;
}

// Layered BP, per-layer path: the min-sum chain with the BP stage-in and layer kernels; the first iteration's layers
// take R = 0 without reading it.
int layered_run_bp_passes(ibl_layered* h, const float* d_llr, int32_t B, float* d_out, int32_t early_stop,
                          int32_t* d_iters, hipStream_t s) {
  const ibl_graph* g = h->g;
  LayPassArgs a{};
  // M1 is R. M2 and PS repeat it only because the shared launchers (launch_lay_syndrome, _finalise, _stage_out)
  // refuse null state pointers; their kernels read none of the three. A shared kernel that starts to touch M2 or PS
  // must stop serving this handle (layered_kernels.hip is not changed by this decoder, so its check stands).
  a.P = h->P; a.M1 = h->R; a.M2 = h->R; a.PS = reinterpret_cast<uint32_t*>(h->R.get());
  a.done = h->done; a.unsat = h->unsat; a.running = h->running; a.bits = h->bits; a.rec = h->rec;
  a.cols = g->csr_cols; a.iters = d_iters;
  a.alpha = 1.f; a.beta = 0.f; a.llr_max = h->llr_max;
  a.n_v = g->n_v; a.n_c = g->n_c; a.B = B; a.ntiles = pass_tiles(B);
  h->last_B = B;
  h->last_compact = 0;
  HIPCHK(launch_laybp_stage_in(a, d_llr, h->imax, s));
  const int32_t n_layers = (int32_t)h->layer_slot.size() - 1;
  for (int32_t it = 1; it <= h->imax; ++it) {
    for (int32_t l = 0; l < n_layers; ++l) {
      const int32_t s0 = h->layer_slot[l], n = h->layer_slot[l + 1] - s0;
      HIPCHK(launch_laybp_layer(a, it == 1, s0, n, s));
    }
    if (early_stop && it < h->imax) {
      HIPCHK(launch_lay_syndrome(a, 1, s));
      HIPCHK(launch_lay_finalise(a, it, s));
    }
  }
  HIPCHK(launch_lay_stage_out(a, d_out, s));
  return IBL_OK;
}

// transpose, the fused kernel, transpose
int layered_run_bp_fused(ibl_layered* h, const float* d_llr, int32_t B, float* d_out, int32_t early_stop,
                         int32_t* d_iters, hipStream_t s) {
  const ibl_graph* g = h->g;
  HIPCHK(launch_lay_transpose(d_llr, h->buf, g->n_v, B, s));
  LayeredArgs a{};
  a.buf = h->buf; a.task = h->task; a.idx = h->idx; a.iters = d_iters;
  a.alpha = 1.f; a.beta = 0.f; a.llr_max = h->llr_max;
  a.n_v = g->n_v; a.n_c = g->n_c; a.n_tasks = h->n_tasks; a.B = B; a.imax = h->imax;
  a.early = early_stop ? 1 : 0;
  a.cw_per_group = h->cw_per_group; a.cw_bytes = (int32_t)h->cw_bytes;
  int32_t grid = 0;
  layered_geometry(h, B, &a.ngroups, &grid);
  HIPCHK(launch_laybp_fused(a, grid, (size_t)h->cw_per_group * h->cw_bytes, s));
  HIPCHK(launch_lay_transpose(h->buf, d_out, B, g->n_v, s));
  return IBL_OK;
}

// Layered BP, half state, per-layer path: layered_run_bp_passes' chain with the half kernels and their own pack
int layered_run_half_passes(ibl_layered* h, const float* d_llr, int32_t B, float* d_out, int32_t early_stop,
                            int32_t* d_iters, hipStream_t s) {
  const ibl_graph* g = h->g;
  LayHalfArgs a{};
  a.P = h->P16; a.R = h->R16; a.done = h->done; a.unsat = h->unsat; a.running = h->running; a.bits = h->bits;
  a.rec = h->rec; a.cols = g->csr_cols; a.iters = d_iters; a.llr_max = h->llr_max;
  a.n_v = g->n_v; a.n_c = g->n_c; a.B = B; a.ntiles = pass_tiles(B); a.ntiles2 = half_tiles(B);
  h->last_B = B;
  h->last_compact = 0;
  HIPCHK(launch_layhp_stage_in(a, d_llr, h->imax, s));
  const int32_t n_layers = (int32_t)h->layer_slot.size() - 1;
  for (int32_t it = 1; it <= h->imax; ++it) {
    for (int32_t l = 0; l < n_layers; ++l) {
      const int32_t s0 = h->layer_slot[l], n = h->layer_slot[l + 1] - s0;
      HIPCHK(launch_layhp_layer(a, it == 1, s0, n, s));
    }
    if (early_stop && it < h->imax) HIPCHK(launch_layhp_stop(a, it, s));
  }
  HIPCHK(launch_layhp_stage_out(a, d_out, s));
  return IBL_OK;
}

// transpose, the fused kernel (which converts as it stages a row in and out), transpose
int layered_run_half_fused(ibl_layered* h, const float* d_llr, int32_t B, float* d_out, int32_t early_stop,
                           int32_t* d_iters, hipStream_t s) {
  const ibl_graph* g = h->g;
  HIPCHK(launch_lay_transpose(d_llr, h->buf, g->n_v, B, s));
  LayeredArgs a{};
  a.buf = h->buf; a.task = h->task; a.idx = h->idx; a.iters = d_iters;
  a.alpha = 1.f; a.beta = 0.f; a.llr_max = h->llr_max;
  a.n_v = g->n_v; a.n_c = g->n_c; a.n_tasks = h->n_tasks; a.B = B; a.imax = h->imax;
  a.early = early_stop ? 1 : 0;
  a.cw_per_group = h->cw_per_group; a.cw_bytes = (int32_t)h->cw_bytes;
  int32_t grid = 0;
  layered_geometry(h, B, &a.ngroups, &grid);
  HIPCHK(launch_layhp_fused(a, grid, (size_t)h->cw_per_group * h->cw_bytes, s));
  HIPCHK(launch_lay_transpose(h->buf, d_out, B, g->n_v, s));
  return IBL_OK;
}

// stage-in, the fused kernel, stage-out: three launches at any imax
int layered_run_fixed_fused(ibl_layered* h, const void* d_llr, int32_t llr_dtype, int32_t B, void* d_out,
                            int32_t out_dtype, int32_t early_stop, int32_t* d_iters, hipStream_t s) {
  const ibl_graph* g = h->g;
  HIPCHK(launch_layfix_fused_stage_in(d_llr, llr_dtype, h->buf8, g->n_v, B, h->scale, s));
  LayFixFusedArgs a{};
  a.buf = h->buf8; a.task = h->task; a.idx = h->idx; a.iters = d_iters;
  a.alpha16 = h->alpha16; a.beta_q = h->beta_q; a.q_max = h->q_max;
  a.n_v = g->n_v; a.ldn = fixfused_ldn(g->n_v); a.n_c = g->n_c; a.n_tasks = h->n_tasks; a.B = B; a.imax = h->imax;
  a.early = early_stop ? 1 : 0;
  a.cw_per_group = h->cw_per_group; a.cw_bytes = (int32_t)h->cw_bytes;
  int32_t grid = 0;
  layered_geometry(h, B, &a.ngroups, &grid);
  HIPCHK(launch_layfix_fused(a, h->wide != 0, grid, (size_t)h->cw_per_group * h->cw_bytes, s));
  HIPCHK(launch_layfix_fused_stage_out(h->buf8, d_out, out_dtype, g->n_v, B, h->scale, s));
  return IBL_OK;
}
}  // namespace

extern "C" {

int ibl_layers_validate(int32_t n_v, int32_t n_c, const int32_t* indptr, const int32_t* cols, int32_t n_layers,
                        const int32_t* layer_ptr, const int32_t* layer_checks) {
  std::string err;
  const int rc = validate_layers(n_v, n_c, indptr, cols, n_layers, layer_ptr, layer_checks, &err);
  if (rc) return fail(rc == -2 ? IBL_EUNSUPPORTED : IBL_EINVAL, err);
  return IBL_OK;
}

int ibl_layered_create(const ibl_graph* g, int32_t n_layers, const int32_t* layer_ptr, const int32_t* layer_checks,
                       int32_t imax, float alpha, float beta, float llr_max, int32_t precision, int32_t max_batch,
                       ibl_layered** out) {
  return ibl_layered_create_path(g, n_layers, layer_ptr, layer_checks, imax, alpha, beta, llr_max, precision,
                                 max_batch, IBL_PATH_FUSED, out);
}

int ibl_layered_create_path(const ibl_graph* g, int32_t n_layers, const int32_t* layer_ptr,
                            const int32_t* layer_checks, int32_t imax, float alpha, float beta, float llr_max,
                            int32_t precision, int32_t max_batch, int32_t path, ibl_layered** out) {
  if (!out) return fail(IBL_EINVAL, "out is NULL");
  *out = nullptr;
  if (!g) return fail(IBL_EINVAL, "graph is NULL");
  if (precision == kF64) return fail(IBL_EUNSUPPORTED, "the layered decoder is fp32 only (fp64 is not built)");
  if (precision != kF32) return fail(IBL_EINVAL, "precision must be IBL_F32");
  if (imax < 1 || max_batch < 1) return fail(IBL_EINVAL, "imax and max_batch must be >= 1");
  if (!(alpha >= 0.f) || !(beta >= 0.f) || !(llr_max > 0.f) || std::isinf(alpha) || std::isinf(beta))
    return fail(IBL_EINVAL, "alpha and beta must be finite and >= 0, llr_max > 0");
  if (int rc = check_path(path)) return rc;
  const std::vector<int32_t> ip = graph_indptr(g);
  int rc = ibl_layers_validate(g->n_v, g->n_c, ip.data(), g->h_cols.data(), n_layers, layer_ptr, layer_checks);
  if (rc) return rc;
  const bool wide = layered_is_wide(g->n_c, ip.data());
  if (path == IBL_PATH_PASSES || (path == IBL_PATH_AUTO && layered_cw_per_group(g->n_v, g->n_c, wide) < 1))
    return layered_create_passes(g, ip, n_layers, layer_ptr, layer_checks, imax, alpha, beta, llr_max, max_batch, out);
  LayeredPlan pl;
  plan_layered(g->n_v, g->n_c, ip.data(), g->h_cols.data(), n_layers, layer_ptr, layer_checks, &pl);
  if (pl.cw_per_group < 1)
    return fail(IBL_EUNSUPPORTED, std::string("code does not fit the layered kernel: one codeword needs ") +
                                      (wide ? "4 N + 16 n_c = " : "4 N + 12 n_c = ") + std::to_string(pl.cw_bytes) +
                                      " bytes of LDS, a workgroup has " + std::to_string(kLayLds));
  HIPCHK(hipSetDevice(g->device));
  std::unique_ptr<ibl_layered> h(new ibl_layered());
  h->g = g; h->imax = imax; h->max_batch = max_batch; h->alpha = alpha; h->beta = beta; h->llr_max = llr_max;
  h->n_tasks = pl.n_tasks; h->cw_per_group = pl.cw_per_group; h->cw_bytes = pl.cw_bytes;
  h->wide = wide;
  if ((rc = h->task.upload(pl.task)) || (rc = h->idx.upload(pl.idx)) ||
      (rc = h->buf.alloc((size_t)max_batch * (size_t)g->n_v)))
    return rc;
  int bpc = 0;
  size_t priv = 0;
  const size_t lds = (size_t)h->cw_per_group * h->cw_bytes;
  const hipError_t e = lay_fused_occupancy(wide, h->cw_per_group, lds, &bpc, &priv);
  if (e != hipSuccess) return fail(IBL_EHIP, std::string("layered kernel occupancy: ") + hipGetErrorString(e));
  if (bpc < 1) return fail(IBL_EHIP, "no occupancy for the layered kernel");
  // same guard as the other fused kernels: built to run without scratch
  if ((rc = refuse_private(priv, "layered kernel has a ", "-byte private segment (register spill): rebuild required")))
    return rc;
  h->bpc = bpc;
  *out = h.release();
  return IBL_OK;
}

int ibl_layered_create_fixed(const ibl_graph* g, int32_t n_layers, const int32_t* layer_ptr,
                             const int32_t* layer_checks, int32_t imax, int32_t alpha16, int32_t beta_q, int32_t q_max,
                             float scale, int32_t max_batch, int32_t path, ibl_layered** out) {
  if (!out) return fail(IBL_EINVAL, "out is NULL");
  *out = nullptr;
  if (imax < 1 || max_batch < 1) return fail(IBL_EINVAL, "imax and max_batch must be >= 1");
  if (!fix_params_ok(alpha16, beta_q, q_max))
    return fail(IBL_EINVAL, "alpha16 must lie in [0, 16], beta_q in [0, 63], q_max in [1, 63]");
  if (!(scale > 0.f) || std::isinf(scale)) return fail(IBL_EINVAL, "scale must be finite and > 0");
  if (int rc = check_path(path)) return rc;
  if (path == IBL_PATH_FUSED)
    return fail(IBL_EUNSUPPORTED, "the fixed-point fused kernel is not built: use IBL_PATH_PASSES or IBL_PATH_AUTO");
  if (!g) return fail(IBL_EINVAL, "graph is NULL");
  const std::vector<int32_t> ip = graph_indptr(g);
  int rc = ibl_layers_validate(g->n_v, g->n_c, ip.data(), g->h_cols.data(), n_layers, layer_ptr, layer_checks);
  if (rc) return rc;
  LayeredPassPlan pl;
  plan_layered_passes(g->n_c, ip.data(), n_layers, layer_ptr, layer_checks, &pl);
  const int64_t rows = std::max(g->n_v, g->n_c);
  if (fix_grid(pl.max_layer, max_batch) > 0x7fffffffll ||
      pass_grid(pass_pack_runs((int32_t)rows), max_batch) > 0x7fffffffll ||
      (rows * fix_tiles(max_batch) + kLayPassWaves - 1) / kLayPassWaves > 0x7fffffffll)
    return fail(IBL_EINVAL, "max_batch is too large for the per-layer kernels' grids");
  HIPCHK(hipSetDevice(g->device));
  const bool wide = layered_is_wide(g->n_c, ip.data());
  size_t priv = 0, priv_stop = 0, priv_wide = 0;
  HIPCHK(layfix_private_bytes(&priv));
  HIPCHK(lay_pass_private_bytes(&priv_stop));   // the shared syndrome and finalise kernels
  if (wide) HIPCHK(lay_wide_private_bytes(&priv_wide));
  if ((rc = refuse_private(std::max({priv, priv_stop, priv_wide}), "a fixed-point layered kernel has a ",
                           "-byte private segment (register spill): rebuild required")))
    return rc;
  std::unique_ptr<ibl_layered> h(new ibl_layered());
  h->g = g; h->imax = imax; h->max_batch = max_batch;
  h->fused = 0; h->fixed = 1; h->wide = wide;
  h->alpha16 = alpha16; h->beta_q = beta_q; h->q_max = q_max; h->scale = scale;
  h->layer_slot = pl.layer_slot;
  // a wide handle's two state arrays are allocations of their own, by.state bytes together
  const LayeredFixBytes by = fix_bytes(g->n_v, g->n_c, max_batch, wide);
  const size_t s_words = by.state / (wide ? 8 : 4);
  if (wide && (rc = h->S1.alloc(s_words))) return rc;
  if ((rc = h->rec.upload(pl.rec)) || (rc = h->P8.alloc(by.P)) || (rc = h->S.alloc(s_words)) ||
      (rc = h->done.alloc(by.mask / 8)) || (rc = h->unsat.alloc(by.mask / 8)) || (rc = h->running.alloc(1)) ||
      (rc = h->bits.alloc(by.bits / 8)))
    return rc;
  *out = h.release();
  return IBL_OK;
}

int ibl_layered_create_fixed_fused(const ibl_graph* g, int32_t n_layers, const int32_t* layer_ptr,
                                   const int32_t* layer_checks, int32_t imax, int32_t alpha16, int32_t beta_q,
                                   int32_t q_max, float scale, int32_t max_batch, ibl_layered** out) {
  if (!out) return fail(IBL_EINVAL, "out is NULL");
  *out = nullptr;
  if (imax < 1 || max_batch < 1) return fail(IBL_EINVAL, "imax and max_batch must be >= 1");
  if (!fix_params_ok(alpha16, beta_q, q_max))
    return fail(IBL_EINVAL, "alpha16 must lie in [0, 16], beta_q in [0, 63], q_max in [1, 63]");
  if (!(scale > 0.f) || std::isinf(scale)) return fail(IBL_EINVAL, "scale must be finite and > 0");
  if (!g) return fail(IBL_EINVAL, "graph is NULL");
  const std::vector<int32_t> ip = graph_indptr(g);
  int rc = ibl_layers_validate(g->n_v, g->n_c, ip.data(), g->h_cols.data(), n_layers, layer_ptr, layer_checks);
  if (rc) return rc;
  const bool wide = layered_is_wide(g->n_c, ip.data());
  // IBL_LAYFIX_FUSED_CW=1..16 replaces the cap on the codewords of a workgroup (DESIGN.md "Layered min-sum: fixed
  // point, fused" for the numbers); read at create
  int32_t cap = kLayFixFusedMaxCw;
  if (const char* v = getenv("IBL_LAYFIX_FUSED_CW")) {
    cap = atoi(v);
    if (cap < 1 || cap > kLayFixFusedBoundCw) return fail(IBL_EINVAL, "IBL_LAYFIX_FUSED_CW must lie in [1, 16]");
  }
  const size_t cw_bytes = fixfused_cw_bytes(g->n_v, g->n_c, wide);
  const int32_t cw = fixfused_cw_per_group(g->n_v, g->n_c, wide, cap);
  if (cw < 1)
    return fail(IBL_EUNSUPPORTED, std::string("code does not fit the fixed-point fused kernel: one codeword needs "
                                              "cw_bytes = ") + (wide ? "N + 8 n_c = " : "N + 4 n_c = ") +
                                      std::to_string(cw_bytes) + " bytes of LDS, a workgroup has " +
                                      std::to_string(kLayLds) + " (160 KiB): use ibl_layered_create_fixed");
  if (fixfused_stage_tiles(g->n_v, max_batch) > 0x7fffffffll)
    return fail(IBL_EINVAL, "max_batch is too large for the staging kernels' grid");
  LayeredPlan pl;
  plan_layered(g->n_v, g->n_c, ip.data(), g->h_cols.data(), n_layers, layer_ptr, layer_checks, &pl);
  HIPCHK(hipSetDevice(g->device));
  std::unique_ptr<ibl_layered> h(new ibl_layered());
  h->g = g; h->imax = imax; h->max_batch = max_batch;
  h->fused = 1; h->fixed = 1; h->wide = wide;
  h->alpha16 = alpha16; h->beta_q = beta_q; h->q_max = q_max; h->scale = scale;
  h->n_tasks = pl.n_tasks; h->cw_per_group = cw; h->cw_bytes = cw_bytes;
  if ((rc = h->task.upload(pl.task)) || (rc = h->idx.upload(pl.idx)) ||
      (rc = h->buf8.alloc(fixfused_buf_bytes(g->n_v, max_batch))))
    return rc;
  int bpc = 0;
  size_t priv = 0;
  const hipError_t e = layfix_fused_occupancy(wide, cw, (size_t)cw * cw_bytes, &bpc, &priv);
  if (e != hipSuccess)
    return fail(IBL_EHIP, std::string("fixed-point fused kernel occupancy: ") + hipGetErrorString(e));
  if (bpc < 1) return fail(IBL_EHIP, "no occupancy for the fixed-point fused kernel");
  if ((rc = refuse_private(priv, "a fixed-point fused layered kernel has a ",
                           "-byte private segment (register spill): rebuild required")))
    return rc;
  h->bpc = bpc;
  *out = h.release();
  return IBL_OK;
}

int ibl_layered_create_bp(const ibl_graph* g, int32_t n_layers, const int32_t* layer_ptr, const int32_t* layer_checks,
                          int32_t imax, float llr_max, int32_t precision, int32_t max_batch, int32_t path,
                          ibl_layered** out) {
  if (!out) return fail(IBL_EINVAL, "out is NULL");
  *out = nullptr;
  if (!g) return fail(IBL_EINVAL, "graph is NULL");
  if (precision == kF64) return fail(IBL_EUNSUPPORTED, "the layered BP decoder is fp32 only (fp64 is not built)");
  if (precision != kF32) return fail(IBL_EINVAL, "precision must be IBL_F32");
  if (imax < 1 || max_batch < 1) return fail(IBL_EINVAL, "imax and max_batch must be >= 1");
  if (!(llr_max > 0.f) || std::isinf(llr_max)) return fail(IBL_EINVAL, "llr_max must be finite and > 0");
  if (int rc = check_path(path)) return rc;
  const std::vector<int32_t> ip = graph_indptr(g);
  int rc = ibl_layers_validate(g->n_v, g->n_c, ip.data(), g->h_cols.data(), n_layers, layer_ptr, layer_checks);
  if (rc) return rc;
  const int32_t bad = laybp_unsupported_check(g->n_c, ip.data());
  if (bad >= 0)
    return fail(IBL_EUNSUPPORTED, "check " + std::to_string(bad) + " has degree " +
                                      std::to_string(ip[(size_t)bad + 1] - ip[bad]) +
                                      ": layered BP supports check degrees 2..16");
  const int64_t n_e = ip[(size_t)g->n_c];
  const int32_t cw = laybp_cw_per_group(g->n_v, n_e);
  HIPCHK(hipSetDevice(g->device));
  if (path == IBL_PATH_PASSES || (path == IBL_PATH_AUTO && cw < 1)) {
    LayeredPassPlan pl;
    plan_layered_passes(g->n_c, ip.data(), n_layers, layer_ptr, layer_checks, &pl);
    if (pass_grid(pl.max_layer, max_batch) > 0x7fffffffll ||
        pass_grid(pass_pack_runs(std::max(g->n_v, g->n_c)), max_batch) > 0x7fffffffll ||
        ((int64_t)g->n_v * pass_tiles(max_batch) + kLayPassWaves - 1) / kLayPassWaves > 0x7fffffffll)
      return fail(IBL_EINVAL, "max_batch is too large for the per-layer kernels' grids");
    size_t priv = 0, priv_shared = 0;
    HIPCHK(laybp_pass_private_bytes(&priv));
    HIPCHK(lay_pass_private_bytes(&priv_shared));   // the shared pack, syndrome, finalise and stage-out kernels
    if ((rc = refuse_private(std::max(priv, priv_shared), "a per-layer layered BP kernel has a ",
                             "-byte private segment (register spill): rebuild required")))
      return rc;
    std::unique_ptr<ibl_layered> h(new ibl_layered());
    h->g = g; h->imax = imax; h->max_batch = max_batch; h->llr_max = llr_max;
    h->fused = 0; h->bp = 1;
    h->layer_slot = pl.layer_slot;
    const LayeredBpBytes by = laybp_pass_bytes(g->n_v, n_e, max_batch);
    if ((rc = h->rec.upload(pl.rec)) || (rc = h->P.alloc(by.P / 4)) || (rc = h->R.alloc(by.R / 4)) ||
        (rc = h->done.alloc(by.mask / 8)) || (rc = h->unsat.alloc(by.mask / 8)) || (rc = h->running.alloc(1)) ||
        (rc = h->bits.alloc(by.bits / 8)))
      return rc;
    *out = h.release();
    return IBL_OK;
  }
  if (cw < 1)
    return fail(IBL_EUNSUPPORTED, "code does not fit the layered BP kernel: one codeword needs 4 N + 4 E = " +
                                      std::to_string(laybp_cw_bytes(g->n_v, n_e)) + " bytes of LDS, a workgroup has " +
                                      std::to_string(kLayLds));
  LayeredBpPlan pl;
  plan_layered_bp(g->n_v, g->n_c, ip.data(), g->h_cols.data(), n_layers, layer_ptr, layer_checks, &pl);
  std::unique_ptr<ibl_layered> h(new ibl_layered());
  h->g = g; h->imax = imax; h->max_batch = max_batch; h->llr_max = llr_max;
  h->fused = 1; h->bp = 1;
  h->n_tasks = pl.n_tasks; h->cw_per_group = pl.cw_per_group; h->cw_bytes = pl.cw_bytes;
  if ((rc = h->task.upload(pl.task)) || (rc = h->idx.upload(pl.idx)) ||
      (rc = h->buf.alloc((size_t)max_batch * (size_t)g->n_v)))
    return rc;
  int bpc = 0;
  size_t priv = 0;
  const hipError_t e = laybp_fused_occupancy(h->cw_per_group, (size_t)h->cw_per_group * h->cw_bytes, &bpc, &priv);
  if (e != hipSuccess) return fail(IBL_EHIP, std::string("layered BP kernel occupancy: ") + hipGetErrorString(e));
  if (bpc < 1) return fail(IBL_EHIP, "no occupancy for the layered BP kernel");
  if ((rc = refuse_private(priv, "the layered BP kernel has a ",
                           "-byte private segment (register spill): rebuild required")))
    return rc;
  h->bpc = bpc;
  *out = h.release();
  return IBL_OK;
}

int ibl_layered_create_bp_half(const ibl_graph* g, int32_t n_layers, const int32_t* layer_ptr,
                               const int32_t* layer_checks, int32_t imax, float llr_max, int32_t max_batch,
                               int32_t path, ibl_layered** out) {
  if (!out) return fail(IBL_EINVAL, "out is NULL");
  *out = nullptr;
  if (!g) return fail(IBL_EINVAL, "graph is NULL");
  if (imax < 1 || max_batch < 1) return fail(IBL_EINVAL, "imax and max_batch must be >= 1");
  if (!(llr_max > 0.f) || std::isinf(llr_max)) return fail(IBL_EINVAL, "llr_max must be finite and > 0");
  if (int rc = check_path(path)) return rc;
  const std::vector<int32_t> ip = graph_indptr(g);
  int rc = ibl_layers_validate(g->n_v, g->n_c, ip.data(), g->h_cols.data(), n_layers, layer_ptr, layer_checks);
  if (rc) return rc;
  const int32_t bad = laybp_unsupported_check(g->n_c, ip.data());
  if (bad >= 0)
    return fail(IBL_EUNSUPPORTED, "check " + std::to_string(bad) + " has degree " +
                                      std::to_string(ip[(size_t)bad + 1] - ip[bad]) +
                                      ": layered BP supports check degrees 2..16");
  const int64_t n_e = ip[(size_t)g->n_c];
  const int32_t cw = layhp_cw_per_group(g->n_v, n_e);
  HIPCHK(hipSetDevice(g->device));
  if (path == IBL_PATH_PASSES || (path == IBL_PATH_AUTO && cw < 1)) {
    LayeredPassPlan pl;
    plan_layered_passes(g->n_c, ip.data(), n_layers, layer_ptr, layer_checks, &pl);
    if (half_grid(pl.max_layer, max_batch) > 0x7fffffffll ||
        pass_grid(pass_pack_runs(std::max(g->n_v, g->n_c)), max_batch) > 0x7fffffffll ||
        ((int64_t)g->n_v * half_tiles(max_batch) + kLayPassWaves - 1) / kLayPassWaves > 0x7fffffffll)
      return fail(IBL_EINVAL, "max_batch is too large for the per-layer kernels' grids");
    size_t priv = 0, priv_shared = 0;
    HIPCHK(layhp_pass_private_bytes(&priv));
    HIPCHK(lay_pass_private_bytes(&priv_shared));   // the shared syndrome and finalise kernels
    if ((rc = refuse_private(std::max(priv, priv_shared), "a per-layer half-state layered BP kernel has a ",
                             "-byte private segment (register spill): rebuild required")))
      return rc;
    std::unique_ptr<ibl_layered> h(new ibl_layered());
    h->g = g; h->imax = imax; h->max_batch = max_batch; h->llr_max = llr_max;
    h->fused = 0; h->bp = 1; h->half = 1;
    h->layer_slot = pl.layer_slot;
    const LayeredBpBytes by = layhp_pass_bytes(g->n_v, n_e, max_batch);
    if ((rc = h->rec.upload(pl.rec)) || (rc = h->P16.alloc(by.P / 2)) || (rc = h->R16.alloc(by.R / 2)) ||
        (rc = h->done.alloc(by.mask / 8)) || (rc = h->unsat.alloc(by.mask / 8)) || (rc = h->running.alloc(1)) ||
        (rc = h->bits.alloc(by.bits / 8)))
      return rc;
    *out = h.release();
    return IBL_OK;
  }
  if (cw < 1)
    return fail(IBL_EUNSUPPORTED, "code does not fit the half-state layered BP kernel: one codeword needs 2 N + 2 E = " +
                                      std::to_string(layhp_cw_bytes(g->n_v, n_e)) + " bytes of LDS, a workgroup has " +
                                      std::to_string(kLayLds));
  LayeredBpPlan pl;
  plan_layered_bp_half(g->n_v, g->n_c, ip.data(), g->h_cols.data(), n_layers, layer_ptr, layer_checks, &pl);
  std::unique_ptr<ibl_layered> h(new ibl_layered());
  h->g = g; h->imax = imax; h->max_batch = max_batch; h->llr_max = llr_max;
  h->fused = 1; h->bp = 1; h->half = 1;
  h->n_tasks = pl.n_tasks; h->cw_per_group = pl.cw_per_group; h->cw_bytes = pl.cw_bytes;
  if ((rc = h->task.upload(pl.task)) || (rc = h->idx.upload(pl.idx)) ||
      (rc = h->buf.alloc((size_t)max_batch * (size_t)g->n_v)))
    return rc;
  int bpc = 0;
  size_t priv = 0;
  const hipError_t e = layhp_fused_occupancy(h->cw_per_group, (size_t)h->cw_per_group * h->cw_bytes, &bpc, &priv);
  if (e != hipSuccess)
    return fail(IBL_EHIP, std::string("half-state layered BP kernel occupancy: ") + hipGetErrorString(e));
  if (bpc < 1) return fail(IBL_EHIP, "no occupancy for the half-state layered BP kernel");
  if ((rc = refuse_private(priv, "the half-state layered BP kernel has a ",
                           "-byte private segment (register spill): rebuild required")))
    return rc;
  h->bpc = bpc;
  *out = h.release();
  return IBL_OK;
}

int ibl_layered_is_half(const ibl_layered* h, int32_t* half) {
  if (!h || !half) return fail(IBL_EINVAL, "NULL argument");
  *half = h->half;
  return IBL_OK;
}

int ibl_layered_is_bp(const ibl_layered* h, int32_t* bp) {
  if (!h || !bp) return fail(IBL_EINVAL, "NULL argument");
  *bp = h->bp;
  return IBL_OK;
}

int ibl_layered_is_fixed(const ibl_layered* h, int32_t* fixed) {
  if (!h || !fixed) return fail(IBL_EINVAL, "NULL argument");
  *fixed = h->fixed;
  return IBL_OK;
}

int ibl_layered_is_wide(const ibl_layered* h, int32_t* wide) {
  if (!h || !wide) return fail(IBL_EINVAL, "NULL argument");
  *wide = h->wide;
  return IBL_OK;
}

int ibl_layered_set_compaction(ibl_layered* h, int32_t every, int32_t min_free_pct) {
  // the numbers are judged before the handle, so these refusals need no device
  if (every < 0 || (every > 0 && (min_free_pct < 1 || min_free_pct > 100)))
    return fail(IBL_EINVAL, "every must be >= 0 (0: off) and min_free_pct lie in [1, 100]");
  if (!h) return fail(IBL_EINVAL, "decoder is NULL");
  if (h->bp) return fail(IBL_EUNSUPPORTED, "compaction is not built for the BP decoder");
  if (h->fixed) return fail(IBL_EUNSUPPORTED, "compaction is not built for the fixed-point decoder");
  if (h->fused) return fail(IBL_EUNSUPPORTED, "compaction needs the per-layer path");
  if (every == 0) {
    h->compact_every = h->compact_pct = 0;
    return IBL_OK;
  }
  if (!h->ctl) {
    if ((pass_compact_rows(h->g->n_v, h->g->n_c, h->wide != 0) + kLayPassWaves - 1) / kLayPassWaves > 0x7fffffffll)
      return fail(IBL_EINVAL, "the code is too large for the compaction kernels' grid");
    HIPCHK(hipSetDevice(h->g->device));
    size_t priv = 0;
    HIPCHK(lay_compact_private_bytes(&priv));
    int rc = refuse_private(priv, "a compaction kernel has a ", "-byte private segment (register spill): rebuild required");
    if (rc) return rc;
    const LayeredCompactBytes by = pass_compact_bytes(h->max_batch);
    DevBuf<int32_t> orig, dest, ctl;
    if ((rc = orig.alloc(by.orig / 4)) || (rc = dest.alloc(by.dest / 4)) || (rc = ctl.alloc_zero(by.ctl / 4))) return rc;
    h->orig = std::move(orig); h->dest = std::move(dest); h->ctl = std::move(ctl);
  }
  h->compact_every = every;
  h->compact_pct = min_free_pct;
  return IBL_OK;
}

int ibl_layered_compaction_stats(const ibl_layered* h, void* stream, int32_t* compactions, int32_t* extent) {
  if (!h || !compactions || !extent) return fail(IBL_EINVAL, "NULL argument");
  if (h->bp) return fail(IBL_EUNSUPPORTED, "compaction is not built for the BP decoder");
  if (h->fixed) return fail(IBL_EUNSUPPORTED, "compaction is not built for the fixed-point decoder");
  if (h->fused) return fail(IBL_EUNSUPPORTED, "compaction needs the per-layer path");
  *compactions = 0;
  *extent = h->last_B;   // a decode without compaction keeps all its columns
  if (!h->last_compact) return IBL_OK;
  int32_t w[kLayCompactCtl] = {0, 0, 0, 0};
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipSetDevice(h->g->device));
  HIPCHK(hipMemcpyAsync(w, h->ctl.get(), sizeof(w), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *compactions = w[kLayCtlCount];
  *extent = w[kLayCtlExtent];
  return IBL_OK;
}

int ibl_layered_geometry(const ibl_layered* h, int32_t B, int32_t* cw_per_group, int32_t* ngroups, int32_t* grid) {
  if (!h || !cw_per_group || !ngroups || !grid) return fail(IBL_EINVAL, "NULL argument");
  if (B < 1 || B > h->max_batch) return fail(IBL_EINVAL, "B must lie in [1, max_batch]");
  if (!h->fused) {
    *cw_per_group = *ngroups = *grid = 0;
    return IBL_OK;
  }
  *cw_per_group = h->cw_per_group;
  layered_geometry(h, B, ngroups, grid);
  return IBL_OK;
}

int ibl_layered_path_in_use(const ibl_layered* h, int32_t* fused) {
  if (!h || !fused) return fail(IBL_EINVAL, "NULL argument");
  *fused = h->fused;
  return IBL_OK;
}

int ibl_layered_decode(ibl_layered* h, const void* d_llr, int32_t llr_dtype, int32_t B, void* d_out,
                       int32_t out_dtype, int32_t early_stop, int32_t* d_iters, void* stream) {
  if (!h) return fail(IBL_EINVAL, "decoder is NULL");
  if (B < 1 || B > h->max_batch) return fail(IBL_EINVAL, "B must lie in [1, max_batch]");
  if (h->fixed) {
    if ((llr_dtype != kF32 && llr_dtype != kI8) || (out_dtype != kF32 && out_dtype != kI8))
      return fail(IBL_EINVAL, "LLR dtypes of a fixed-point decoder must be IBL_F32 or IBL_I8");
    if (!d_llr || !d_out) return fail(IBL_EINVAL, "NULL buffer");
    HIPCHK(hipSetDevice(h->g->device));
    if (h->fused)
      return layered_run_fixed_fused(h, d_llr, llr_dtype, B, d_out, out_dtype, early_stop, d_iters,
                                     (hipStream_t)stream);
    return layered_run_fixed(h, d_llr, llr_dtype, B, d_out, out_dtype, early_stop, d_iters, (hipStream_t)stream);
  }
  if (llr_dtype == kF64 || out_dtype == kF64) return fail(IBL_EUNSUPPORTED, "the layered decoder is fp32 only");
  if (llr_dtype != kF32 || out_dtype != kF32) return fail(IBL_EINVAL, "LLR dtypes must be IBL_F32");
  if (!d_llr || !d_out) return fail(IBL_EINVAL, "NULL buffer");
  const ibl_graph* g = h->g;
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipSetDevice(g->device));
  if (h->half)
    return (h->fused ? layered_run_half_fused : layered_run_half_passes)(
        h, static_cast<const float*>(d_llr), B, static_cast<float*>(d_out), early_stop, d_iters, s);
  if (h->bp)
    return (h->fused ? layered_run_bp_fused : layered_run_bp_passes)(
        h, static_cast<const float*>(d_llr), B, static_cast<float*>(d_out), early_stop, d_iters, s);
  if (!h->fused)
    return layered_decode_passes(h, static_cast<const float*>(d_llr), B, static_cast<float*>(d_out), early_stop,
                                 d_iters, s);
  HIPCHK(launch_lay_transpose(static_cast<const float*>(d_llr), h->buf, g->n_v, B, s));
  LayeredArgs a{};
  a.buf = h->buf; a.task = h->task; a.idx = h->idx; a.iters = d_iters;
  a.alpha = h->alpha; a.beta = h->beta; a.llr_max = h->llr_max;
  a.n_v = g->n_v; a.n_c = g->n_c; a.n_tasks = h->n_tasks; a.B = B; a.imax = h->imax;
  a.early = early_stop ? 1 : 0;
  a.cw_per_group = h->cw_per_group; a.cw_bytes = (int32_t)h->cw_bytes;
  int32_t grid = 0;
  layered_geometry(h, B, &a.ngroups, &grid);
#if IBL_DIAG
  // diagnostic builds only: IBL_TRACE_LAYERED=<file> records workgroup 0 / wave 0's clocks at every task of its
  // first codeword's second iteration (with -DIBL_LAY_TRACE=1 kernels, tools/variants.py laytrace)
  const char* ltrace = getenv("IBL_TRACE_LAYERED");
  TraceBuf tr;
  int rc;
  if (ltrace) {
    if ((rc = tr.open((size_t)3 * h->n_tasks, s))) return rc;
    a.trace = tr.d;
  }
#endif
  HIPCHK(launch_lay_fused(a, h->wide != 0, grid, (size_t)h->cw_per_group * h->cw_bytes, s));
#if IBL_DIAG
  if (ltrace && (rc = tr.save(s, ltrace, 0, tr.n))) return rc;
#endif
  HIPCHK(launch_lay_transpose(h->buf, static_cast<float*>(d_out), B, g->n_v, s));
  return IBL_OK;
}

void ibl_layered_destroy(ibl_layered* h) {
  if (h) (void)hipSetDevice(h->g->device);
  delete h;
}

}  // extern "C"
