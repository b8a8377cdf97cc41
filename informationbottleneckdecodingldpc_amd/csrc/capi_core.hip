// C ABI (include/ibldpc.h): version, last error, device count, the graph handle, and the stateless channel,
// random-bit and count entries. The decoders and the encoder have a translation unit each (capi_ib.hip,
// capi_float.hip, capi_layered.hip, capi_encoder.hip); host.h is what they share.
#include <cmath>

#include "host.h"

using namespace ibl;

int ibl::set_error(int code, const char* msg) { return fail(code, msg ? msg : ""); }

extern "C" {

int ibl_version(void) { return IBL_VERSION; }
const char* ibl_last_error(void) { return g_err.c_str(); }

int ibl_device_count(int32_t* n) {
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (n) *n = (e == hipSuccess) ? c : 0;
  return IBL_OK;
}

int ibl_map_node_connections(int32_t n_v, int32_t n_c, const int32_t* indptr, const int32_t* cols,
                             int32_t* cn_start, int32_t* cn_deg, int32_t* tgt_cn, int32_t* vn_start,
                             int32_t* vn_deg, int32_t* tgt_vn) {
  std::string err;
  if (!map_node_connections(n_v, n_c, indptr, cols, cn_start, cn_deg, tgt_cn, vn_start, vn_deg, tgt_vn, &err))
    return fail(IBL_EINVAL, err);
  return IBL_OK;
}

int ibl_graph_create(int32_t n_v, int32_t n_c, const int32_t* indptr, const int32_t* cols, int32_t device,
                     ibl_graph** out) {
  if (!out) return fail(IBL_EINVAL, "out is NULL");
  *out = nullptr;
  if (n_v <= 0 || n_c <= 0) return fail(IBL_EINVAL, "empty graph");
  const int64_t E = indptr[n_c];
  std::vector<int32_t> cs(n_c), cd(n_c), tc(E), vs(n_v), vd(n_v), tv(E);
  int rc = ibl_map_node_connections(n_v, n_c, indptr, cols, cs.data(), cd.data(), tc.data(), vs.data(), vd.data(),
                                    tv.data());
  if (rc) return rc;
  for (int32_t c = 0; c < n_c; ++c)
    if (cd[c] < 2 || cd[c] > 255) return fail(IBL_EUNSUPPORTED, "check-node degrees must lie in [2, 255]");
  for (int32_t v = 0; v < n_v; ++v)
    if (vd[v] < 1 || vd[v] > 255) return fail(IBL_EUNSUPPORTED, "variable-node degrees must lie in [1, 255]");
  HIPCHK(hipSetDevice(device));
  std::unique_ptr<ibl_graph> g(new ibl_graph());
  g->device = device;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) g->num_cus = prop.multiProcessorCount;
  g->n_v = n_v;
  g->n_c = n_c;
  g->n_e = E;
  g->dcm = *std::max_element(cd.begin(), cd.end());
  g->dvm = *std::max_element(vd.begin(), vd.end());
  g->dc_min = *std::min_element(cd.begin(), cd.end());
  g->h_cn_deg = cd;
  g->h_vn_deg = vd;
  g->h_cn_start = cs;
  g->h_cols.assign(cols, cols + E);
  g->h_vn_start = vs;
  g->h_tgt_vn = tv;
  const std::vector<int32_t> ci = work_order(cs, cd, &g->cn_heavy), vi = work_order(vs, vd, &g->vn_heavy);
  const std::vector<int32_t> ct = order_tasks(ci), vt = order_tasks(vi);
  g->n_cn_task = (int32_t)(ct.size() / 4);
  g->n_vn_task = (int32_t)(vt.size() / 4);
  if ((rc = g->cn_start.upload(cs)) || (rc = g->cn_deg.upload(cd)) || (rc = g->tgt_cn.upload(tc)) ||
      (rc = g->vn_start.upload(vs)) || (rc = g->vn_deg.upload(vd)) || (rc = g->tgt_vn.upload(tv)) ||
      (rc = g->csr_cols.upload(cols, E)) || (rc = g->cn_info.upload(ci)) || (rc = g->vn_info.upload(vi)) ||
      (rc = g->cn_task.upload(ct)) || (rc = g->vn_task.upload(vt)))
    return rc;
  *out = g.release();
  return IBL_OK;
}

int ibl_graph_info(const ibl_graph* g, int32_t* n_v, int32_t* n_c, int64_t* n_e, int32_t* dcm, int32_t* dvm) {
  if (!g) return fail(IBL_EINVAL, "graph is NULL");
  if (n_v) *n_v = g->n_v;
  if (n_c) *n_c = g->n_c;
  if (n_e) *n_e = g->n_e;
  if (dcm) *dcm = g->dcm;
  if (dvm) *dvm = g->dvm;
  return IBL_OK;
}

void ibl_graph_destroy(ibl_graph* g) {
  if (g) (void)hipSetDevice(g->device);
  delete g;
}

int ibl_channel_sample(const double* cdf, int32_t T, const double* llr, uint64_t seed, uint64_t offset, int32_t n,
                       int32_t B, const uint8_t* d_bits, void* d_out, int32_t out_dtype, int64_t ld, void* stream) {
  if (!cdf || !d_out) return fail(IBL_EINVAL, "NULL cdf or output");
  if (T < 1 || T > kMaxT) return fail(IBL_EINVAL, "T must lie in [1, 64]");
  if (n < 0 || B < 0) return fail(IBL_EINVAL, "negative shape");
  if (ld < B) return fail(IBL_EINVAL, "ld must be >= B");
  if (out_dtype != kU8 && out_dtype != kI32 && out_dtype != kF32 && out_dtype != kF64)
    return fail(IBL_EINVAL, "unknown output dtype");
  if ((out_dtype == kF32 || out_dtype == kF64) && !llr) return fail(IBL_EINVAL, "LLR output needs llr[T]");
  if (out_dtype == kU8 && T > 256) return fail(IBL_EINVAL, "u8 output needs T <= 256");
  ChArgs a{};
  for (int w = 0; w <= T; ++w) {   // exact: scaling by 2^53 is exact in double; cdf outside [0, 1] saturates
    const double c = std::ldexp(cdf[w], 53);
    a.kthr[w] = std::isnan(c) ? ~0ull : (c <= 0.0 ? 0ull : (c >= 18446744073709551615.0 ? ~0ull : (uint64_t)std::floor(c)));
  }
  if (llr)
    for (int w = 0; w < T; ++w) a.llr[w] = llr[w];
  // binned inversion (sorted thresholds): bin b of m = u 2^53 (b = m >> kChBinSh) holds base = #{w : kthr[w] < bin
  // start} — thresholds every m of the bin exceeds — and n = #{w : kthr[w] inside the bin}, the next n indices
  a.sorted = std::is_sorted(a.kthr + 1, a.kthr + T + 1) ? 1 : 0;
  if (a.sorted)
    for (int b = 0; b < kChBins; ++b) {
      const uint64_t lo = (uint64_t)b << kChBinSh, hi = lo + (1ull << kChBinSh);
      unsigned base = 0, nin = 0;
      for (int w = 1; w <= T; ++w) {
        base += a.kthr[w] < lo ? 1u : 0u;
        nin += (a.kthr[w] >= lo && a.kthr[w] < hi) ? 1u : 0u;
      }
      a.bin[b] = (uint16_t)(base | (nin << 8));
    }
  a.ctr[0] = offset;
  a.key[0] = seed;
  a.bits = d_bits;
  a.out = d_out;
  a.total = (int64_t)n * B;
  a.ld = ld;
  a.B = B;
  a.T = T;
  a.dtype = out_dtype;
  if (a.total == 0) return IBL_OK;
  HIPCHK(launch_ch_sample(a, (hipStream_t)stream));
  return IBL_OK;
}

int ibl_random_bits(uint64_t seed, uint64_t offset, int32_t n, int32_t B, uint8_t* d_out, void* stream) {
  if (!d_out || n < 0 || B < 0) return fail(IBL_EINVAL, "bad arguments");
  if ((int64_t)n * B == 0) return IBL_OK;
  HIPCHK(launch_random_bits(seed, offset, (int64_t)n * B, d_out, (hipStream_t)stream));
  return IBL_OK;
}

int ibl_count_errors(const void* d_x, int32_t dtype, int64_t rows, int32_t B, int64_t ld, double threshold,
                     const uint8_t* d_bits, int64_t bits_ld, int64_t* d_count, void* stream) {
  if (!d_x || !d_bits || !d_count) return fail(IBL_EINVAL, "NULL buffer");
  if (dtype != kU8 && dtype != kI32 && dtype != kF32 && dtype != kF64) return fail(IBL_EINVAL, "unknown dtype");
  if (rows < 0 || B < 0 || ld < B || bits_ld < B) return fail(IBL_EINVAL, "bad shape");
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipMemsetAsync(d_count, 0, sizeof(int64_t), s));
  if (rows * B == 0) return IBL_OK;
  HIPCHK(launch_count_errors(d_x, dtype, rows, B, ld, threshold, d_bits, bits_ld,
                             reinterpret_cast<unsigned long long*>(d_count), s));
  return IBL_OK;
}

int ibl_count_below(const void* d_x, int32_t dtype, int64_t rows, int32_t B, int64_t ld, double threshold,
                    int64_t* d_count, void* stream) {
  if (!d_x || !d_count) return fail(IBL_EINVAL, "NULL buffer");
  if (dtype < kU8 || dtype > kF64) return fail(IBL_EINVAL, "bad dtype");
  if (rows < 0 || B < 0 || ld < B) return fail(IBL_EINVAL, "bad shape");
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipMemsetAsync(d_count, 0, sizeof(int64_t), s));
  if (rows == 0 || B == 0) return IBL_OK;
  HIPCHK(launch_count_below(d_x, dtype, rows, B, ld, threshold, reinterpret_cast<unsigned long long*>(d_count), s));
  return IBL_OK;
}

}  // extern "C"
