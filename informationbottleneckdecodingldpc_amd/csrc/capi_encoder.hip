// C ABI (include/ibldpc.h): the encoder handle (plan.h encoder_plan; encoder_kernels.hip).
#include "host.h"

using namespace ibl;

struct ibl_encoder {
  int device = 0;
  int32_t N = 0, K = 0, M = 0, max_batch = 0, Bw = 0, method = 0, dir = 1, chain = 0;
  std::string algo;
  DevBuf<int32_t> a_ip, a_ix, l_ip, l_ix, p_ip, p_ix, order;
  DevBuf<uint32_t> x, r, t, p, tot;
};

extern "C" {

int ibl_encoder_create(int32_t n_v, int32_t n_c, const int32_t* indptr, const int32_t* cols, int32_t max_batch,
                       int32_t device, ibl_encoder** out) {
  if (!out) return fail(IBL_EINVAL, "out is NULL");
  *out = nullptr;
  if (n_v <= n_c || n_c <= 0) return fail(IBL_EINVAL, "H must have fewer rows than columns");
  if (max_batch < 1) return fail(IBL_EINVAL, "max_batch must be >= 1");
  const int32_t N = n_v, M = n_c, K = N - M;
  HIPCHK(hipSetDevice(device));
  EncPlan pl;
  std::string err;
  const int prc = encoder_plan(N, M, indptr, cols, &pl, &err);
  if (prc != 0) return fail(prc == -3 ? IBL_EUNSUPPORTED : IBL_EINVAL, err);
  std::unique_ptr<ibl_encoder> h(new ibl_encoder());
  h->device = device; h->N = N; h->K = K; h->M = M; h->max_batch = max_batch;
  h->Bw = (max_batch + 31) / 32;
  h->algo = pl.algo;
  h->method = pl.method;
  h->dir = pl.dir;
  h->chain = pl.chain;
  int rc;
  if ((rc = h->a_ip.upload(pl.A.ip)) || (rc = h->a_ix.upload(pl.A.ix)) || (rc = h->p_ip.upload(pl.P.ip)) ||
      (rc = h->p_ix.upload(pl.P.ix)))
    return rc;
  if (h->method == 1 && ((rc = h->l_ip.upload(pl.L.ip)) || (rc = h->l_ix.upload(pl.L.ix)))) return rc;
  if (!pl.order.empty() && (rc = h->order.upload(pl.order))) return rc;
  const size_t wm = (size_t)M * h->Bw;
  if ((rc = h->x.alloc((size_t)K * h->Bw)) || (rc = h->r.alloc(wm)) || (rc = h->t.alloc(wm)) || (rc = h->p.alloc(wm)) ||
      (rc = h->tot.alloc((size_t)enc_scan_segments() * h->Bw)))
    return rc;
  *out = h.release();
  return IBL_OK;
}

const char* ibl_encoder_algorithm(const ibl_encoder* h) { return h ? h->algo.c_str() : ""; }

int ibl_encode(ibl_encoder* h, const uint8_t* d_info, int32_t B, uint8_t* d_code, void* stream) {
  if (!h) return fail(IBL_EINVAL, "encoder is NULL");
  if (B < 1 || B > h->max_batch) return fail(IBL_EINVAL, "B must lie in [1, max_batch]");
  if (!d_info || !d_code) return fail(IBL_EINVAL, "NULL buffer");
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipSetDevice(h->device));
  const int Bw = (B + 31) / 32, M = h->M;
  HIPCHK(launch_enc_pack(d_info, h->K, B, Bw, h->x, s));
  HIPCHK(launch_enc_ax(h->x, h->a_ip, h->a_ix, M, Bw, h->r, s));
  uint32_t* cur = h->r;
  if (h->method == 1) {                                 // L substitution (forward), then row order
    HIPCHK(launch_enc_subst(cur, h->t, h->l_ip, h->l_ix, M, Bw, 1, s));
    cur = h->t;
  }
  if (h->order) {
    uint32_t* dst = cur == h->r ? h->t : h->r;
    HIPCHK(launch_enc_gather(cur, h->order, M, Bw, dst, s));
    cur = dst;
  }
  if (h->chain) HIPCHK(launch_enc_scan(cur, h->tot, M, Bw, h->dir, h->p, s));
  else HIPCHK(launch_enc_subst(cur, h->p, h->p_ip, h->p_ix, M, Bw, h->dir, s));
  HIPCHK(launch_enc_unpack(d_info, h->p, h->K, M, B, Bw, d_code, s));
  return IBL_OK;
}

void ibl_encoder_destroy(ibl_encoder* h) {
  if (h) (void)hipSetDevice(h->device);
  delete h;
}

}  // extern "C"
