// Host-only plumbing shared by the C ABI's translation units (capi_*.hip): the per-thread last error, the HIP
// error check, device-memory ownership (DevBuf), launch timing, captured small-batch chains, the device graph
// handle, and the few helpers more than one decoder uses. No kernel includes this header.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "common.h"
#include "ibldpc.h"

// IBL_DIAG=1 (diagnostic builds, tools/variants.py): the timing-only hooks IBL_VN_PART, IBL_TRACE_WAVES,
// IBL_TRACE_FUSED and IBL_TRACE_LAYERED, IBL_DEBUG_SYNC, and IBL_ALLOW_SCRATCH (create accepts a fast-path build
// with a private segment). The product build has none of them: no decode call reads the environment, and create
// always refuses scratch.
#ifndef IBL_DIAG
#define IBL_DIAG 0
#endif

namespace ibl {

inline thread_local std::string g_err;   // ibl_last_error; ibl::set_error (capi_core.hip) for the other units

inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
// Diagnostic builds: IBL_DEBUG_SYNC=1 synchronises after every launch so an asynchronous fault is
// reported at the launch that caused it (breaks the no-host-sync property of decode).
inline bool debug_sync() {
#if IBL_DIAG
  static const bool on = [] {
    const char* v = getenv("IBL_DEBUG_SYNC");
    return v && *v && *v != '0';
  }();
  return on;
#else
  return false;
#endif
}
#define HIPCHK(expr)                                                                        \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e == hipSuccess && debug_sync()) _e = hipDeviceSynchronize();                      \
    if (_e != hipSuccess)                                                                   \
      return fail(IBL_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e));            \
  } while (0)

// Move-only owner of one hipMalloc: whatever path leaves a create function or drops a handle frees it.
template <typename T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
  DevBuf& operator=(DevBuf&& o) noexcept { return std::swap(p_, o.p_), *this; }
  ~DevBuf() { if (p_) (void)hipFree(p_); }
  int alloc(size_t count) {   // an empty buffer still holds one element: kernels get a valid pointer
    *this = DevBuf();
    hipError_t e = hipMalloc((void**)&p_, std::max<size_t>(count, 1) * sizeof(T));
    if (e != hipSuccess) return fail(IBL_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    return IBL_OK;
  }
  int alloc_zero(size_t count) {
    if (int rc = alloc(count)) return rc;
    return hipMemset(p_, 0, count * sizeof(T)) == hipSuccess ? IBL_OK : fail(IBL_EHIP, "hipMemset failed");
  }
  int upload(const T* h, size_t count) {
    if (int rc = alloc(count)) return rc;
    if (count) HIPCHK(hipMemcpy(p_, h, count * sizeof(T), hipMemcpyHostToDevice));
    return IBL_OK;
  }
  int upload(const std::vector<T>& h) { return upload(h.data(), h.size()); }
  T* get() const { return p_; }
  operator T*() const { return p_; }   // the kernels' Args structs take the raw pointer

 private:
  T* p_ = nullptr;
};

// HIP-event timing of the CN / VN launches (benchmark only).
struct KTimer {
  bool on = false;
  std::vector<hipEvent_t> pool;
  std::vector<std::pair<int, int>> pending;  // (kind 0=CN 1=VN, first event index)
  size_t next = 0;
  int mark(hipStream_t s) {
    if (next == pool.size()) {
      hipEvent_t e;
      if (hipEventCreate(&e) != hipSuccess) return -1;
      pool.push_back(e);
    }
    (void)hipEventRecord(pool[next], s);
    return (int)next++;
  }
  template <typename F>
  hipError_t timed(int kind, hipStream_t s, F&& launch) {
    if (!on) return launch();
    const int a = mark(s);
    hipError_t e = launch();
    mark(s);
    if (a >= 0) pending.emplace_back(kind, a);
    return e;
  }
  int read(double* cn_ms, int32_t* cn_n, double* vn_ms, int32_t* vn_n) {
    double ms[2] = {0, 0};
    int32_t n[2] = {0, 0};
    for (auto& p : pending) {
      if (hipEventSynchronize(pool[p.second + 1]) != hipSuccess) return -1;
      float t = 0.f;
      if (hipEventElapsedTime(&t, pool[p.second], pool[p.second + 1]) != hipSuccess) return -1;
      ms[p.first] += t;
      n[p.first] += 1;
    }
    pending.clear();
    next = 0;
    if (cn_ms) *cn_ms = ms[0];
    if (cn_n) *cn_n = n[0];
    if (vn_ms) *vn_ms = ms[1];
    if (vn_n) *vn_n = n[1];
    return 0;
  }
  ~KTimer() {
    for (auto e : pool) (void)hipEventDestroy(e);
  }
};
// ibl_ib_timing / ibl_float_timing and their _read
template <class H>
int timing_enable(H* h, int32_t enable) {
  if (!h) return fail(IBL_EINVAL, "decoder is NULL");
  h->timer.on = enable != 0;
  return IBL_OK;
}
template <class H>
int timing_read(H* h, double* cn_ms, int32_t* cn_n, double* vn_ms, int32_t* vn_n) {
  if (!h) return fail(IBL_EINVAL, "decoder is NULL");
  return h->timer.read(cn_ms, cn_n, vn_ms, vn_n) ? fail(IBL_EHIP, "event timing failed") : IBL_OK;
}

struct KCfg {
  int grid = 0, block = 256;
  size_t lds = 0;
};

// Small-batch pass chains replayed from captured graphs. A decode of a few codewords is ~2 i_max dependent launches
// of a few microseconds each; launching them one by one costs the host about as much as the GPU spends running
// them, so a caller that does anything else per batch (the BER driver) leaves the GPU waiting. The chain between
// channel staging and the stop-iteration / decision kernels touches only the decoder's own buffers, so it is
// captured once per (batch, early stop) on a private stream and replayed on the caller's stream with one call.
struct ChainGraphs {
  hipStream_t cap = nullptr;
  std::map<std::pair<int, int>, hipGraphExec_t> execs;
  bool on = false;
  void clear() {
    for (auto& e : execs) (void)hipGraphExecDestroy(e.second);
    execs.clear();
  }
  ~ChainGraphs() {
    clear();
    if (cap) (void)hipStreamDestroy(cap);
  }
  // run chain(stream) for key on stream s: replay its graph, capturing it first if needed
  template <class F>
  hipError_t run(int B, int early, hipStream_t s, F&& chain) {
    const auto key = std::make_pair(B, early);
    auto it = execs.find(key);
    if (it == execs.end()) {
      if (!cap) {
        const hipError_t e = hipStreamCreateWithFlags(&cap, hipStreamNonBlocking);
        if (e != hipSuccess) return e;
      }
      if (execs.size() >= 64) clear();   // bounded: at most 64 batch sizes kept
      hipError_t e = hipStreamBeginCapture(cap, hipStreamCaptureModeThreadLocal);
      if (e != hipSuccess) return e;
      const hipError_t ec = chain(cap);
      hipGraph_t graph = nullptr;
      e = hipStreamEndCapture(cap, &graph);
      if (ec != hipSuccess || e != hipSuccess) {
        if (graph) (void)hipGraphDestroy(graph);
        return ec != hipSuccess ? ec : e;
      }
      hipGraphExec_t exec = nullptr;
      e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
      (void)hipGraphDestroy(graph);
      if (e != hipSuccess) return e;
      it = execs.emplace(key, exec).first;
    }
    return hipGraphLaunch(it->second, s);
  }
};

// A create-time A/B knob that is on unless the environment sets it to 0.
inline bool env_on(const char* name) {
  const char* v = getenv(name);
  return !(v && v[0] == '0');
}
// Small-batch settings read once at create: IBL_SMALL_B overrides the default threshold (0 turns the kernels
// off, as does a build whose small-batch kernels need scratch), IBL_SMALL_GRAPH=0 launches the chains pass by pass.
inline void small_batch_env(bool s_ok, int32_t dflt, int32_t* small_b, ChainGraphs* graphs) {
  const char* sb = getenv("IBL_SMALL_B");
  *small_b = s_ok ? (sb ? std::max(0, atoi(sb)) : dflt) : 0;
  graphs->on = env_on("IBL_SMALL_GRAPH");
}

inline int check_path(int32_t path) {
  if (path != IBL_PATH_AUTO && path != IBL_PATH_PASSES && path != IBL_PATH_FUSED)
    return fail(IBL_EINVAL, "path must be IBL_PATH_AUTO, IBL_PATH_PASSES or IBL_PATH_FUSED");
  return IBL_OK;
}

// The decode kernels are built to run without a private segment (launch bounds sized to the node bodies'
// registers, item buffers forced inline). A build whose compiler spills registers or passes an item through
// scratch would silently lose the register budget the design rests on, and such a build once faulted
// (DESIGN.md "Private segment"): create refuses it loudly, with head + the segment's bytes + tail as the message.
inline int refuse_private(size_t priv, const std::string& head, const char* tail) {
  return priv == 0 ? IBL_OK : fail(IBL_EHIP, head + std::to_string(priv) + tail);
}

// Early-stop flag words of iteration j (kShards per iteration), or nullptr when `on` is false: a launch's gate
// (run only if the words are non-zero) or the words its check pass sets.
inline int32_t* flag_row(int32_t* flags, bool on, int j) { return on ? flags + (size_t)j * kShards : nullptr; }

// Whether the output kernels may store n codewords of esz bytes at once: whole groups, d_out aligned to them.
inline int32_t out_aligned(int B, const void* d_out, int n, size_t esz) {
  return ((B % n) == 0 && ((uintptr_t)d_out % (n * esz)) == 0) ? 1 : 0;
}

// Task tables of a fused on-chip kernel (plan.h FusedTasks) on the device, with their counts.
struct FusedTaskBufs {
  DevBuf<int32_t> cn_task, vn_task, vn_node, vn_slot;
  int32_t n_cn = 0, n_vn = 0, n_vs = 0;   // check / variable tasks, variable slots
  int upload(const FusedTasks& ft) {
    int rc;
    if ((rc = cn_task.upload(ft.cn_task)) || (rc = vn_task.upload(ft.vn_task)) || (rc = vn_node.upload(ft.vn_node)) ||
        (rc = vn_slot.upload(ft.vn_slot)))
      return rc;
    n_cn = (int32_t)(ft.cn_task.size() / 4);
    n_vn = (int32_t)(ft.vn_task.size() / 4);
    n_vs = (int32_t)ft.vn_slot.size();
    return IBL_OK;
  }
};
// candidates the fused kernels' bank-order greedy scans per lane (IBL_FUSED_VWIN at create, A/B; default 256)
inline size_t fused_vwin() {
  const char* vw = getenv("IBL_FUSED_VWIN");
  return (size_t)std::max(1, vw ? atoi(vw) : 256);
}

#if IBL_DIAG
// Diagnostic builds: a zeroed device buffer of 64-bit trace words for one launch, written to a file once the
// stream has drained (IBL_TRACE_FUSED, IBL_TRACE_LAYERED, IBL_TRACE_WAVES).
struct TraceBuf {
  DevBuf<uint64_t> d;
  size_t n = 0;
  int open(size_t words, hipStream_t s) {
    if (int rc = d.alloc(n = words)) return rc;
    HIPCHK(hipMemsetAsync(d, 0, sizeof(uint64_t) * n, s));
    return IBL_OK;
  }
  int save(hipStream_t s, const std::string& path, size_t first, size_t count) {
    std::vector<uint64_t> hv(count);
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipMemcpy(hv.data(), d.get() + first, sizeof(uint64_t) * count, hipMemcpyDeviceToHost));
    if (FILE* fp = fopen(path.c_str(), "wb")) {
      fwrite(hv.data(), sizeof(uint64_t), count, fp);
      fclose(fp);
    }
    return IBL_OK;
  }
};
#endif

}  // namespace ibl

struct ibl_graph : ibl::HostGraph {   // host copies (plan.h: fold / fused task set-up) + the device arrays
  int device = 0, num_cus = 256;
  int32_t dcm = 0, dvm = 0, dc_min = 0;   // largest check / variable degree, smallest check degree
  ibl::DevBuf<int32_t> cn_start, cn_deg, tgt_cn;
  ibl::DevBuf<int32_t> vn_start, vn_deg, tgt_vn, csr_cols;
  // fast-path work order: {node, start, degree, 0} per position, heaviest first (stable)
  ibl::DevBuf<int32_t> cn_info, vn_info;
  int32_t cn_heavy = 0, vn_heavy = 0;
  // small-batch kernels: tasks of up to 64 consecutive same-degree positions of cn_info / vn_info
  ibl::DevBuf<int32_t> cn_task, vn_task;
  int32_t n_cn_task = 0, n_vn_task = 0;
};
