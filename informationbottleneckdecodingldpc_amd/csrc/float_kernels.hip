// Float min-sum / belief-propagation LDPC decoding kernels for MI355X (gfx950).
//
// Replaces Continous_LDPC_Decoding/kernels_min_and_BP.cl (fp64 in the reference):
//   send_channel_values_to_checknode_inbox -> fl_stage + fl_cn (first pass gathers nothing: the
//                                            staged channel rows are scattered by fl_send)
//   checknode_update_minsum (:126-167)    -> fl_cn<MINSUM>
//   checknode_update + boxplus (:5-71)    -> fl_cn<BP>
//   varnode_update (:76-123)              -> fl_vn
//   calc_syndrome (:206-227)              -> fused into fl_cn (parity of its inputs)
//   calc_varnode_output (:170-204)        -> fl_dec
//
// Precision: F = float (the BASELINE's float32 build) or double (strict parity build).
//   * min-sum is computed from (min1, min2, sign product, zero count) of the node's inputs —
//     bit-identical to the reference's sequential sign/min fold, which only selects values;
//   * BP folds are evaluated with prefix sharing in exactly the reference's per-output order
//     (t = boxplus(m_next, t), clamped at every step); fp64 uses the reference's formula
//     log((1+e^{a+b})/(e^a+e^b)), fp32 the overflow-free equivalent
//     sgn(a)sgn(b)min(|a|,|b|) + log1p(e^-|a+b|) - log1p(e^-|a-b|) (the naive form overflows
//     float for a+b > 88);
//   * variable-node sums keep the reference's addition order (channel first, then ascending
//     edges) through prefix sharing, so fp64 sums are bit-identical.
// Each wave item is one node x kChunk codewords; a lane holds 16 bytes of every edge row
// (4 fp32 or 2 fp64 codewords; fp64 items cover 128 codewords).
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "boxplus.h"

namespace ibl {

// Work-item geometry from the hardware registers and the implicit kernel arguments. This source is built with
// the IEEE mode off (_build.py), an attribute the device libraries do not share, so HIP's threadIdx /
// blockIdx / blockDim / gridDim — calls into them — would stay out-of-line calls in every kernel.
// The grid size is the implicit argument hidden_block_count_x (code object v5: offset 0), in the kernarg
// segment. __builtin_amdgcn_grid_size_x() reads the AQL dispatch packet instead, which lives in the queue's
// ring buffer in host memory: every CU's first wave then waits on a host round trip, ~20 us of every launch
// (round 6: the float small-batch passes took 23-32 us at B = 2, the IB ones 7-9 us).
__device__ __forceinline__ int fl_tid() { return (int)__builtin_amdgcn_workitem_id_x(); }
__device__ __forceinline__ int fl_bid() { return (int)__builtin_amdgcn_workgroup_id_x(); }
__device__ __forceinline__ int fl_bdim() { return (int)__builtin_amdgcn_workgroup_size_x(); }
__device__ __forceinline__ int fl_gdim() {
  return *(cint32*)__builtin_amdgcn_implicitarg_ptr();   // constant address space, as the pointer is
}

template <typename F> struct Vec;
template <> struct Vec<float> {
  static constexpr int N = 4;
  using T = float4;
  __device__ static float get(const T& v, int s) { return s == 0 ? v.x : s == 1 ? v.y : s == 2 ? v.z : v.w; }
  __device__ static void set(T& v, int s, float x) {
    if (s == 0) v.x = x; else if (s == 1) v.y = x; else if (s == 2) v.z = x; else v.w = x;
  }
};
template <> struct Vec<double> {
  static constexpr int N = 2;
  using T = double2;
  __device__ static double get(const T& v, int s) { return s == 0 ? v.x : v.y; }
  __device__ static void set(T& v, int s, double x) { if (s == 0) v.x = x; else v.y = x; }
};

// sign(t) * min(llr_max, sign(t) * t)  (kernels_min_and_BP.cl:69,120) is the clamp of t to
// [-llr_max, llr_max] for every non-NaN t, signed zeros included (sign(+-0) = +-0 gives +-0 back):
// one v_med3_f32 in fp32 instead of the 3 compares, 3 selects, 2 products and a min of the literal
// form. Messages are never NaN (ibldpc.h's precondition), and this source is built with
// -fno-honor-nans and the IEEE mode off (_build.py): min / max / median then take their operands
// directly instead of quieting each through a v_max x, x first.
__device__ __forceinline__ float clampllr(float t, float lm) { return __builtin_amdgcn_fmed3f(t, -lm, lm); }
__device__ __forceinline__ double clampllr(double t, double lm) { return fmin(fmax(t, -lm), lm); }

// sign-bit arithmetic of the min-sum check node
template <typename F> struct Bits;
template <> struct Bits<float> {
  using U = uint32_t;
  static constexpr U kSign = 0x80000000u;
  __device__ static U of(float x) { return __float_as_uint(x); }
  __device__ static float from(U u) { return __uint_as_float(u); }
  // on raw messages: min(|a|, |b|), max(|a|, |b|), median(lo, hi, |x|), min(lo, |x|)
  __device__ static float lo_aa(float a, float b) { return fminf(fabsf(a), fabsf(b)); }
  __device__ static float hi_aa(float a, float b) { return fmaxf(fabsf(a), fabsf(b)); }
  __device__ static float med3_a(float lo, float hi, float x) { return __builtin_amdgcn_fmed3f(lo, hi, fabsf(x)); }
  __device__ static float lo_a(float lo, float x) { return fminf(lo, fabsf(x)); }
  __device__ static float lo(float a, float b) { return fminf(a, b); }
  // the compiler keeps v_and_b32 + v_or_b32 for this (gfx9 VOP3 takes no literal): one v_and_or_b32 with
  // the mask in an SGPR places a sign bit
  __device__ static U and_or(U a, U k, U b) {
    U r;
    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(k), "v"(b));
    return r;
  }
  __device__ static U sign_mask() { return __builtin_amdgcn_readfirstlane(kSign); }
};
template <> struct Bits<double> {
  using U = uint64_t;
  static constexpr U kSign = 0x8000000000000000ull;
  __device__ static U of(double x) { return (U)__double_as_longlong(x); }
  __device__ static double from(U u) { return __longlong_as_double((long long)u); }
  // median of (lo <= hi, |x|): max(lo, min(hi, |x|))
  __device__ static double lo_aa(double a, double b) { return fmin(fabs(a), fabs(b)); }
  __device__ static double hi_aa(double a, double b) { return fmax(fabs(a), fabs(b)); }
  __device__ static double med3_a(double lo, double hi, double x) { return fmax(lo, fmin(hi, fabs(x))); }
  __device__ static double lo_a(double lo, double x) { return fmin(lo, fabs(x)); }
  __device__ static double lo(double a, double b) { return fmin(a, b); }
  __device__ static U and_or(U a, U k, U b) { return (a & k) | b; }
  __device__ static U sign_mask() { return kSign; }
};

__device__ __forceinline__ double boxplus(double a, double b, double lm) {
  const double boxp = log((1.0 + exp(a + b)) / (exp(a) + exp(b)));
  return clampllr(boxp, lm);
}
// the fp32 box-plus, boxplus(float, float, lm): boxplus.h (shared with the layered BP kernels)

__device__ __forceinline__ bool fl_gate(const int32_t* gate, int lane) {
  if (!gate) return true;
  return __ballot(gate[lane] != 0) != 0ull;
}

// Node bodies work on all N codewords of the lane at once. Output rows of degrees > 8 are stored
// as soon as they are final, so only the D input rows are live in registers (WLAN's degree-11
// variable nodes: 136 -> 85 VGPRs, +14 %); degrees <= 8 keep their outputs and store them together
// at the end of the item, which measured 9 % faster on DVB-S2 (3.21 -> 2.93 ms per VN pass).
// IBL_FL_NT = 1: the per-pass kernels' message / channel rows as nontemporal loads and stores (every row is
// streamed once per pass, far beyond the caches at C5's B = 8192). Same box, two repetitions
// (profiles/r05_c5_nontemporal_ab.json): C5 16.37k / 16.39k cw/s vs 16.17k / 16.18k plain (fl_vn 2.05 vs 2.12 ms).
#ifndef IBL_FL_NT
#define IBL_FL_NT 1
#endif
template <typename F> struct NtVec;
template <> struct NtVec<float> { typedef float T __attribute__((ext_vector_type(4))); };
template <> struct NtVec<double> { typedef double T __attribute__((ext_vector_type(2))); };

// One lane's 16 bytes (Vec<F>::N codewords): codewords cw0.. of row `row` of the [.][ldb] message or channel array
// at `base`, or the LDS slot at `base` itself (no row: the fused items pass the slot's address, which keeps their
// addresses 32-bit). NT: a nontemporal access (kFlNt) — the per-pass kernels' row loads and stores and the
// small-batch kernels' row stores; the small-batch and decision kernels' loads and every LDS access are plain.
constexpr bool kFlNt = IBL_FL_NT != 0;
template <bool NT, typename F>
__device__ __forceinline__ void fl_load16(const void* base, F (&v)[Vec<F>::N], int ldb = 0, int row = 0, int cw0 = 0) {
  using V = Vec<F>;
  const F* p = reinterpret_cast<const F*>(base) + (size_t)row * ldb + cw0;
  if constexpr (NT) {
    const typename NtVec<F>::T r = __builtin_nontemporal_load(reinterpret_cast<const typename NtVec<F>::T*>(p));
#pragma unroll
    for (int s = 0; s < V::N; ++s) v[s] = r[s];
  } else {
    const typename V::T r = *reinterpret_cast<const typename V::T*>(p);
#pragma unroll
    for (int s = 0; s < V::N; ++s) v[s] = V::get(r, s);
  }
}
template <bool NT, typename F>
__device__ __forceinline__ void fl_store16(void* base, const F (&v)[Vec<F>::N], int ldb = 0, int row = 0, int cw0 = 0) {
  using V = Vec<F>;
  F* p = reinterpret_cast<F*>(base) + (size_t)row * ldb + cw0;
  if constexpr (NT) {
    typename NtVec<F>::T o;
#pragma unroll
    for (int s = 0; s < V::N; ++s) o[s] = v[s];
    __builtin_nontemporal_store(o, reinterpret_cast<typename NtVec<F>::T*>(p));
  } else {
    typename V::T o;
#pragma unroll
    for (int s = 0; s < V::N; ++s) V::set(o, s, v[s]);
    *reinterpret_cast<typename V::T*>(p) = o;
  }
}

template <typename F, int D>
struct FlOut {
  static constexpr bool kImmediate = D > 8;
  static constexpr int N = Vec<F>::N;
  F v[kImmediate ? 1 : D][N];
  // sink(w, o) stores output w
  template <class Sink>
  __device__ __forceinline__ void put(int w, const F (&o)[N], Sink&& sink) {
    if constexpr (kImmediate) {
      sink(w, o);
    } else {
#pragma unroll
      for (int s = 0; s < N; ++s) v[w][s] = o[s];
    }
  }
  template <class Sink>
  __device__ __forceinline__ void flush(Sink&& sink) {
    if constexpr (!kImmediate) {
#pragma unroll
      for (int w = 0; w < D; ++w) sink(w, v[w]);
    }
  }
};

// XOR of the inputs' sign bits for codeword s. Its sign bit is also
// the syndrome parity of the inputs (calc_syndrome, kernels_min_and_BP.cl:206-227: parity of m < 0):
// a check's inputs are never -0, since the staged channel holds no -0 (fl_stage*, which turn -0 into +0:
// equal values) and a variable's output clamp(ch + sum) is -0 only if every addend is.
template <typename F, int D>
__device__ __forceinline__ typename Bits<F>::U sign_xor(const F (&m)[D][Vec<F>::N], int s) {
  using Bt = Bits<F>;
  typename Bt::U x = Bt::of(m[0][s]);
#pragma unroll
  for (int j = 1; j < D; ++j) x ^= Bt::of(m[j][s]);
  return x;
}

// Syndrome parity of codeword s's inputs: the sign bit of sign_xor (degrees <= 8); larger degrees keep
// the compare-and-mask form (lane masks in SGPRs), which needs no VGPR beside the 16 inputs.
template <typename F, int D>
__device__ __forceinline__ bool syndrome_bit(const F (&m)[D][Vec<F>::N], int s) {
  if constexpr (D <= 8) {
    return (sign_xor<F, D>(m, s) >> (8 * sizeof(F) - 1)) != 0;
  } else {
    bool p = false;
#pragma unroll
    for (int j = 0; j < D; ++j) p ^= (m[j][s] < F(0));
    return p;
  }
}

// Check-body kinds: the public IBL_MINSUM (0) and IBL_BP (1), and the library's own corrected min-sum.
constexpr int kFlCorrected = 2;
// The check and fused kernels take the kind as KX = kind plus flag bits (kFlEach, at fl_fused: the per-codeword-stop
// form). kFlWide marks the wide instantiations and goes with MAXD = kFlWideD: a bit of the kind and not a parameter
// or a kernel of another name, so that the narrow instantiations keep their symbols and a wide kernel's symbol differs
// from every narrow one's in its first argument (the censuses of the narrow kernels by kind, as
// tests/test_cpu_minsum_corrected.py's of kind 2, then count what they always counted).
constexpr int kFlWide = 8;

// Corrected min-sum magnitude (ibldpc.h "Corrected min-sum"): r = max(a * M - b, 0) as one rounded
// multiplication and one rounded subtraction. HIP contracts a * M - b into a fused multiply-add by default,
// which rounds once: contraction is off for these two operations only (the rest of this source keeps it).
template <typename F>
__device__ __forceinline__ F fl_corrected(F M, F a, F b) {
#pragma clang fp contract(off)
  const F t = a * M;
  const F u = t - b;
  return fmax(u, F(0));
}

// alpha and beta of the corrected kind from the kernel arguments (FlArgs / FlFusedArgs); the other kinds
// read neither
template <int KIND, typename F, class Args>
__device__ __forceinline__ void fl_correction(const Args& a, F& ca, F& cb) {
  if constexpr (KIND == kFlCorrected) {
    ca = (F)a.cor_a;
    cb = (F)a.cor_b;
  } else {
    ca = F(1);
    cb = F(0);
  }
}

// Check-node body on the inputs m of the lane's codewords (min-sum, BP or corrected min-sum with alpha ca and
// beta cb); put(w, o) receives output w (any order of w).
template <int KIND, typename F, int D, class Put>
__device__ __forceinline__ void fl_cn_body(const F (&m)[D][Vec<F>::N], F lm, F ca, F cb, Put&& put) {
  constexpr int N = Vec<F>::N;
  F o[N];
  if constexpr (KIND == 0 && D <= 8) {
    // min-sum (kernels_min_and_BP.cl:156-162) with prefix / suffix minima: |out_w| = min over the others =
    // min(P_w, S_{w+1}), P_w = min |m_0..m_{w-1}|, S_j = min |m_j..m_{D-1}| — 3(D-2) v_min (|x| as an input
    // modifier) instead of the running (min, second min) pair plus a compare and a select per output
    // (4D - 2); min only selects, so the outputs are the same bits. Signs: XOR of the others' sign bits
    // (sign_xor ^ own), placed with one v_and_or_b32. A zero input gives every other output +-0 and its own
    // the others' minimum, as the reference's sign(0) = 0 fold; the same tiny-LLR assumption as below.
    using Bt = Bits<F>;
    using U = typename Bt::U;
    const U ks = Bt::sign_mask();
    U sg[N];
#pragma unroll
    for (int s = 0; s < N; ++s) sg[s] = sign_xor<F, D>(m, s);
    auto emit = [&](int w, const F (&mag)[N]) __attribute__((always_inline)) {
#pragma unroll
      for (int s = 0; s < N; ++s) o[s] = Bt::from(Bt::and_or(sg[s] ^ Bt::of(m[w][s]), ks, Bt::of(mag[s])));
      put(w, o);
    };
    if constexpr (D == 2) {
      F a[N], b[N];
#pragma unroll
      for (int s = 0; s < N; ++s) { a[s] = fabs(m[1][s]); b[s] = fabs(m[0][s]); }
      emit(0, a);
      emit(1, b);
    } else {
      F S[D][N], P[N], mg[N];   // S[j] for j = 1..D-2
#pragma unroll
      for (int s = 0; s < N; ++s) S[D - 2][s] = Bt::lo_aa(m[D - 2][s], m[D - 1][s]);
#pragma unroll
      for (int j = D - 3; j >= 1; --j)
#pragma unroll
        for (int s = 0; s < N; ++s) S[j][s] = Bt::lo_a(S[j + 1][s], m[j][s]);
      emit(0, S[1]);
#pragma unroll
      for (int s = 0; s < N; ++s) P[s] = fabs(m[0][s]);
#pragma unroll
      for (int w = 1; w <= D - 2; ++w) {
#pragma unroll
        for (int s = 0; s < N; ++s) mg[s] = w + 1 <= D - 2 ? Bt::lo(P[s], S[w + 1][s]) : Bt::lo_a(P[s], m[D - 1][s]);
        emit(w, mg);
#pragma unroll
        for (int s = 0; s < N; ++s) P[s] = Bt::lo_a(P[s], m[w][s]);
      }
      emit(D - 1, P);
    }
  } else if constexpr (KIND != 1) {
    // min-sum at degrees > 8 and corrected min-sum at every degree, on the running (min, second min) pair.
    // min-sum (kernels_min_and_BP.cl:156-162): the fold t = sgn(m t) min(|t|, |m|) over the others of
    // output w only selects values, so |out_w| = min over the others = mn1, or mn2 where |m_w| is the
    // minimum (on a tie mn2 == mn1), and its sign is the XOR of the others' sign bits. A zero input
    // (sign() = 0 kills the reference's fold) makes mn1 = 0, so every other output is +-0 as there; the
    // zero's own output is the others' min. Running (mn1, mn2) with v_min / v_med3 on |m| (abs is an
    // input modifier), signs XORed as bits: ~2.5 VALU per input and 4 per output.
    // Assumption (the only case where the closed form and the fold differ): no product m*t of the fold
    // underflows to 0 (sign(0) = 0 would zero the reference's output). Every message is a sum of channel
    // LLRs and selected messages, so each nonzero one is a multiple of the ulp q of the smallest nonzero
    // |channel LLR|; with that LLR >= 2^-50 (fp32; 2^-450 fp64) every product is >= 2^-146 and none
    // underflows (tests/test_gpu_float.py::test_float32_minsum_tiny_llrs runs that boundary bit-exactly).
    // Corrected min-sum (kind 2): the correction on those two values only (2 x {mul, sub, max} per check and
    // codeword, whatever the degree; correcting the prefix / suffix form's outputs would cost 3 per edge).
    // Output w takes the corrected second minimum where |m_w| is the minimum (on a tie both are equal) and the
    // corrected minimum elsewhere — the compare stays against the uncorrected mn1: the closed form of the
    // specification, since the correction is a function of the magnitude alone. r >= +0, so OR-ing the sign
    // bit negates it; the sign of a zero is not specified. Per edge: 2 (running pair) + 1 (sign XOR) +
    // 4 (compare, select, XOR, and-or), plus 6 per check (2 x {mul, sub, max}).
    using Bt = Bits<F>;
    using U = typename Bt::U;
    F mn1[N], mn2[N], r1[N], r2[N];   // r1, r2: the corrected pair (kind 2 only)
    U sg[N];
    const U ks = Bt::sign_mask();
#pragma unroll
    for (int s = 0; s < N; ++s) {
      mn1[s] = Bt::lo_aa(m[0][s], m[1][s]);
      mn2[s] = Bt::hi_aa(m[0][s], m[1][s]);
      sg[s] = sign_xor<F, D>(m, s);
#pragma unroll
      for (int j = 2; j < D; ++j) {
        mn2[s] = Bt::med3_a(mn1[s], mn2[s], m[j][s]);
        mn1[s] = Bt::lo_a(mn1[s], m[j][s]);
      }
      if constexpr (KIND == kFlCorrected) {
        r1[s] = fl_corrected(mn1[s], ca, cb);
        r2[s] = fl_corrected(mn2[s], ca, cb);
      }
    }
    // the pair an output selects from: references, so the plain kind's code holds no copy of it
    const F (&o1)[N] = KIND == kFlCorrected ? r1 : mn1;
    const F (&o2)[N] = KIND == kFlCorrected ? r2 : mn2;
#pragma unroll
    for (int w = 0; w < D; ++w) {
#pragma unroll
      for (int s = 0; s < N; ++s) {
        const F mag = (fabs(m[w][s]) == mn1[s]) ? o2[s] : o1[s];
        const U sx = sg[s] ^ Bt::of(m[w][s]);
        // one v_and_or_b32 for degrees <= 8; degrees > 8 keep the compiler's and / or form: the asm operand
        // copies would push the 16-input body past the 128 VGPRs of a 1024-thread block
        o[s] = Bt::from(D <= 8 ? Bt::and_or(sx, ks, Bt::of(mag)) : (sx & Bt::kSign) | Bt::of(mag));
      }
      put(w, o);
    }
  } else if constexpr (sizeof(F) == 4) {
    // fp32 BP: forward-backward box-plus, 3(D-2) operations instead of the (D-2)(D+3)/2 of the
    // reference's per-output folds (degree 7: 15 vs 25; each costs 4 transcendentals). Box-plus is
    // commutative and associative, and |a [+] b| <= min(|a|,|b|) keeps every partial result inside
    // the clamp for clamped inputs, so only the fp32 rounding differs from the reference order
    // (within the tolerance of tests/test_gpu_float.py; the fp64 build keeps the exact order below).
    F S[D][N], P[N];   // S[j] = m_j [+] ... [+] m_{D-1}, j >= 1
#pragma unroll
    for (int s = 0; s < N; ++s) S[D - 1][s] = m[D - 1][s];
#pragma unroll
    for (int j = D - 2; j >= 1; --j)
#pragma unroll
      for (int s = 0; s < N; ++s) S[j][s] = boxplus(m[j][s], S[j + 1][s], lm);
#pragma unroll
    for (int s = 0; s < N; ++s) o[s] = clampllr(S[1][s], lm);
    put(0, o);
#pragma unroll
    for (int s = 0; s < N; ++s) P[s] = m[0][s];
#pragma unroll
    for (int w = 1; w <= D - 2; ++w) {
#pragma unroll
      for (int s = 0; s < N; ++s) o[s] = clampllr(boxplus(P[s], S[w + 1][s], lm), lm);
      put(w, o);
#pragma unroll
      for (int s = 0; s < N; ++s) P[s] = boxplus(m[w][s], P[s], lm);
    }
#pragma unroll
    for (int s = 0; s < N; ++s) o[s] = clampllr(P[s], lm);
    put(D - 1, o);
  } else {
    // BP sequential box-plus folds with prefix sharing (kernels_min_and_BP.cl:63-69)
    F t[N], P[N];
#pragma unroll
    for (int s = 0; s < N; ++s) t[s] = m[1][s];
#pragma unroll
    for (int j = 2; j < D; ++j)
#pragma unroll
      for (int s = 0; s < N; ++s) t[s] = boxplus(m[j][s], t[s], lm);
#pragma unroll
    for (int s = 0; s < N; ++s) o[s] = clampllr(t[s], lm);
    put(0, o);
#pragma unroll
    for (int s = 0; s < N; ++s) P[s] = m[0][s];
#pragma unroll
    for (int w = 1; w <= D - 2; ++w) {
#pragma unroll
      for (int s = 0; s < N; ++s) t[s] = P[s];
#pragma unroll
      for (int j = w + 1; j < D; ++j)
#pragma unroll
        for (int s = 0; s < N; ++s) t[s] = boxplus(m[j][s], t[s], lm);
#pragma unroll
      for (int s = 0; s < N; ++s) o[s] = clampllr(t[s], lm);
      put(w, o);
#pragma unroll
      for (int s = 0; s < N; ++s) P[s] = boxplus(m[w][s], P[s], lm);
    }
#pragma unroll
    for (int s = 0; s < N; ++s) o[s] = clampllr(P[s], lm);
    put(D - 1, o);
  }
}

// Wide check-node body: one body for every degree d in 17..kFlWideD (wave-uniform, taken at run time), for the wide
// instantiations (MAXD = kFlWideD) of the three families. It holds no input array: load(j, r) fetches input j of
// the lane's codewords (any number of times), put(w, o) receives output w in ascending w, and input w is always
// loaded before output w is put, so the fused kernel may run it in place. par[s] gets the XOR of the high words of
// codeword s's inputs (bit 31: the syndrome parity, as syndrome_bit).
//   min-sum / corrected: the running (min, second min, position of the first minimum) and a word of the inputs'
//     sign bits per codeword (the wide layered kernels' form): output w takes the second minimum at the first
//     minimum's position and the minimum elsewhere. On a tie the second minimum equals the minimum, so the values
//     are those of fl_cn_body's |m_w| == mn1 ? o2 : o1 bit for bit; zero inputs and the tiny-LLR assumption as there.
//   fp32 BP: fl_cn_body's forward-backward form in the same association order (S_j = m_j [+] S_{j+1},
//     out_w = P_w [+] S_{w+1}, P_{w+1} = m_w [+] P_w). The suffixes stay in registers (31 x N), the steps are fully
//     unrolled and predicated on the degree, and the forward sweep loads each input again instead of keeping it.
//   fp64 BP: the reference's per-output sequential folds with the shared prefix (kernels_min_and_BP.cl:63-69), as
//     rolled loops that load their inputs again: (d - 2)(d + 3) / 2 box-pluses, each an exp and a log call.
template <typename F> __device__ __forceinline__ uint32_t fl_hi32(F x) {
  if constexpr (sizeof(F) == 4) return __float_as_uint(x);
  else return (uint32_t)((uint64_t)__double_as_longlong(x) >> 32);
}
template <typename F> __device__ __forceinline__ F fl_with_sign(F mag, uint32_t sign31) {   // mag >= +0
  if constexpr (sizeof(F) == 4) return __uint_as_float((sign31 & 0x80000000u) | __float_as_uint(mag));
  else return __longlong_as_double((long long)(((uint64_t)(sign31 & 0x80000000u) << 32) | (uint64_t)__double_as_longlong(mag)));
}
template <int KIND, typename F, class Load, class Put>
__device__ __forceinline__ void fl_cn_wide_body(int d, F lm, F ca, F cb, uint32_t (&par)[Vec<F>::N], Load&& load,
                                                Put&& put) {
  constexpr int N = Vec<F>::N;
  F o[N], r[N];
  if constexpr (KIND != 1) {
    using Bt = Bits<F>;
    F mn1[N], mn2[N];
    uint32_t sw[N];   // bit j = sign of input j
    int pos[N];
    load(0, r);
#pragma unroll
    for (int s = 0; s < N; ++s) {
      mn1[s] = fabs(r[s]);
      mn2[s] = __builtin_huge_val();
      pos[s] = 0;
      par[s] = fl_hi32(r[s]);
      sw[s] = par[s] >> 31;
    }
#pragma unroll 8
    for (int j = 1; j < d; ++j) {
      load(j, r);
#pragma unroll
      for (int s = 0; s < N; ++s) {
        const uint32_t h = fl_hi32(r[s]);
        par[s] ^= h;
        sw[s] |= (h >> 31) << j;
        pos[s] = fabs(r[s]) < mn1[s] ? j : pos[s];
        mn2[s] = Bt::med3_a(mn1[s], mn2[s], r[s]);
        mn1[s] = Bt::lo_a(mn1[s], r[s]);
      }
    }
    F o1[N], o2[N];
#pragma unroll
    for (int s = 0; s < N; ++s) {
      o1[s] = KIND == kFlCorrected ? fl_corrected(mn1[s], ca, cb) : mn1[s];
      o2[s] = KIND == kFlCorrected ? fl_corrected(mn2[s], ca, cb) : mn2[s];
    }
#pragma unroll 2
    for (int w = 0; w < d; ++w) {
#pragma unroll
      for (int s = 0; s < N; ++s)
        o[s] = fl_with_sign<F>(pos[s] == w ? o2[s] : o1[s], par[s] ^ ((sw[s] >> w) << 31));
      put(w, o);
    }
  } else if constexpr (sizeof(F) == 4) {
    F S[kFlWideD][N], P[N];   // S[j] = m_j [+] ... [+] m_{d-1}, 1 <= j <= d - 1
#pragma unroll
    for (int s = 0; s < N; ++s) par[s] = 0;
#pragma unroll
    for (int j = kFlWideD - 1; j >= 1; --j) {
      if (j <= 16 || j < d) {   // d >= 17
        load(j, r);
        constexpr int kLast = kFlWideD - 1;
        const int jn = j < kLast ? j + 1 : kLast;   // j = 31 is always the last input
#pragma unroll
        for (int s = 0; s < N; ++s) par[s] ^= fl_hi32(r[s]);
        if (j >= 16 && j == d - 1) {
#pragma unroll
          for (int s = 0; s < N; ++s) S[j][s] = r[s];
        } else {
#pragma unroll
          for (int s = 0; s < N; ++s) S[j][s] = boxplus(r[s], S[jn][s], lm);
        }
      }
    }
    load(0, r);
#pragma unroll
    for (int s = 0; s < N; ++s) {
      par[s] ^= fl_hi32(r[s]);
      o[s] = clampllr(S[1][s], lm);
      P[s] = r[s];
    }
    put(0, o);
#pragma unroll
    for (int w = 1; w <= kFlWideD - 2; ++w) {
      if (w <= 15 || w <= d - 2) {
        load(w, r);
#pragma unroll
        for (int s = 0; s < N; ++s) o[s] = clampllr(boxplus(P[s], S[w + 1][s], lm), lm);
        put(w, o);
#pragma unroll
        for (int s = 0; s < N; ++s) P[s] = boxplus(r[s], P[s], lm);
      }
    }
#pragma unroll
    for (int s = 0; s < N; ++s) o[s] = clampllr(P[s], lm);
    put(d - 1, o);
  } else {
    F t[N], P[N];
    load(1, t);
#pragma unroll
    for (int s = 0; s < N; ++s) par[s] = fl_hi32(t[s]);
    for (int j = 2; j < d; ++j) {
      load(j, r);
#pragma unroll
      for (int s = 0; s < N; ++s) {
        par[s] ^= fl_hi32(r[s]);
        t[s] = boxplus(r[s], t[s], lm);
      }
    }
    load(0, P);
#pragma unroll
    for (int s = 0; s < N; ++s) {
      par[s] ^= fl_hi32(P[s]);
      o[s] = clampllr(t[s], lm);
    }
    put(0, o);
    for (int w = 1; w <= d - 2; ++w) {
#pragma unroll
      for (int s = 0; s < N; ++s) t[s] = P[s];
      for (int j = w + 1; j < d; ++j) {
        load(j, r);
#pragma unroll
        for (int s = 0; s < N; ++s) t[s] = boxplus(r[s], t[s], lm);
      }
      load(w, r);
#pragma unroll
      for (int s = 0; s < N; ++s) o[s] = clampllr(t[s], lm);
      put(w, o);
#pragma unroll
      for (int s = 0; s < N; ++s) P[s] = boxplus(r[s], P[s], lm);
    }
#pragma unroll
    for (int s = 0; s < N; ++s) o[s] = clampllr(P[s], lm);
    put(d - 1, o);
  }
}


// Degree-2 variable fold (FlArgs::fold): a degree-2 variable's update is one add and a clamp per output,
// out(c1) = clamp(ch + m(c2 -> v)) (kernels_min_and_BP.cl:110-118; fl_vn_body<D=2> in the same order), so
// the check that produces m(c2 -> v) writes v's message to c1 itself, straight into the next check pass's
// inbox (fout, double-buffered: this pass never reads what it writes), and the variable pass skips v. Per
// folded variable and codeword that moves 2 channel reads instead of the variable pass's 2 message reads,
// 1 channel read and 2 message writes; the outputs are the same bits.
template <int KIND, typename F, int D>
__device__ __forceinline__ void fl_cn_item(const FlArgs& a, int node, int st, int cw0, bool do_par, int valid,
                                           bool& unsat) {
  using V = Vec<F>;
  constexpr int N = V::N;
  const F lm = (F)a.llr_max;
  int tg[D];   // output rows, loaded up front as scalars (the stores follow each output)
#pragma unroll
  for (int w = 0; w < D; ++w) tg[w] = sload(a.tgt, st + w);
  F m[D][N];
#pragma unroll
  for (int j = 0; j < D; ++j) fl_load16<kFlNt, F>(a.in, m[j], a.ldb, st + j, cw0);
  // fold record: wave-uniform (scalar) positions, rows and variables; the channel rows load with the inputs
  int fp0 = -1, fp1 = -1, fd0 = 0, fd1 = 0;
  F c0[N], c1[N];
  if (a.fold_mode) {
    const int* fr = a.fold + (size_t)kFoldRec * node;
    fp0 = sload(fr, 0);
    fp1 = sload(fr, 1);
    fd0 = sload(fr, 2);
    fd1 = sload(fr, 3);
    if (fp0 >= 0) fl_load16<kFlNt, F>(a.ch, c0, a.ldb, sload(fr, 4), cw0);
    if (fp1 >= 0) fl_load16<kFlNt, F>(a.ch, c1, a.ldb, sload(fr, 5), cw0);
  }
  if (do_par) {
#pragma unroll
    for (int s = 0; s < N; ++s) unsat |= syndrome_bit<F, D>(m, s) && s < valid;
  }
  auto fold_put = [&](int w, const F (&c)[N], int row, const F (&o)[N]) __attribute__((always_inline)) {
    F f[N];
#pragma unroll
    for (int s = 0; s < N; ++s) f[s] = clampllr(c[s] + o[s], lm);
    fl_store16<kFlNt, F>(a.fout, f, a.ldb, row, cw0);
    if (a.fold_mode == 2) fl_store16<kFlNt, F>(a.out, o, a.ldb, tg[w], cw0);
  };
  auto sink = [&](int w, const F (&o)[N]) __attribute__((always_inline)) {
    if (w == fp0) fold_put(w, c0, fd0, o);
    else if (w == fp1) fold_put(w, c1, fd1, o);
    else fl_store16<kFlNt, F>(a.out, o, a.ldb, tg[w], cw0);
  };
  FlOut<F, D> ob;
  F ca, cb;
  fl_correction<KIND, F>(a, ca, cb);
  fl_cn_body<KIND, F, D>(m, lm, ca, cb,
                         [&](int w, const F (&o)[N]) __attribute__((always_inline)) { ob.put(w, o, sink); });
  ob.flush(sink);
}

// Syndrome of a wide check from fl_cn_wide_body's parity words; U as fused_cn_item's
template <typename F, class U>
__device__ __forceinline__ void fl_wide_syndrome(const uint32_t (&par)[Vec<F>::N], int valid, U& unsat) {
#pragma unroll
  for (int s = 0; s < Vec<F>::N; ++s) {
    const bool p = (par[s] >> 31) != 0 && s < valid;
    if constexpr (std::is_same_v<U, bool>) unsat |= p;
    else unsat |= (U)p << s;
  }
}

// fl_cn_item for a check of degree d in 17..kFlWideD (fl_cn_wide_body): the same fold sink, every output stored as
// soon as it is final, its row loaded as a scalar then
template <int KIND, typename F>
__device__ __forceinline__ void fl_cn_wide_item(const FlArgs& a, int node, int st, int d, int cw0, bool do_par,
                                                int valid, bool& unsat) {
  constexpr int N = Vec<F>::N;
  const F lm = (F)a.llr_max;
  int fp0 = -1, fp1 = -1, fd0 = 0, fd1 = 0;
  F c0[N], c1[N];
  if (a.fold_mode) {
    const int* fr = a.fold + (size_t)kFoldRec * node;
    fp0 = sload(fr, 0);
    fp1 = sload(fr, 1);
    fd0 = sload(fr, 2);
    fd1 = sload(fr, 3);
    if (fp0 >= 0) fl_load16<kFlNt, F>(a.ch, c0, a.ldb, sload(fr, 4), cw0);
    if (fp1 >= 0) fl_load16<kFlNt, F>(a.ch, c1, a.ldb, sload(fr, 5), cw0);
  }
  auto fold_put = [&](int w, const F (&c)[N], int row, const F (&o)[N]) __attribute__((always_inline)) {
    F f[N];
#pragma unroll
    for (int s = 0; s < N; ++s) f[s] = clampllr(c[s] + o[s], lm);
    fl_store16<kFlNt, F>(a.fout, f, a.ldb, row, cw0);
    if (a.fold_mode == 2) fl_store16<kFlNt, F>(a.out, o, a.ldb, sload(a.tgt, st + w), cw0);
  };
  F ca, cb;
  fl_correction<KIND, F>(a, ca, cb);
  uint32_t par[N];
  fl_cn_wide_body<KIND, F>(
      d, lm, ca, cb, par,
      [&](int j, F (&r)[N]) __attribute__((always_inline)) { fl_load16<kFlNt, F>(a.in, r, a.ldb, st + j, cw0); },
      [&](int w, const F (&o)[N]) __attribute__((always_inline)) {
        if (w == fp0) fold_put(w, c0, fd0, o);
        else if (w == fp1) fold_put(w, c1, fd1, o);
        else fl_store16<kFlNt, F>(a.out, o, a.ldb, sload(a.tgt, st + w), cw0);
      });
  if (do_par) fl_wide_syndrome<F>(par, valid, unsat);
}

// Variable-node body on channel c and inputs m; put(w, o) receives extrinsic output w.
template <typename F, int D, class Put>
__device__ __forceinline__ void fl_vn_body(const F (&c)[Vec<F>::N], const F (&m)[D][Vec<F>::N], F lm, Put&& put) {
  constexpr int N = Vec<F>::N;
  F o[N];
  if constexpr (D == 1) {
#pragma unroll
    for (int s = 0; s < N; ++s) o[s] = clampllr(c[s], lm);
    put(0, o);
  } else {
    // t = ch + others in ascending order (kernels_min_and_BP.cl:113-118)
    F t[N], Q[N];
#pragma unroll
    for (int s = 0; s < N; ++s) t[s] = c[s] + m[1][s];
#pragma unroll
    for (int j = 2; j < D; ++j)
#pragma unroll
      for (int s = 0; s < N; ++s) t[s] = t[s] + m[j][s];
#pragma unroll
    for (int s = 0; s < N; ++s) o[s] = clampllr(t[s], lm);
    put(0, o);
#pragma unroll
    for (int s = 0; s < N; ++s) Q[s] = c[s] + m[0][s];
#pragma unroll
    for (int w = 1; w <= D - 2; ++w) {
#pragma unroll
      for (int s = 0; s < N; ++s) t[s] = Q[s];
#pragma unroll
      for (int j = w + 1; j < D; ++j)
#pragma unroll
        for (int s = 0; s < N; ++s) t[s] = t[s] + m[j][s];
#pragma unroll
      for (int s = 0; s < N; ++s) o[s] = clampllr(t[s], lm);
      put(w, o);
#pragma unroll
      for (int s = 0; s < N; ++s) Q[s] = Q[s] + m[w][s];
    }
#pragma unroll
    for (int s = 0; s < N; ++s) o[s] = clampllr(Q[s], lm);
    put(D - 1, o);
  }
}


template <typename F, int D>
__device__ __forceinline__ void fl_vn_item(const FlArgs& a, int node, int st, int cw0) {
  using V = Vec<F>;
  constexpr int N = V::N;
  const F lm = (F)a.llr_max;
  int tg[D];   // output rows, loaded up front as scalars (the stores follow each output)
#pragma unroll
  for (int w = 0; w < D; ++w) tg[w] = sload(a.tgt, st + w);
  F c[N], m[D][N];
  fl_load16<kFlNt, F>(a.ch, c, a.ldb, node, cw0);
#pragma unroll
  for (int j = 0; j < D; ++j) fl_load16<kFlNt, F>(a.in, m[j], a.ldb, st + j, cw0);
  auto sink = [&](int w, const F (&o)[N]) __attribute__((always_inline)) {
    fl_store16<kFlNt, F>(a.out, o, a.ldb, tg[w], cw0);
  };
  FlOut<F, D> ob;
  fl_vn_body<F, D>(c, m, lm, [&](int w, const F (&o)[N]) __attribute__((always_inline)) { ob.put(w, o, sink); });
  ob.flush(sink);
}

// Threads per block of every float node kernel: the one statement of the rule, read by the kernels'
// __launch_bounds__ and by the host's launches (fl_kernel). maxd: the largest degree the kernel has a body
// for (the check degree for the fused kernel).
// MAXD = largest degree with a body in the switch (8 or 16): the registers of the degree-16 bodies
// would cap every launch's occupancy, so codes with degrees <= 8 get their own instantiation.
// 1024-thread blocks so a CU's waves share one work counter, except where the body needs more than
// the 128 VGPRs such a block allows: the box-plus check node at MAXD=16 or in fp64, and the per-pass
// fp32 min-sum check node at MAXD=16 (512 threads). The fused kernel: 1024 threads (16 waves share the
// phases) unless the check bodies need more than 128 VGPRs (check degree > 8, or fp64 box-plus). Corrected
// min-sum (kind 2) takes plain min-sum's block sizes here and in the fused kernel: its bodies need no private
// segment at either. The small-batch kernels run kFlSmallBlock threads, the per-pass decision 256.
// The wide instantiations (MAXD = kFlWideD) take the MAXD = 16 sizes, which `maxd > 8` already says: they hold the
// degree-16 bodies, and the wide body (fl_cn_wide_body) keeps no input array — its largest form, the fp32
// box-plus with 31 x 4 suffixes in registers, fits the 256 VGPRs of a 512-thread block.
constexpr int fl_block(FlFamily fam, FlPass pass, int kind, bool f64, int maxd) {
  if (fam == kFlSmall) return kFlSmallBlock;
  if (fam == kFlFused) return (maxd > 8 || (kind == 1 && f64)) ? 512 : 1024;
  if (pass == kFlDecision) return 256;
  return (pass == kFlCheck && ((kind == 1 && (maxd > 8 || f64)) || (kind != 1 && maxd > 8 && !f64))) ? 512 : 1024;
}

// The degree switch of every node kernel: calls f(std::integral_constant<int, D>{}) for the degree d of a node,
// 2 <= D <= MAXD, and for D = 1 when ONE (variable nodes); other degrees have no body and do nothing.
template <int MAXD, bool ONE, class Fn>
__device__ __forceinline__ void fl_by_degree(int d, Fn&& f) {
  switch (d) {
    case 1: if constexpr (ONE) f(std::integral_constant<int, 1>{}); break;
#define X(D) case D: if constexpr (D <= MAXD) f(std::integral_constant<int, D>{}); break;
    X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)
#undef X
    default: break;
  }
}

// The check kernels' wide instantiations (MAXD = kFlWideD) run a degree above 16 through the one wide body before this
// switch, under `if constexpr (MAXD > 16)`, so that the other instantiations hold the statements they always held;
// degrees up to 16 keep their bodies in every instantiation (fl_narrow(MAXD): the switch's largest degree).
constexpr int fl_narrow(int maxd) { return maxd > 16 ? 16 : maxd; }

// Items (node, chunk) are dealt to blocks round-robin ({b*wpb + w + nw*i}) and handed to the
// block's waves by LDS tickets (take_ticket): ticket k -> item b*wpb + k % wpb + nw * (k / wpb).
__device__ __forceinline__ int fl_next_item(int* ctr, int lane, int wpb, int nw) {
  const int k = take_ticket(ctr, lane);
  return (int)fl_bid() * wpb + (k % wpb) + nw * (k / wpb);
}

template <int KX, typename F, int MAXD>
__global__ __launch_bounds__(fl_block(kFlPerPass, kFlCheck, KX & 3, sizeof(F) == 8, MAXD)) void fl_cn(FlArgs a) {
  constexpr int KIND = KX & 3;
  static_assert(((KX & kFlWide) != 0) == (MAXD > 16), "kFlWide goes with MAXD = kFlWideD");
  const int lane = fl_tid() & 63;
  if (!fl_gate(a.gate, lane)) return;
  constexpr int CWL = Vec<F>::N;
  constexpr int CH = 64 * CWL;
  const bool do_par = a.unsat != nullptr;
  bool unsat = false;
  __shared__ int ctr;
  if (fl_tid() == 0) ctr = 0;
  __syncthreads();
  const int wpb = fl_bdim() >> 6, nw = fl_gdim() * wpb, nitems = a.n_nodes * a.nchunks;
  for (;;) {
    const int item = fl_next_item(&ctr, lane, wpb, nw);
    if (item >= nitems) break;
    const int node = __builtin_amdgcn_readfirstlane(item / a.nchunks);
    const int chunk = __builtin_amdgcn_readfirstlane(item - node * a.nchunks);
    const int d = sload(a.deg, node), st = sload(a.start, node);
    const int cw0 = chunk * CH + lane * CWL;
    const int valid = a.B - cw0;
    if constexpr (MAXD > 16) {
      if (d > 16) {
        fl_cn_wide_item<KIND, F>(a, node, st, d, cw0, do_par, valid, unsat);
        continue;
      }
    }
    fl_by_degree<fl_narrow(MAXD), false>(d, [&](auto D) __attribute__((always_inline)) {
      fl_cn_item<KIND, F, decltype(D)::value>(a, node, st, cw0, do_par, valid, unsat);
    });
  }
  if (do_par && __ballot(unsat) != 0ull && lane == 0)
    atomicOr(&a.unsat[(fl_bid() * wpb + (fl_tid() >> 6)) & (kShards - 1)], 1);
}

template <typename F, int MAXD>
__global__ __launch_bounds__(fl_block(kFlPerPass, kFlVariable, 0, sizeof(F) == 8, MAXD)) void fl_vn(FlArgs a) {
  const int lane = fl_tid() & 63;
  if (!fl_gate(a.gate, lane)) return;
  constexpr int CWL = Vec<F>::N;
  constexpr int CH = 64 * CWL;
  __shared__ int ctr;
  if (fl_tid() == 0) ctr = 0;
  __syncthreads();
  const int wpb = fl_bdim() >> 6, nw = fl_gdim() * wpb, nitems = a.n_nodes * a.nchunks;
  for (;;) {
    const int item = fl_next_item(&ctr, lane, wpb, nw);
    if (item >= nitems) break;
    const int pos = __builtin_amdgcn_readfirstlane(item / a.nchunks);
    const int chunk = __builtin_amdgcn_readfirstlane(item - pos * a.nchunks);
    const int node = a.nodes ? sload(a.nodes, pos) : pos;   // the fold's variable list skips folded nodes
    const int d = sload(a.deg, node), st = sload(a.start, node);
    const int cw0 = chunk * CH + lane * CWL;
    fl_by_degree<MAXD, true>(d, [&](auto D) __attribute__((always_inline)) {
      fl_vn_item<F, decltype(D)::value>(a, node, st, cw0);
    });
  }
}

// APP LLR = ch + sum of all inputs in ascending order, unclamped (kernels_min_and_BP.cl:196-202): x holds the
// channel values, load(k, r) fetches input k of the node's d. Before the first check pass (L == 0) there are no
// inputs: the callers run this under `if (L > 0)` (inside this helper, the test cost every fused kernel a VGPR).
template <typename F, class Load>
__device__ __forceinline__ void fl_app_sum(F (&x)[Vec<F>::N], int d, Load&& load) {
  for (int k = 0; k < d; ++k) {
    F r[Vec<F>::N];
    load(k, r);
#pragma unroll
    for (int s = 0; s < Vec<F>::N; ++s) x[s] = x[s] + r[s];
  }
}

// The lane's APP LLRs x to the user's [N][B] output at element o = node * B + cw0; `valid` = B - cw0 of them
// exist. One vector store where the output may vectorise (vec: out_aligned of the batch and the pointer) and
// all Vec<F>::N exist, else element by element. The fp64 decoders' fp32 output takes an 8-byte float2:
// vec is then out_aligned(B, out, 2, 4), B even and out % 8 == 0, and cw0 is a multiple of 2 (fused: 2 grp),
// so o is even. The fp32 decoders' fp64 output (32 bytes) always goes element by element.
template <typename F>
__device__ __forceinline__ void fl_app_store(void* out, int out_dtype, size_t o, const F (&x)[Vec<F>::N], int vec,
                                             int valid) {
  constexpr int N = Vec<F>::N;
  if (out_dtype == kF32) {
    float* p = reinterpret_cast<float*>(out) + o;
    if (vec && valid >= N) {
      if constexpr (N == 4) *reinterpret_cast<float4*>(p) = make_float4((float)x[0], (float)x[1], (float)x[2], (float)x[3]);
      else *reinterpret_cast<float2*>(p) = make_float2((float)x[0], (float)x[1]);
      return;
    }
#pragma unroll
    for (int s = 0; s < N; ++s)
      if (s < valid) p[s] = (float)x[s];
  } else {
    double* p = reinterpret_cast<double*>(out) + o;
    if constexpr (N == 2) {
      if (vec && valid >= 2) {
        *reinterpret_cast<double2*>(p) = make_double2((double)x[0], (double)x[1]);
        return;
      }
    }
#pragma unroll
    for (int s = 0; s < N; ++s)
      if (s < valid) p[s] = (double)x[s];
  }
}

// The codewords in `some` only (bit s = codeword s, a subset of the existing ones: the per-codeword stop's output of
// the codewords that stop at this pass). All Vec<F>::N of them take fl_app_store's vector store.
template <typename F>
__device__ __forceinline__ void fl_app_store_some(void* out, int out_dtype, size_t o, const F (&x)[Vec<F>::N], int vec,
                                                  int valid, uint32_t some) {
  constexpr int N = Vec<F>::N;
  if (some == (1u << N) - 1u) {
    fl_app_store<F>(out, out_dtype, o, x, vec, valid);
    return;
  }
#pragma unroll
  for (int s = 0; s < N; ++s) {
    if (!((some >> s) & 1u)) continue;
    if (out_dtype == kF32) reinterpret_cast<float*>(out)[o + s] = (float)x[s];
    else reinterpret_cast<double*>(out)[o + s] = (double)x[s];
  }
}

// Decision of the per-pass path. Wave item = (node, chunk of 64*N codewords); vector loads of every edge row,
// vector stores when the user buffer is aligned (scalar tail otherwise).
template <typename F>
__global__ __launch_bounds__(256) void fl_dec(FlDecArgs a) {
  using V = Vec<F>;
  constexpr int N = V::N, CH = 64 * N;
  const int L = __builtin_amdgcn_readfirstlane(*a.iters);
  const void* vin = (L & 1) ? a.vin1 : a.vin0;
  const int lane = fl_tid() & 63;
  const int gw = fl_bid() * (fl_bdim() >> 6) + (fl_tid() >> 6), nw = fl_gdim() * (fl_bdim() >> 6);
  const int nitems = a.n_nodes * a.nchunks;
  for (int item = gw; item < nitems; item += nw) {
    const int n = __builtin_amdgcn_readfirstlane(item / a.nchunks);
    const int chunk = __builtin_amdgcn_readfirstlane(item - n * a.nchunks);
    const int cw0 = chunk * CH + lane * N;
    if (cw0 >= a.B) continue;
    const int d = sload(a.deg, n), st = sload(a.start, n);
    F x[N];
    fl_load16<false, F>(a.ch, x, a.ldb, n, cw0);
    if (L > 0)
      fl_app_sum<F>(x, d, [&](int v, F (&r)[N]) __attribute__((always_inline)) {
        fl_load16<false, F>(vin, r, a.ldb, st + v, cw0);
      });
    fl_app_store<F>(a.out, a.out_dtype, (size_t)n * a.B + cw0, x, a.aligned, a.B - cw0);
  }
}

// Channel-LLR precondition (ibldpc.h, ibl_float_input_check), on the bit pattern of the caller's value (this
// source is built with -fno-honor-nans, under which a float compare may be folded as if NaN did not exist):
//   rule 0 checks nothing; rule 1 (min-sum) flags NaN;
//   rule 2 (BP, fp64 decoder) flags NaN and |x| > 709.089: the reference's box-plus
//     log((1 + e^(a+b)) / (e^a + e^b)) (kernels_min_and_BP.cl:5-9) is NaN once the denominator overflows beside
//     an infinite numerator (inf / inf), and the first check pass box-pluses two raw channel values: for a = b > 0
//     that is 2 e^a > DBL_MAX, i.e. a > ln(DBL_MAX / 2) = 709.0895657128241 (not ln(DBL_MAX) = 709.78, where e^a
//     alone overflows). The bound sits 5.7e-4 below it, so 2 e^|x| <= DBL_MAX e^-5.7e-4 stays finite whatever the
//     last-ulp error of the device exp. Within the bound an infinite numerator over a finite denominator, or a
//     finite numerator over a tiny one, gives +-inf or a large finite value, which the clamp maps to +-llr_max;
//   rule 3 (BP, fp32 decoder) flags NaN and +-inf of the value the decoder stages (a caller f64 beyond FLT_MAX
//     rounds to inf): the fp32 box-plus (boxplus(float, ...)) is overflow-free for every finite input.
__device__ __forceinline__ bool llr_bad(double x, int rule) {
  const uint64_t u = (uint64_t)__double_as_longlong(x) & 0x7fffffffffffffffull;
  if (rule == 3) return ((uint32_t)__float_as_uint((float)x) & 0x7fffffffu) >= 0x7f800000u;
  return rule != 0 && u > (rule == 2 ? 0x408628b645a1cac1ull /* 709.089 */ : 0x7ff0000000000000ull);
}
__device__ __forceinline__ bool llr_bad(float x, int rule) {
  const uint32_t u = __float_as_uint(x) & 0x7fffffffu;
  if (rule == 2) return llr_bad((double)x, 2);
  return rule != 0 && u >= (rule == 3 ? 0x7f800000u : 0x7f800001u);
}
// violations counted per lane (rare path: the check itself is one compare per value)
__device__ __forceinline__ void llr_count(int32_t* bad, int nb) {
  if (nb) atomicAdd(bad, nb);
}

// channel staging: user LLRs (f32/f64, [N][B]) -> F [N][ldb], zero padded, -0 stored as +0; counts inputs that
// violate the precondition of `rule` into *bad
template <typename F>
__global__ void fl_stage(const void* x, int in_dtype, int n, int B, F* dst, int ldb, int rule, int32_t* bad) {
  const size_t total = (size_t)n * ldb;
  int nb = 0;
  for (size_t i = (size_t)fl_bid() * fl_bdim() + fl_tid(); i < total; i += (size_t)fl_gdim() * fl_bdim()) {
    const int row = (int)(i / ldb);
    const int b = (int)(i - (size_t)row * ldb);
    F v = F(0);
    if (b < B) {
      const size_t k = (size_t)row * B + b;
      if (in_dtype == kF32) {
        const float xv = reinterpret_cast<const float*>(x)[k];
        nb += llr_bad(xv, rule);
        v = (F)xv;
      } else {
        const double xv = reinterpret_cast<const double*>(x)[k];
        nb += llr_bad(xv, rule);
        v = (F)xv;
      }
    }
    dst[i] = v + F(0);   // -0 -> +0 (equal values; see sign_xor)
  }
  llr_count(bad, nb);
}

// channel staging for the fused decoder: user LLRs [N][B] -> [group][variable position] 16-byte slots
// (Vec<F>::N codewords of variable perm[pos]), zero padded past B. A slot is N consecutive codewords of
// one row, so each cell is ONE 16-byte load (rows read along the codewords, 512 B per row and tile) and
// the LDS tile only transposes whole cells: 64 positions x 32 groups, rows padded by one cell (the
// position-major reads of a ds_read_b128 lane group then hit 16 distinct 4-bank groups); the slots are
// written along the positions (1 KiB per wave). Non-vector inputs (other dtype, B % N != 0, unaligned)
// load element by element.
template <typename F>
__global__ __launch_bounds__(256) void fl_stage_t(const void* x, int in_dtype, int n, int B, const int32_t* perm,
                                                  typename Vec<F>::T* dst, int rule, int32_t* bad) {
  using V = Vec<F>;
  using VT = typename V::T;
  constexpr int N = V::N, P = 64, G = 32, RW = G + 1;
  __shared__ VT tile[P * RW];
  const int ngroups = (B + N - 1) / N;
  const int ptiles = (n + P - 1) / P, gtiles = (ngroups + G - 1) / G;
  const int own = sizeof(F) == 4 ? kF32 : kF64;
  const bool vec = in_dtype == own && (B % N) == 0 && (reinterpret_cast<uintptr_t>(x) % sizeof(VT)) == 0;
  for (int t = fl_bid(); t < ptiles * gtiles; t += fl_gdim()) {
    const int p0 = (t % ptiles) * P, g0 = (t / ptiles) * G;
    __syncthreads();
    constexpr int kPer = P * G / 256;   // cells per thread, all loads issued before the LDS stores
    VT v[kPer];
    int nb = 0;
#pragma unroll
    for (int it = 0; it < kPer; ++it) {
      const int i = fl_tid() + it * 256;
      const int r = i / G, c = i - r * G;
      const int p = p0 + r, g = g0 + c;
#pragma unroll
      for (int s = 0; s < N; ++s) V::set(v[it], s, F(0));
      if (p < n && g < ngroups) {
        const size_t k = (size_t)perm[p] * B + (size_t)g * N;
        if (vec) {
          v[it] = *reinterpret_cast<const VT*>(reinterpret_cast<const F*>(x) + k);
#pragma unroll
          for (int s = 0; s < N; ++s) nb += llr_bad(V::get(v[it], s), rule);
        } else {
#pragma unroll
          for (int s = 0; s < N; ++s)
            if (g * N + s < B) {
              if (in_dtype == kF32) {
                const float xv = reinterpret_cast<const float*>(x)[k + s];
                nb += llr_bad(xv, rule);
                V::set(v[it], s, (F)xv);
              } else {
                const double xv = reinterpret_cast<const double*>(x)[k + s];
                nb += llr_bad(xv, rule);
                V::set(v[it], s, (F)xv);
              }
            }
        }
      }
    }
    llr_count(bad, nb);
#pragma unroll
    for (int it = 0; it < kPer; ++it) {
      const int i = fl_tid() + it * 256;
      const int r = i / G, c = i - r * G;
      VT o;
#pragma unroll
      for (int s = 0; s < N; ++s) V::set(o, s, V::get(v[it], s) + F(0));   // -0 -> +0 (see sign_xor)
      tile[r * RW + c] = o;
    }
    __syncthreads();
    for (int i = fl_tid(); i < P * G; i += fl_bdim()) {
      const int g = i / P, p = i - g * P;
      if (p0 + p < n && g0 + g < ngroups) dst[(size_t)(g0 + g) * n + p0 + p] = tile[p * RW + g];
    }
  }
}

// send_channel_values_to_checknode_inbox (kernels_min_and_BP.cl:12-29): scatter staged rows
template <typename F>
__global__ void fl_send(FlArgs a) {
  const F* ch = reinterpret_cast<const F*>(a.ch);
  F* dst = reinterpret_cast<F*>(a.out);
  const int per = a.ldb / 4;
  const size_t total = (size_t)a.n_nodes * per;
  for (size_t i = (size_t)fl_bid() * fl_bdim() + fl_tid(); i < total; i += (size_t)fl_gdim() * fl_bdim()) {
    const int n = (int)(i / per);
    const int b4 = (int)(i - (size_t)n * per) * 4;
    if (b4 >= a.B) continue;
    const int d = a.deg[n], st = a.start[n];
    F v[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) v[s] = ch[(size_t)n * a.ldb + b4 + s];
    for (int w = 0; w < d; ++w) {
      F* p = dst + (size_t)a.tgt[st + w] * a.ldb + b4;
#pragma unroll
      for (int s = 0; s < 4; ++s) p[s] = v[s];
    }
  }
}

// ------------------------------------------------------- small-batch per-pass kernels
// As the IB small-batch kernels (ib_kernels.hip): the per-pass kernels' wave item is one node x 64 lanes x
// Vec<F>::N codewords, so a batch of 2 costs a pass what B = 256 costs. For small batches a wave item is
// (task, word): up to 64 consecutive same-degree positions of the work order (lane = node) x one word of
// Vec<F>::N codewords, each lane gathering its node's 16-byte pieces of its rows. The node bodies are the
// per-pass kernels' (fl_cn_body / fl_vn_body on the lane's N codewords, same operations in the same order),
// so outputs equal the per-pass path's bit for bit. No fold (the small path runs every variable update).
// A task record {first position, count, degree, contiguous} with contiguous = st0 + 1 says its nodes are
// consecutive with edges st0 + k·d (every DVB-S2 task; plan.h order_tasks): the lane's first edge then needs
// no load and its node (NODE: variable passes) one scalar load per task, as in the IB small-batch kernels.
template <bool NODE, class Args, class Body>
__device__ __forceinline__ void fl_small_items(const Args& a, int lane, Body&& body) {
  const int wpb = fl_bdim() >> 6;
  const int gw = __builtin_amdgcn_readfirstlane(fl_bid() * wpb + (fl_tid() >> 6));
  const int nw = fl_gdim() * wpb, nitems = a.n_tasks * a.nwords;
  for (int item = gw; item < nitems; item += nw) {
    const int t = __builtin_amdgcn_readfirstlane(item / a.nwords);
    const int c = __builtin_amdgcn_readfirstlane(item - t * a.nwords);
    const int p0 = sload(a.task, 4 * t), cnt = sload(a.task, 4 * t + 1), d = sload(a.task, 4 * t + 2);
    const int st1 = sload(a.task, 4 * t + 3);
    if (lane < cnt) {
      int node = 0, st;
      if (st1 != 0) {   // wave-uniform
        st = st1 - 1 + lane * d;
        if constexpr (NODE) node = sload(a.info, 4 * p0) + lane;
      } else {
        st = a.info[4 * (p0 + lane) + 1];
        if constexpr (NODE) node = a.info[4 * (p0 + lane)];
      }
      body(node, st, c, d);
    }
  }
}

template <int KIND, typename F, int D>
__device__ __forceinline__ void fl_cn_small_item(const FlArgs& a, int st, int cw0, bool do_par, bool& unsat) {
  const F lm = (F)a.llr_max;
  int tg[D];
  F m[D][Vec<F>::N];
#pragma unroll
  for (int j = 0; j < D; ++j) {
    tg[j] = a.tgt[st + j];
    fl_load16<false, F>(a.in, m[j], a.ldb, st + j, cw0);
  }
  if (do_par) {
    const int valid = a.B - cw0;
#pragma unroll
    for (int s = 0; s < Vec<F>::N; ++s) unsat |= syndrome_bit<F, D>(m, s) && s < valid;
  }
  F ca, cb;
  fl_correction<KIND, F>(a, ca, cb);
  fl_cn_body<KIND, F, D>(m, lm, ca, cb, [&](int w, const F (&o)[Vec<F>::N]) __attribute__((always_inline)) {
    fl_store16<kFlNt, F>(a.out, o, a.ldb, tg[w], cw0);
  });
}

// a check of degree d in 17..kFlWideD (fl_cn_wide_body)
template <int KIND, typename F>
__device__ __forceinline__ void fl_cn_small_wide_item(const FlArgs& a, int st, int d, int cw0, bool do_par, bool& unsat) {
  constexpr int N = Vec<F>::N;
  F ca, cb;
  fl_correction<KIND, F>(a, ca, cb);
  uint32_t par[N];
  fl_cn_wide_body<KIND, F>(
      d, (F)a.llr_max, ca, cb, par,
      [&](int j, F (&r)[N]) __attribute__((always_inline)) { fl_load16<false, F>(a.in, r, a.ldb, st + j, cw0); },
      [&](int w, const F (&o)[N]) __attribute__((always_inline)) {
        fl_store16<kFlNt, F>(a.out, o, a.ldb, a.tgt[st + w], cw0);
      });
  if (do_par) fl_wide_syndrome<F>(par, a.B - cw0, unsat);
}

template <typename F, int D>
__device__ __forceinline__ void fl_vn_small_item(const FlArgs& a, int node, int st, int cw0) {
  const F lm = (F)a.llr_max;
  int tg[D];
  F c[Vec<F>::N], m[D][Vec<F>::N];
  fl_load16<false, F>(a.ch, c, a.ldb, node, cw0);
#pragma unroll
  for (int j = 0; j < D; ++j) {
    tg[j] = a.tgt[st + j];
    fl_load16<false, F>(a.in, m[j], a.ldb, st + j, cw0);
  }
  fl_vn_body<F, D>(c, m, lm, [&](int w, const F (&o)[Vec<F>::N]) __attribute__((always_inline)) {
    fl_store16<kFlNt, F>(a.out, o, a.ldb, tg[w], cw0);
  });
}

template <int KX, typename F, int MAXD>
__global__ __launch_bounds__(kFlSmallBlock) void fl_cn_small(FlArgs a) {
  constexpr int KIND = KX & 3;
  static_assert(((KX & kFlWide) != 0) == (MAXD > 16), "kFlWide goes with MAXD = kFlWideD");
  const int lane = fl_tid() & 63;
  if (!fl_gate(a.gate, lane)) return;
  const bool do_par = a.unsat != nullptr;
  bool unsat = false;
  fl_small_items<false>(a, lane, [&](int, int st, int c, int d) __attribute__((always_inline)) {
    const int cw0 = c * Vec<F>::N;
    if constexpr (MAXD > 16) {
      if (d > 16) {
        fl_cn_small_wide_item<KIND, F>(a, st, d, cw0, do_par, unsat);
        return;
      }
    }
    fl_by_degree<fl_narrow(MAXD), false>(d, [&](auto D) __attribute__((always_inline)) {
      fl_cn_small_item<KIND, F, decltype(D)::value>(a, st, cw0, do_par, unsat);
    });
  });
  if (do_par && __ballot(unsat) != 0ull && lane == 0)
    atomicOr(&a.unsat[(fl_bid() * (fl_bdim() >> 6) + (fl_tid() >> 6)) & (kShards - 1)], 1);
}

template <typename F, int MAXD>
__global__ __launch_bounds__(kFlSmallBlock) void fl_vn_small(FlArgs a) {
  const int lane = fl_tid() & 63;
  if (!fl_gate(a.gate, lane)) return;
  fl_small_items<true>(a, lane, [&](int node, int st, int c, int d) __attribute__((always_inline)) {
    const int cw0 = c * Vec<F>::N;
    fl_by_degree<MAXD, true>(d, [&](auto D) __attribute__((always_inline)) {
      fl_vn_small_item<F, decltype(D)::value>(a, node, st, cw0);
    });
  });
}

// APP LLR of the small path: ch + every input in ascending edge order, unclamped (as fl_dec)
template <typename F>
__global__ __launch_bounds__(kFlSmallBlock) void fl_dec_small(FlDecArgs a) {
  const int L = __builtin_amdgcn_readfirstlane(*a.iters);
  const void* vin = (L & 1) ? a.vin1 : a.vin0;
  const int lane = fl_tid() & 63;
  fl_small_items<true>(a, lane, [&](int node, int st, int c, int d) __attribute__((always_inline)) {
    const int cw0 = c * Vec<F>::N;
    F x[Vec<F>::N];
    fl_load16<false, F>(a.ch, x, a.ldb, node, cw0);
    if (L > 0)
      fl_app_sum<F>(x, d, [&](int v, F (&r)[Vec<F>::N]) __attribute__((always_inline)) {
        fl_load16<false, F>(vin, r, a.ldb, st + v, cw0);
      });
    // element stores only: this path never sets FlDecArgs::aligned
    fl_app_store<F>(a.out, a.out_dtype, (size_t)node * a.B + cw0, x, 0, a.B - cw0);
  });
}

// ------------------------------------------------------------ fused on-chip decoder
// For codes whose messages fit in LDS ((E + N) * 16 B <= 160 KiB, e.g. WLAN N=1944: 142.6 KB), one
// workgroup decodes Vec<F>::N codewords (4 fp32 / 2 fp64, one 16-byte slot per edge and per
// variable) through ALL iterations without touching HBM: the flooding schedule of
// decode_OpenCL_min_sum / decode_OpenCL_belief_propagation (min_sum_decoder_irreg.py:221-287,
// bp_decoder_irreg.py:221-286) as barrier-separated phases over one in-place message array:
//   send (kernels_min_and_BP.cl:12-29); for j = 1..L { CN pass (+ syndrome of its inputs, :206-227);
//   VN pass (:76-123) unless j == L }; APP output (:170-204) from the last CN pass.
// Check and variable nodes own their slots (a node reads all its inputs before writing its outputs
// to the same slots), so one array serves both directions. Node bodies are the per-pass kernels'
// (fl_cn_body / fl_vn_body), same operations in the same order: outputs equal the per-pass path's
// bit for bit. Work inside a phase: tasks of up to 64 same-degree nodes, heaviest first, handed to
// waves by LDS tickets; two counters alternate between phases (reset one phase ahead).
// Early stop is batch-global in the reference (stop when the WHOLE batch's syndrome is zero): pass 1
// runs imax-1 iterations and records each CN pass's syndrome in the same flag words as the per-pass
// path; finalize_iters turns them into L; pass 2 (dL set) re-runs the batch to L only if L < imax-1.
// A message slot holds Vec<F>::N codewords (16 bytes), and a task works on whole slots.
// Per-codeword stop (kFlEach, ibldpc.h "Per-codeword stop"): one pass over the batch. The stop of iteration i is the
// syndrome of variable pass i's outputs, which check pass i + 1 reads — after variable pass i has overwritten, in
// place, the check messages that the APP output of iteration i sums. So every variable pass i also stores the APP
// LLRs of the codewords still running to the user's output (fused_vn_app_item), a later pass of the same codeword
// overwrites them (the barriers between the phases wait for the stores), and a codeword that check pass i + 1 finds
// satisfied keeps what variable pass i stored and gets iters = i. Check pass j >= 2 reduces its syndrome to a
// mask of the group's unsatisfied codewords in an LDS word (two words after the ticket counters, word j & 1 for pass
// j, reset one check pass ahead as the counters are), every wave reads that word after the barrier, and the
// workgroup leaves the group once no codeword is running; those still running after check pass imax-1 take the
// output phase and iters = imax-1.
// unsat: bool (some codeword of the slot unsatisfied, the batch-global stop) or uint32_t (bit s = codeword s
// unsatisfied, the per-codeword stop)
template <int KIND, typename F, int D, int CNT = 0, class U>
__device__ __forceinline__ void fused_cn_item(typename Vec<F>::T* msg, int first, int cnt_, int lane, F lm, F ca, F cb,
                                              bool do_par, int valid, U& unsat) {
  constexpr int N = Vec<F>::N;
  // CNT > 0: a full task (CNT nodes) — the edge stride is a constant, so one address register serves all
  // D loads and stores through their immediate offsets
  const int cnt = CNT > 0 ? CNT : cnt_;
  F m[D][N];
#pragma unroll
  for (int j = 0; j < D; ++j) fl_load16<false, F>(msg + (first + j * cnt + lane), m[j]);
  if (do_par) {
#pragma unroll
    for (int s = 0; s < N; ++s) {
      if constexpr (std::is_same_v<U, bool>) unsat |= syndrome_bit<F, D>(m, s) && s < valid;
      else unsat |= (U)(syndrome_bit<F, D>(m, s) && s < valid) << s;
    }
  }
  fl_cn_body<KIND, F, D>(m, lm, ca, cb, [&](int w, const F (&o)[N]) __attribute__((always_inline)) {
    fl_store16<false, F>(msg + (first + w * cnt + lane), o);
  });
}

// a check of degree d in 17..kFlWideD (fl_cn_wide_body), in place: the body loads input w before it puts output w,
// and the inputs it loads again lie above the outputs already stored
template <int KIND, typename F, class U>
__device__ __forceinline__ void fused_cn_wide_item(typename Vec<F>::T* msg, int first, int cnt, int d, int lane, F lm,
                                                   F ca, F cb, bool do_par, int valid, U& unsat) {
  constexpr int N = Vec<F>::N;
  typename Vec<F>::T* p = msg + (first + lane);
  uint32_t par[N];
  fl_cn_wide_body<KIND, F>(
      d, lm, ca, cb, par,
      [&](int j, F (&r)[N]) __attribute__((always_inline)) { fl_load16<false, F>(p + j * cnt, r); },
      [&](int w, const F (&o)[N]) __attribute__((always_inline)) { fl_store16<false, F>(p + w * cnt, o); });
  if (do_par) fl_wide_syndrome<F>(par, valid, unsat);
}

// Variable-edge slot indices: staged into LDS as 16-bit values beside the messages (the fused path
// requires the room for them, capi_float.hip fused_setup), row k of a task at sfirst + 64k: the D loads share
// one address and take their row offsets as immediates.
template <typename F, int D>
__device__ __forceinline__ void fused_vn_item(typename Vec<F>::T* msg, const typename Vec<F>::T* chL,
                                              const uint16_t* vn_slot, int pos, int sfirst, int lane, F lm) {
  constexpr int N = Vec<F>::N;
  int sl[D];
#pragma unroll
  for (int k = 0; k < D; ++k) sl[k] = vn_slot[sfirst + 64 * k + lane];
  F c[N], m[D][N];
  fl_load16<false, F>(chL + pos, c);
#pragma unroll
  for (int k = 0; k < D; ++k) fl_load16<false, F>(msg + sl[k], m[k]);
  fl_vn_body<F, D>(c, m, lm, [&](int w, const F (&o)[N]) __attribute__((always_inline)) {
    fl_store16<false, F>(msg + sl[w], o);
  });
}

// Per-codeword stop: the variable update, and before it the APP LLRs of the same inputs (fl_app_sum's order: the
// channel, then the edges ascending) of the running codewords `run` to the user's output at element o.
template <typename F, int D>
__device__ __forceinline__ void fused_vn_app_item(typename Vec<F>::T* msg, const typename Vec<F>::T* chL,
                                                  const uint16_t* vn_slot, int pos, int sfirst, int lane, F lm,
                                                  void* out, int out_dtype, size_t o, int vec, int valid, uint32_t run) {
  constexpr int N = Vec<F>::N;
  if constexpr (D > 8) {
    // the variable body of these degrees fills the 128 registers of a 1024-thread block: the APP sum reads the
    // inputs on its own first, four at a time (few variables have such degrees)
    F x[N];
    fl_load16<false, F>(chL + pos, x);
#pragma unroll 4
    for (int k = 0; k < D; ++k) {
      F r[N];
      fl_load16<false, F>(msg + vn_slot[sfirst + 64 * k + lane], r);
#pragma unroll
      for (int s = 0; s < N; ++s) x[s] = x[s] + r[s];
    }
    fl_app_store_some<F>(out, out_dtype, o, x, vec, valid, run);
    __builtin_amdgcn_sched_barrier(0);   // the sum's registers are free before the body's are taken
    fused_vn_item<F, D>(msg, chL, vn_slot, pos, sfirst, lane, lm);
    return;
  }
  int sl[D];
#pragma unroll
  for (int k = 0; k < D; ++k) sl[k] = vn_slot[sfirst + 64 * k + lane];
  F c[N], m[D][N], x[N];
  fl_load16<false, F>(chL + pos, c);
#pragma unroll
  for (int k = 0; k < D; ++k) fl_load16<false, F>(msg + sl[k], m[k]);
#pragma unroll
  for (int s = 0; s < N; ++s) x[s] = c[s];
#pragma unroll
  for (int k = 0; k < D; ++k) {
#pragma unroll
    for (int s = 0; s < N; ++s) x[s] = x[s] + m[k][s];
  }
  fl_app_store_some<F>(out, out_dtype, o, x, vec, valid, run);
  __builtin_amdgcn_sched_barrier(0);   // the store's registers are free before the body's are taken
  fl_vn_body<F, D>(c, m, lm, [&](int w, const F (&o2)[N]) __attribute__((always_inline)) {
    fl_store16<false, F>(msg + sl[w], o2);
  });
}

// CMAX / VMAX: largest check / variable degree with a body (WLAN: checks <= 8, variables up to 11 ->
// fl_fused<.., 8, 16>, without the 16-input check bodies' registers)
// KX: the check-body kind, plus kFlEach for the per-codeword-stop form (a bit of the kind and not a further
// parameter, so that the instantiations without it keep their symbols)
constexpr int kFlEach = 4;
template <int KX, typename F, int CMAX, int VMAX>
__global__ __launch_bounds__(fl_block(kFlFused, kFlCheck, KX & 3, sizeof(F) == 8, CMAX)) void fl_fused(FlFusedArgs a) {
  constexpr int KIND = KX & 3;
  constexpr bool EACH = (KX & kFlEach) != 0;
  static_assert(((KX & kFlWide) != 0) == (CMAX > 16), "kFlWide goes with CMAX = kFlWideD");
  using V = Vec<F>;
  using VT = typename V::T;
  constexpr int N = V::N;
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  VT* msg = reinterpret_cast<VT*>(lds);
  VT* chL = msg + a.n_e;
  int* ctr = reinterpret_cast<int*>(chL + a.n_v);
  const int lane = fl_tid() & 63;
  const F lm = (F)a.llr_max;
  F ca, cb;
  fl_correction<KIND, F>(a, ca, cb);
  int L = a.imax - 1;
  if (a.dL) {
    L = __builtin_amdgcn_readfirstlane(*a.dL);
    if (L >= a.imax - 1) return;   // no early stop happened: pass 1's outputs stand
  }
  if (fl_tid() < 2) ctr[fl_tid()] = 0;
  // variable-edge slot indices, [ctr x 4][n_vs x u16] after the channel slots
  uint16_t* vs = reinterpret_cast<uint16_t*>(ctr + 4);
  for (int i = fl_tid(); i < a.n_vs; i += fl_bdim()) vs[i] = (uint16_t)a.vn_slot[i];
  __syncthreads();
  int ph = 0;
  const int shard = (int)((fl_bid() * (fl_bdim() >> 6) + (fl_tid() >> 6)) & (kShards - 1));
  // one phase: tasks dealt by ticket; the next phase's counter is reset while this one runs
#ifndef IBL_FUSED_TRACE
#define IBL_FUSED_TRACE 0
#endif
  // phase trace of block 0's first group (diagnostic builds): kFlTraceWords per phase (common.h)
  const int wv = fl_tid() >> 6;
  constexpr int TW = kFlTraceWords;
  uint64_t* tr = (IBL_FUSED_TRACE && a.trace && fl_bid() == 0 && lane == 0) ? a.trace : nullptr;
  if (IBL_FUSED_TRACE && tr && wv == 0) tr[0] = __builtin_readcyclecounter();
  // ---- task bodies (one task = up to 64 same-degree nodes, lane i = node i) ----
  // send: every variable's channel slot and its edge slots
  auto send_task = [&](int t, int grp) __attribute__((always_inline)) {
    const int pos = sload(a.vn_task, 4 * t), cnt = sload(a.vn_task, 4 * t + 1);
    const int d = sload(a.vn_task, 4 * t + 2), sf = sload(a.vn_task, 4 * t + 3);
    if (lane < cnt) {
      // channel staged as [group][variable position] (fl_stage_t): a task reads consecutive slots
      const VT c = reinterpret_cast<const VT*>(a.ch)[(size_t)grp * a.n_v + pos + lane];
      chL[pos + lane] = c;
      for (int k = 0; k < d; ++k) msg[vs[sf + 64 * k + lane]] = c;
    }
  };
  auto cn_task = [&](int t, int valid, bool do_par, auto& unsat) __attribute__((always_inline)) {
    const int first = sload(a.cn_task, 4 * t), cnt = sload(a.cn_task, 4 * t + 1), d = sload(a.cn_task, 4 * t + 2);
    // full tasks (64 nodes) run a body with the constant edge stride; it exists for degrees <= 8 only, and full
    // tasks of larger degrees take the general branch below (every lane < cnt = 64)
    if (cnt == 64 && d <= 8) {
      fl_by_degree<(CMAX < 8 ? CMAX : 8), false>(d, [&](auto D) __attribute__((always_inline)) {
        fused_cn_item<KIND, F, decltype(D)::value, 64>(msg, first, cnt, lane, lm, ca, cb, do_par, valid, unsat);
      });
    } else if (lane < cnt) {
      if constexpr (CMAX > 16) {
        if (d > 16) {
          fused_cn_wide_item<KIND, F>(msg, first, cnt, d, lane, lm, ca, cb, do_par, valid, unsat);
          return;
        }
      }
      fl_by_degree<fl_narrow(CMAX), false>(d, [&](auto D) __attribute__((always_inline)) {
        fused_cn_item<KIND, F, decltype(D)::value>(msg, first, cnt, lane, lm, ca, cb, do_par, valid, unsat);
      });
    }
  };
  auto vn_task = [&](int t) __attribute__((always_inline)) {
    const int pos = sload(a.vn_task, 4 * t), cnt = sload(a.vn_task, 4 * t + 1);
    const int d = sload(a.vn_task, 4 * t + 2), sf = sload(a.vn_task, 4 * t + 3);
    if (lane < cnt) {
      fl_by_degree<VMAX, true>(d, [&](auto D) __attribute__((always_inline)) {
        fused_vn_item<F, decltype(D)::value>(msg, chL, vs, pos + lane, sf, lane, lm);
      });
    }
  };
  // APP output: ch + all inputs of the last CN pass in ascending edge order, unclamped
  auto out_task = [&](int t, int cw0, int valid) __attribute__((always_inline)) {
    const int pos = sload(a.vn_task, 4 * t), cnt = sload(a.vn_task, 4 * t + 1);
    const int d = sload(a.vn_task, 4 * t + 2), sf = sload(a.vn_task, 4 * t + 3);
    if (lane < cnt) {
      const int node = a.vn_node[pos + lane];
      F x[N];
      fl_load16<false, F>(chL + pos + lane, x);
      if (L > 0)
        fl_app_sum<F>(x, d, [&](int k, F (&r)[N]) __attribute__((always_inline)) {
          fl_load16<false, F>(msg + vs[sf + 64 * k + lane], r);
        });
      fl_app_store<F>(a.out, a.out_dtype, (size_t)node * a.B + cw0, x, a.aligned, valid);
    }
  };
  // per-codeword stop: the variable pass that also stores the running codewords' APP output
  auto vn_app_task = [&](int t, int cw0, int valid, uint32_t run) __attribute__((always_inline)) {
    const int pos = sload(a.vn_task, 4 * t), cnt = sload(a.vn_task, 4 * t + 1);
    const int d = sload(a.vn_task, 4 * t + 2), sf = sload(a.vn_task, 4 * t + 3);
    if (lane < cnt) {
      const size_t o = (size_t)a.vn_node[pos + lane] * a.B + cw0;
      fl_by_degree<VMAX, true>(d, [&](auto D) __attribute__((always_inline)) {
        fused_vn_app_item<F, decltype(D)::value>(msg, chL, vs, pos + lane, sf, lane, lm, a.out, a.out_dtype, o,
                                                 a.aligned, valid, run);
      });
    }
  };
  // per-codeword stop: the APP output of the codewords in `some` from the last check pass (sum) or, with imax = 1,
  // from the channel alone
  auto out_some_task = [&](int t, int cw0, int valid, uint32_t some, bool sum) __attribute__((always_inline)) {
    const int pos = sload(a.vn_task, 4 * t), cnt = sload(a.vn_task, 4 * t + 1);
    const int d = sload(a.vn_task, 4 * t + 2), sf = sload(a.vn_task, 4 * t + 3);
    if (lane < cnt) {
      const int node = a.vn_node[pos + lane];
      F x[N];
      fl_load16<false, F>(chL + pos + lane, x);
      if (sum)
        fl_app_sum<F>(x, d, [&](int k, F (&r)[N]) __attribute__((always_inline)) {
          fl_load16<false, F>(msg + vs[sf + 64 * k + lane], r);
        });
      fl_app_store_some<F>(a.out, a.out_dtype, (size_t)node * a.B + cw0, x, a.aligned, valid, some);
    }
  };

  // ---- phases separated by barriers: the tasks (phase_run), then the barrier (phase_end)
  auto phase_run = [&](int ntasks, auto&& body) __attribute__((always_inline)) {
    int* c = ctr + (ph & 1);
    if (fl_tid() == 0) ctr[(ph + 1) & 1] = 0;
    int taken = 0;
    for (;;) {
      const int t = take_ticket(c, lane);
      if (t >= ntasks) break;
      if constexpr (IBL_FUSED_TRACE) {
        if (tr && taken == 0) tr[TW * ph + 33 + wv] = __builtin_readcyclecounter();
      }
      body(t);
      if constexpr (IBL_FUSED_TRACE) {
        if (tr && taken == 0) tr[TW * ph + 49 + wv] = __builtin_readcyclecounter();
      }
      ++taken;
    }
    if constexpr (IBL_FUSED_TRACE) {
      if (tr) {
        tr[TW * ph + 1 + wv] = __builtin_readcyclecounter();
        tr[TW * ph + 17 + wv] = (uint64_t)taken;
      }
    }
  };
  auto phase_end = [&]() __attribute__((always_inline)) {
    __syncthreads();
    ++ph;
    if constexpr (IBL_FUSED_TRACE) {
      if (tr && wv == 0) tr[TW * ph] = __builtin_readcyclecounter();
    }
  };
  auto phase = [&](int ntasks, auto&& body) __attribute__((always_inline)) {
    phase_run(ntasks, body);
    phase_end();
  };
  if constexpr (EACH) {
    int* um = ctr + 2;   // unsatisfied-codeword masks: word j & 1 for check pass j
    const int Lm = a.imax - 1;
    for (int grp = fl_bid(); grp < a.ngroups; grp += fl_gdim()) {
      const int cw0 = grp * N;
      const int valid = a.B - cw0;
      // codewords still running (workgroup-uniform: scalars and the LDS word only); columns past the batch never are
      uint32_t run = valid >= N ? (1u << N) - 1u : (1u << valid) - 1u;
      auto set_iters = [&](uint32_t some, int it) __attribute__((always_inline)) {
        if (a.iters && fl_tid() < N && ((some >> fl_tid()) & 1u)) a.iters[cw0 + fl_tid()] = it;
      };
      phase(a.n_vn_tasks, [&](int t) __attribute__((always_inline)) { send_task(t, grp); });
      for (int j = 1; j <= Lm; ++j) {
        // check pass j >= 2 holds the stop of iteration j - 1 (pass 1 reads the channel: no stop)
        const bool do_par = j >= 2;
        uint32_t un = 0;
        if (fl_tid() == 0) um[(j + 1) & 1] = 0;
        phase_run(a.n_cn_tasks, [&](int t) __attribute__((always_inline)) { cn_task(t, valid, do_par, un); });
        if (do_par) {
          uint32_t w = 0;
#pragma unroll
          for (int s = 0; s < N; ++s) w |= __ballot((un >> s) & 1u) != 0ull ? 1u << s : 0u;
          if (w != 0 && lane == 0) atomicOr(&um[j & 1], (int)w);
        }
        phase_end();
        if (do_par) {   // satisfied: variable pass j - 1 stored their output
          const uint32_t done = run & ~(uint32_t)__builtin_amdgcn_readfirstlane(um[j & 1]);
          set_iters(done, j - 1);
          run &= ~done;
          if (run == 0) break;
        }
        if (j == Lm) break;
        phase(a.n_vn_tasks, [&](int t) __attribute__((always_inline)) { vn_app_task(t, cw0, valid, run); });
      }
      if (run != 0) {   // still running after check pass imax-1 (or imax = 1: the channel alone)
        set_iters(run, Lm);
        phase(a.n_vn_tasks, [&](int t) __attribute__((always_inline)) { out_some_task(t, cw0, valid, run, Lm > 0); });
      }
    }
    return;
  }
  for (int grp = fl_bid(); grp < a.ngroups; grp += fl_gdim()) {
    const int cw0 = grp * N;
    const int valid = a.B - cw0;
    phase(a.n_vn_tasks, [&](int t) __attribute__((always_inline)) { send_task(t, grp); });
    for (int j = 1; j <= L; ++j) {
      const bool do_par = a.unsat != nullptr;
      bool unsat = false;
      phase(a.n_cn_tasks, [&](int t) __attribute__((always_inline)) { cn_task(t, valid, do_par, unsat); });
      if (do_par && __ballot(unsat) != 0ull && lane == 0) atomicOr(&a.unsat[(size_t)(j - 1) * kShards + shard], 1);
      if (j == L) break;
      phase(a.n_vn_tasks, [&](int t) __attribute__((always_inline)) { vn_task(t); });
    }
    phase(a.n_vn_tasks, [&](int t) __attribute__((always_inline)) { out_task(t, cw0, valid); });
    tr = nullptr;   // trace the first group only
  }
}

// ---------------------------------------------------------------------- launchers
hipError_t launch_fl_stage(const void* x, int in_dtype, int n, int B, void* dst, int prec, int ldb, int rule,
                           int32_t* bad, hipStream_t s) {
  const size_t total = (size_t)n * ldb;
  const int grid = (int)std::min<size_t>((total + 255) / 256, 8192);
  if (prec == kF32)
    hipLaunchKernelGGL(fl_stage<float>, dim3(grid), dim3(256), 0, s, x, in_dtype, n, B, (float*)dst, ldb, rule, bad);
  else
    hipLaunchKernelGGL(fl_stage<double>, dim3(grid), dim3(256), 0, s, x, in_dtype, n, B, (double*)dst, ldb, rule, bad);
  return hipGetLastError();
}

hipError_t launch_fl_stage_t(const void* x, int in_dtype, int n, int B, const int32_t* perm, void* dst, int prec,
                             int rule, int32_t* bad, hipStream_t s) {
  const int cwl = fl_cw_per_lane(prec);
  const size_t tiles = (size_t)((n + 63) / 64) * (size_t)((((B + cwl - 1) / cwl) + 31) / 32);
  const int grid = (int)std::max<size_t>(1, std::min<size_t>(tiles, 8192));
  if (prec == kF32)
    hipLaunchKernelGGL(fl_stage_t<float>, dim3(grid), dim3(256), 0, s, x, in_dtype, n, B, perm, (float4*)dst, rule, bad);
  else
    hipLaunchKernelGGL(fl_stage_t<double>, dim3(grid), dim3(256), 0, s, x, in_dtype, n, B, perm, (double2*)dst, rule, bad);
  return hipGetLastError();
}

// Host-side operand checks before a launch: a missing array would fault the device, not fail the call.
static bool fl_args_ok(FlFamily fam, FlPass pass, const FlArgs& a) {
  if (fam == kFlSmall)
    return a.info && a.task && a.in && a.out && a.tgt && (pass != kFlVariable || a.ch) && a.nwords >= 1 && a.ldb > 0 &&
           a.B > 0;
  if (!a.out || !a.start || !a.deg || !a.tgt || a.ldb <= 0 || a.n_nodes < 0 || a.B <= 0 || a.B > a.ldb) return false;
  if (pass == kFlCheck) return a.in && (a.fold_mode == 0 || (a.fold && a.fout && a.ch));
  if (pass == kFlVariable) return a.in && a.ch;
  return a.ch != nullptr;   // send
}

hipError_t launch_fl_send(const FlArgs& a, int prec, hipStream_t s) {
  if (!fl_args_ok(kFlPerPass, kFlSend, a)) return hipErrorInvalidValue;
  const size_t total = (size_t)a.n_nodes * (a.ldb / 4);
  const int grid = (int)std::min<size_t>((total + 255) / 256, 8192);
  if (prec == kF32) hipLaunchKernelGGL(fl_send<float>, dim3(grid), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(fl_send<double>, dim3(grid), dim3(256), 0, s, a);
  return hipGetLastError();
}

// The one table of the node and decision kernels: entry point, threads per block (fl_block) and name of the
// kernel of (family, pass, check-body kind, precision, largest check / variable degree). Degrees <= 8 take the
// MAXD = 8 instantiations, a largest check degree above 16 the check and fused kernels' MAXD = kFlWideD ones (wide
// handles); the fused kernel is one kernel for every pass.
struct FlKernel {
  const void* fn;
  int block;
  const char* name;
};
template <int KIND, typename F>
static const void* fl_entry(FlFamily fam, FlPass pass, bool c8, bool v8, bool each, bool wide) {
  if (wide) {   // a check of degree 17..kFlWideD: the check kernels' wide column (the others have no check body)
    constexpr int KW = KIND | kFlWide;
    if (fam == kFlFused)
      return each ? (const void*)fl_fused<KW | kFlEach, F, kFlWideD, 16> : (const void*)fl_fused<KW, F, kFlWideD, 16>;
    if (pass == kFlCheck)
      return fam == kFlSmall ? (const void*)fl_cn_small<KW, F, kFlWideD> : (const void*)fl_cn<KW, F, kFlWideD>;
  }
  if (fam == kFlFused && each)
    return !c8 ? (const void*)fl_fused<KIND | kFlEach, F, 16, 16>
               : v8 ? (const void*)fl_fused<KIND | kFlEach, F, 8, 8> : (const void*)fl_fused<KIND | kFlEach, F, 8, 16>;
  if (fam == kFlFused)
    return !c8 ? (const void*)fl_fused<KIND, F, 16, 16>
               : v8 ? (const void*)fl_fused<KIND, F, 8, 8> : (const void*)fl_fused<KIND, F, 8, 16>;
  if (fam == kFlSmall) {
    if (pass == kFlCheck) return c8 ? (const void*)fl_cn_small<KIND, F, 8> : (const void*)fl_cn_small<KIND, F, 16>;
    if (pass == kFlVariable) return v8 ? (const void*)fl_vn_small<F, 8> : (const void*)fl_vn_small<F, 16>;
    return (const void*)fl_dec_small<F>;
  }
  if (pass == kFlCheck) return c8 ? (const void*)fl_cn<KIND, F, 8> : (const void*)fl_cn<KIND, F, 16>;
  if (pass == kFlVariable) return v8 ? (const void*)fl_vn<F, 8> : (const void*)fl_vn<F, 16>;
  return (const void*)fl_dec<F>;
}
static FlKernel fl_kernel(FlFamily fam, FlPass pass, int kind, int prec, int cmax, int vmax, bool each = false) {
  static const char* const names[3][3] = {
      {"fl_cn", "fl_vn", "fl_dec"}, {"fl_cn_small", "fl_vn_small", "fl_dec_small"}, {"fl_fused", "fl_fused", "fl_fused"}};
  const bool f64 = prec != kF32, c8 = cmax <= 8, v8 = vmax <= 8, wd = cmax > 16;
  const void* fn =
      kind == 0 ? (f64 ? fl_entry<0, double>(fam, pass, c8, v8, each, wd) : fl_entry<0, float>(fam, pass, c8, v8, each, wd))
      : kind == kFlCorrected
          ? (f64 ? fl_entry<2, double>(fam, pass, c8, v8, each, wd) : fl_entry<2, float>(fam, pass, c8, v8, each, wd))
          : (f64 ? fl_entry<1, double>(fam, pass, c8, v8, each, wd) : fl_entry<1, float>(fam, pass, c8, v8, each, wd));
  const int maxd = (fam == kFlFused || pass == kFlCheck) ? cmax : vmax;
  return {fn, fl_block(fam, pass, kind, f64, maxd), each ? "fl_fused (per-codeword stop)" : names[fam][pass]};
}
template <class Args>
static hipError_t fl_launch(const FlKernel& k, const Args& a, int grid, size_t lds, hipStream_t s) {
  Args args = a;
  void* p[] = {&args};
  return hipLaunchKernel(k.fn, dim3(grid), dim3(k.block), p, lds, s);
}

hipError_t launch_fl_pass(FlFamily fam, FlPass pass, const FlArgs& a, int kind, int prec, int maxd, int grid,
                          hipStream_t s) {
  if (!fl_args_ok(fam, pass, a)) return hipErrorInvalidValue;
  return fl_launch(fl_kernel(fam, pass, kind, prec, maxd, maxd), a, grid, 0, s);
}

hipError_t launch_fl_dec(FlFamily fam, const FlDecArgs& a, int prec, int grid, hipStream_t s) {
  if (fam == kFlSmall && (!a.info || !a.task || !a.vin0 || !a.vin1 || !a.ch || !a.out || a.nwords < 1))
    return hipErrorInvalidValue;
  return fl_launch(fl_kernel(fam, kFlDecision, 0, prec, 0, 0), a, grid, 0, s);
}

hipError_t launch_fl_fused(const FlFusedArgs& a, int kind, int prec, int cmax, int vmax, int grid, size_t lds,
                           hipStream_t s, bool each) {
  return fl_launch(fl_kernel(kFlFused, kFlCheck, kind, prec, cmax, vmax, each), a, grid, lds, s);
}

hipError_t fl_occupancy(FlFamily fam, FlPass pass, int kind, int prec, int cmax, int vmax, size_t lds,
                        int* blocks_per_cu, int* block, bool each) {
  const FlKernel k = fl_kernel(fam, pass, kind, prec, cmax, vmax, each);
  *block = k.block;
  if (fam == kFlFused) {
    const hipError_t e = hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
    if (e != hipSuccess) return e;
  }
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, k.fn, k.block, lds);
}

hipError_t fl_private_bytes(FlFamily fam, int kind, int prec, int cn_maxd, int vn_maxd, bool fused, size_t* bytes,
                            const char** name) {
  FlKernel ks[4] = {fl_kernel(fam, kFlCheck, kind, prec, cn_maxd, vn_maxd),
                    fl_kernel(fam, kFlVariable, kind, prec, cn_maxd, vn_maxd), {}, {}};
  if (fam == kFlSmall) ks[2] = fl_kernel(fam, kFlDecision, kind, prec, 0, 0);
  else if (fused) {   // both forms of the fused kernel: batch stop and per-codeword stop
    ks[2] = fl_kernel(kFlFused, kFlCheck, kind, prec, cn_maxd, vn_maxd);
    ks[3] = fl_kernel(kFlFused, kFlCheck, kind, prec, cn_maxd, vn_maxd, true);
  }
  *bytes = 0;
  *name = "";
  for (const FlKernel& k : ks) {
    if (!k.fn) continue;
    hipFuncAttributes fa;
    const hipError_t e = hipFuncGetAttributes(&fa, k.fn);
    if (e != hipSuccess) return e;
    if (fa.localSizeBytes > *bytes) {
      *bytes = fa.localSizeBytes;
      *name = k.name;
    }
  }
  return hipSuccess;
}

}  // namespace ibl
