// The layered BP check core, the one statement of the check update for the fp32 kernels (layered_bp_kernels.hip) and
// the half-precision-state kernels (layered_half_kernels.hip). Device code only; include after common.h, boxplus.h and
// layered_plan.h.
#pragma once

#include <type_traits>

namespace ibl {

#define LAYBP_CASES                                                                                            \
  LAY_CASE(2) LAY_CASE(3) LAY_CASE(4) LAY_CASE(5) LAY_CASE(6) LAY_CASE(7) LAY_CASE(8) LAY_CASE(9) LAY_CASE(10) \
  LAY_CASE(11) LAY_CASE(12) LAY_CASE(13) LAY_CASE(14) LAY_CASE(15) LAY_CASE(16)

// store_r(k, x) and the message that enters P: a store_r that returns nothing keeps x as it is (fp32 state); one that
// returns a float has rounded x to its storage format and gives the rounded value back (half state: P = Q + f(h(R'))).
template <class StoreR>
__device__ __forceinline__ float lay_bp_put(StoreR& store_r, int k, float x) {
  if constexpr (std::is_void_v<decltype(store_r(k, x))>) {
    store_r(k, x);
    return x;
  } else {
    return store_r(k, x);
  }
}

// The BP check update of one check of degree D, the one statement of it for both kernels: load_p(k) is P of edge k,
// load_r(k) its R of the previous iteration, store_p / store_r(k, x) write the new ones back; all four are called
// inside the unrolled loops, so a caller's memory accesses sit where the arithmetic uses them. S_j and F are box-plus
// results and so lie inside the clamp; only the degree-2 messages, which are copies of Q, need a clamp of their own.
// 3 (D - 2) box-pluses.
template <int D, class LoadP, class LoadR, class StoreP, class StoreR>
__device__ __forceinline__ void lay_bp(LoadP load_p, LoadR load_r, StoreP store_p, StoreR store_r, float L) {
  static_assert(D >= kLayMinD && D <= kLayBpMaxD, "degree body out of range");
  float q[D];
#pragma unroll
  for (int k = 0; k < D; ++k) q[k] = load_p(k) - load_r(k);
  if constexpr (D == 2) {
    const float r0 = __builtin_amdgcn_fmed3f(q[1], -L, L), r1 = __builtin_amdgcn_fmed3f(q[0], -L, L);
    store_p(0, q[0] + lay_bp_put(store_r, 0, r0));
    store_p(1, q[1] + lay_bp_put(store_r, 1, r1));
  } else {
    float S[D];   // S[j] = Q_j [+] ... [+] Q_{D-1}, j >= 1
    S[D - 1] = q[D - 1];
#pragma unroll
    for (int j = D - 2; j >= 1; --j) S[j] = boxplus(q[j], S[j + 1], L);
    store_p(0, q[0] + lay_bp_put(store_r, 0, S[1]));
    float F = q[0];   // Q_0 [+] ... [+] Q_{w-1}
#pragma unroll
    for (int w = 1; w <= D - 2; ++w) {
      const float r = boxplus(F, S[w + 1], L);
      store_p(w, q[w] + lay_bp_put(store_r, w, r));
      F = boxplus(q[w], F, L);
    }
    store_p(D - 1, q[D - 1] + lay_bp_put(store_r, D - 1, F));
  }
}

}  // namespace ibl
