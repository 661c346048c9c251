// Device self-test: ONE field / group-law primitive per lane, on operands the caller chose (mi355zk_selftest_dev_op, include/mi355zk.h).
//
// TEST INFRASTRUCTURE.  The host hooks of field_ops.hip run fieldu.hpp / curveu.hpp compiled for the host; this runs the gfx950 object code
// of the same headers, and the code that exists in the device pass only: Fp::mul (mont_mul_gfx950.inc), the quad- and pair-per-bucket
// additions (DPP permutes).  Every primitive is called as the product kernels call it -- the __forceinline__ functions of field.hpp,
// fieldu.hpp and curveu.hpp, no copy of a body -- on operands loaded from global memory (nothing to fold), and the result leaves by plain
// vector stores.
//
// This header is included by TWO translation units, because fieldu.hpp is shipped in two forms:
//   selftest_dev.hip        as msm_g2.hip, scalar_mul.hip and the point FFTs include it (no ZK_CHAIN_MAD): every op
//   selftest_dev_chain.hip  with ZK_CHAIN_MAD 1 as msm_g1.hip and ntt.hip define it: the U-form ops over Fq and Fr and the G1 group law
//                           (op | MI355ZK_DEVOP_CHAIN); the Fq2 / G2 code is never built with it
// The including unit defines ZK_ST_NS (the namespace that keeps the two sets of kernels apart) and ZK_ST_CHAIN (0 / 1).
//
// Layout: case i = in[i * in_words .. ], result i = out[i * out_words .. ]; lane i works on case i.  The launcher pads the case count to
// whole 256-lane workgroups by repeating the last case, so every quad and pair is fully active (the DPP forms require it).  For the
// lane-group ops the caller lays the SAME case in the 4 (2) lanes of a group and reads every lane's result.
#pragma once

#include "api_internal.hpp"
#include "mi355zk.h"

namespace zk {
namespace ZK_ST_NS {

struct DevOpShape {
  int in_words, out_words;   // per case; 0 / 0: no such op
  int group;                 // lanes that cooperate on one case (1, 2 or 4): n_cases must be a multiple
  bool fr;                   // the op exists over Fr as well (which == 1)
  bool chain;                // the op is built in the ZK_CHAIN_MAD unit as well
};

constexpr DevOpShape devop_shape(int op) {
  switch (op) {
    case MI355ZK_DEVOP_FP_MUL: case MI355ZK_DEVOP_FP_ADD: case MI355ZK_DEVOP_FP_SUB: return {16, 8, 1, true, false};
    case MI355ZK_DEVOP_FP_SQR: case MI355ZK_DEVOP_FP_DBL: case MI355ZK_DEVOP_FP_NEG: case MI355ZK_DEVOP_FP_REDUCE_ONCE:
    case MI355ZK_DEVOP_FP_INV: return {8, 8, 1, true, false};
    case MI355ZK_DEVOP_FQ2_MUL: case MI355ZK_DEVOP_FQ2_ADD: case MI355ZK_DEVOP_FQ2_SUB: return {32, 16, 1, false, false};
    case MI355ZK_DEVOP_FQ2_SQR: case MI355ZK_DEVOP_FQ2_INV: case MI355ZK_DEVOP_FQ2_NEG: return {16, 16, 1, false, false};
    case MI355ZK_DEVOP_U_FROM_STD: return {8, 9, 1, true, true};
    case MI355ZK_DEVOP_U_CARRY: case MI355ZK_DEVOP_U_DBL: case MI355ZK_DEVOP_U_SQR: return {9, 9, 1, true, true};
    case MI355ZK_DEVOP_U_TO_STD_LT2P: case MI355ZK_DEVOP_U_TO_STD_LT32P: return {9, 8, 1, true, true};
    case MI355ZK_DEVOP_U_ADD: case MI355ZK_DEVOP_U_MUL:
    case MI355ZK_DEVOP_U_SUB_1_1: case MI355ZK_DEVOP_U_SUB_2_1: case MI355ZK_DEVOP_U_SUB_3_1: case MI355ZK_DEVOP_U_SUB_4_1:
    case MI355ZK_DEVOP_U_SUB_4_2: case MI355ZK_DEVOP_U_SUB_4_3: case MI355ZK_DEVOP_U_SUB_8_1: case MI355ZK_DEVOP_U_SUB_16_1:
      return {18, 9, 1, true, true};
    case MI355ZK_DEVOP_U_MUL2: return {36, 9, 1, true, true};
    case MI355ZK_DEVOP_U_MUL3: return {54, 9, 1, true, true};
    case MI355ZK_DEVOP_U_MUL4: return {72, 9, 1, true, true};
    case MI355ZK_DEVOP_U_MUL_SHOUP: return {17, 18, 1, true, true};   // a (9), w_plain (8)  ->  a * w (9), wq (9)
    case MI355ZK_DEVOP_U_IS_ZERO_LT2P: case MI355ZK_DEVOP_U_IS_ZERO_LT8P: return {9, 1, 1, true, true};
    case MI355ZK_DEVOP_F2U_MUL_2: case MI355ZK_DEVOP_F2U_MUL_4: case MI355ZK_DEVOP_F2U_MUL_8:
    case MI355ZK_DEVOP_F2U_SUB_2: case MI355ZK_DEVOP_F2U_SUB_3: case MI355ZK_DEVOP_F2U_SUB_8: return {36, 18, 1, false, false};
    case MI355ZK_DEVOP_F2U_SQR_2: case MI355ZK_DEVOP_F2U_SQR_4: case MI355ZK_DEVOP_F2U_SQR_6: case MI355ZK_DEVOP_F2U_SQR_8:
      return {18, 18, 1, false, false};
    // G1: a register-form point is 36 words (X, Y, ZZ, ZZZ on nine limbs), a record 32, an affine coordinate 8
    case MI355ZK_DEVOP_G1_DOUBLE_AFFINE: return {16, 36, 1, false, true};
    case MI355ZK_DEVOP_G1_DOUBLE: return {36, 36, 1, false, true};
    case MI355ZK_DEVOP_G1_ADD_MIXED: return {53, 68, 1, false, true};        // acc, x, y, negate  ->  acc', xyzzu_to_r(acc')
    case MI355ZK_DEVOP_G1_RADD: return {72, 68, 1, false, true};             // acc, o  ->  acc', xyzzr_store(acc')
    case MI355ZK_DEVOP_G1_RECORD_TRIP: return {36, 100, 1, false, true};     // acc -> xyzzu_to_r, xyzzu_from_r of it, xyzzr_store(xyzzr_load) of it
    case MI355ZK_DEVOP_G1_RADD_QUAD: return {72, 68, 4, false, true};
    case MI355ZK_DEVOP_G1_PAIR_ADD_MIXED: return {53, 34, 2, false, true};   // -> this lane's (a, z) and its two record coordinates
    case MI355ZK_DEVOP_G1_ADD_AFFINE_PAIR: return {34, 68, 1, false, true};   // x1, y1, x2, y2, negate1, negate2  ->  acc, xyzzu_to_r(acc)
    case MI355ZK_DEVOP_G2_DOUBLE_AFFINE: return {32, 72, 1, false, false};
    case MI355ZK_DEVOP_G2_DOUBLE: return {72, 72, 1, false, false};
    case MI355ZK_DEVOP_G2_ADD_MIXED: return {105, 136, 1, false, false};
    case MI355ZK_DEVOP_G2_RADD: return {144, 136, 1, false, false};
    case MI355ZK_DEVOP_G2_RECORD_TRIP: return {72, 200, 1, false, false};
    case MI355ZK_DEVOP_G2_RADD_QUAD: return {144, 136, 4, false, false};
    case MI355ZK_DEVOP_G2_PAIR_ADD_MIXED: return {105, 68, 2, false, false};
    // Jacobian forms of the scalar multiplications (scalar_mul.hip, point_fft_g2.hip): a point is X, Y, Z in U-form (27 / 54 words)
    case MI355ZK_DEVOP_G1_JAC_DOUBLE: return {27, 27, 1, false, false};
    case MI355ZK_DEVOP_G1_JAC_ADD_MIXED: return {46, 27, 1, false, false};   // acc, x2, y2 (U-form, 2^261 domain), negate
    case MI355ZK_DEVOP_G1_JAC_ADD_TAB: return {55, 45, 1, false, false};     // acc, q, negate -> acc + jacu_tab_entry(q); the entry's zz, zzz
    case MI355ZK_DEVOP_G2_JAC_DOUBLE: return {54, 54, 1, false, false};
    case MI355ZK_DEVOP_G2_JAC_ADD_TAB: return {109, 90, 1, false, false};
    case MI355ZK_DEVOP_G2_JAC_TAB_PSI: return {90, 90, 1, false, false};     // q, cx, cy -> jacu2_tab_psi(jacu2_tab_entry(q), cx, cy): x, y, z, zz, zzz
    default: return {0, 0, 1, false, false};
  }
}

template <class T>
__device__ __forceinline__ T st_ld(const uint32_t* p) {
  static_assert(sizeof(T) % 4 == 0, "whole words");
  T t;
  __builtin_memcpy(&t, p, sizeof(T));
  return t;
}
template <class T>
__device__ __forceinline__ void st_st(uint32_t* p, const T& t) {
  __builtin_memcpy(p, &t, sizeof(T));
}

// the names that differ between the two groups; everything else is an overload
struct G1Ops {
  using F = Fq;
  using FU = FqU;
  using A = XYZZU<FqParams>;
  using R = XYZZ<Fq>;
  using Pair = PairAcc1;
  __device__ __forceinline__ static FU from_std(const F& a) { return u_from_std(a); }
  __device__ __forceinline__ static A double_affine(const FU& x, const FU& y) { return xyzzu_double_affine(x, y); }
  __device__ __forceinline__ static A dbl(const A& a) { return xyzzu_double(a); }
  __device__ __forceinline__ static void add_mixed(A& acc, const F& x, const F& y, bool neg) { xyzzu_add_mixed(acc, x, y, neg); }
  using J = JacU<FqParams>;
  using T = JacTabU<FqParams>;
  __device__ __forceinline__ static J jdbl(const J& a) { return jacu_double(a); }
  __device__ __forceinline__ static T tab_entry(const J& q) { return jacu_tab_entry(q); }
  __device__ __forceinline__ static void add_tab(J& acc, const T& t, bool neg) { jacu_add_tab(acc, t, neg); }
};
struct G2Ops {
  using F = Fq2;
  using FU = Fq2U;
  using A = XYZZU2;
  using R = XYZZ<Fq2>;
  using Pair = PairAcc2;
  __device__ __forceinline__ static FU from_std(const F& a) { return f2u_from_std(a); }
  __device__ __forceinline__ static A double_affine(const FU& x, const FU& y) { return xyzzu2_double_affine(x, y); }
  __device__ __forceinline__ static A dbl(const A& a) { return xyzzu2_double(a); }
  __device__ __forceinline__ static void add_mixed(A& acc, const F& x, const F& y, bool neg) { xyzzu2_add_mixed(acc, x, y, neg); }
  using J = JacU2;
  using T = JacTabU2;
  __device__ __forceinline__ static J jdbl(const J& a) { return jacu2_double(a); }
  __device__ __forceinline__ static T tab_entry(const J& q) { return jacu2_tab_entry(q); }
  __device__ __forceinline__ static void add_tab(J& acc, const T& t, bool neg) { jacu2_add_tab(acc, t, neg); }
};

// WHAT: 0 double, 1 add_mixed (G1), 2 tab_entry + add_tab, 3 tab_entry + tab_psi (G2)
template <class G, int WHAT>
__device__ __forceinline__ void jac_op(const uint32_t* in, uint32_t* out) {
  using J = typename G::J;
  using FU = typename G::FU;
  constexpr int UW = sizeof(FU) / 4, JW = 3 * UW;
  static_assert(sizeof(J) == 4 * JW, "X, Y, Z");
  if constexpr (WHAT == 0) {
    st_st(out, G::jdbl(st_ld<J>(in)));
  } else if constexpr (WHAT == 1) {
    J acc = st_ld<J>(in);
    jacu_add_mixed(acc, st_ld<FU>(in + JW), st_ld<FU>(in + JW + UW), in[JW + 2 * UW] != 0);
    st_st(out, acc);
  } else if constexpr (WHAT == 2) {
    J acc = st_ld<J>(in);
    const typename G::T t = G::tab_entry(st_ld<J>(in + JW));
    G::add_tab(acc, t, in[2 * JW] != 0);
    st_st(out, acc);
    st_st(out + JW, t.zz);
    st_st(out + JW + UW, t.zzz);
  } else {
    const JacTabU2 t = jacu2_tab_psi(jacu2_tab_entry(st_ld<J>(in)), st_ld<Fq2U>(in + JW), st_ld<Fq2U>(in + JW + UW));
    st_st(out, t.x);
    st_st(out + UW, t.y);
    st_st(out + 2 * UW, t.z);
    st_st(out + 3 * UW, t.zz);
    st_st(out + 4 * UW, t.zzz);
  }
}

// WHAT: 0 double_affine, 1 double, 2 add_mixed, 3 xyzzr_add, 4 record trip, 5 xyzzr_add_quad, 6 pair_add_mixed
template <class G, int WHAT>
__device__ __forceinline__ void group_op(const uint32_t* in, uint32_t* out, uint32_t lane) {
  using F = typename G::F;
  using A = typename G::A;
  using R = typename G::R;
  constexpr int FW = sizeof(F) / 4, AW = sizeof(A) / 4, RW = sizeof(R) / 4;
  if constexpr (WHAT == 0) {
    st_st(out, G::double_affine(G::from_std(st_ld<F>(in)), G::from_std(st_ld<F>(in + FW))));
  } else if constexpr (WHAT == 1) {
    st_st(out, G::dbl(st_ld<A>(in)));
  } else if constexpr (WHAT == 2) {
    A acc = st_ld<A>(in);
    G::add_mixed(acc, st_ld<F>(in + AW), st_ld<F>(in + AW + FW), in[AW + 2 * FW] != 0);
    st_st(out, acc);
    st_st(out + AW, xyzzu_to_r(acc));
  } else if constexpr (WHAT == 3) {
    A acc = st_ld<A>(in);
    xyzzr_add(acc, st_ld<A>(in + AW));
    st_st(out, acc);
    st_st(out + AW, xyzzr_store(acc));
  } else if constexpr (WHAT == 4) {
    const R rec = xyzzu_to_r(st_ld<A>(in));
    st_st(out, rec);
    st_st(out + RW, xyzzu_from_r(rec));
    st_st(out + RW + AW, xyzzr_store(xyzzr_load(rec)));
  } else if constexpr (WHAT == 5) {
    const A res = xyzzr_add_quad(st_ld<A>(in), st_ld<A>(in + AW), lane & 3u);   // the role as msm_impl.hpp takes it: lane & 3
    st_st(out, res);
    st_st(out + AW, xyzzr_store(res));
  } else {
    // the pair kernels' split (msm_impl.hpp: msm_accumulate_pair_kernel): the even lane holds (X, ZZ) and gathers x, the odd lane (Y, ZZZ) and y
    using P = typename G::Pair;
    using FU = typename G::FU;
    constexpr int UW = sizeof(FU) / 4;
    const bool odd = (lane & 1u) != 0;
    const P acc{st_ld<FU>(in + (odd ? UW : 0)), st_ld<FU>(in + (odd ? 3 * UW : 2 * UW))};
    const P res = pair_add_mixed(acc, st_ld<F>(in + AW + (odd ? FW : 0)), in[AW + 2 * FW] != 0, odd);
    F oa, oz;
    pair_to_r(res, oa, oz);
    st_st(out, res.a);
    st_st(out + UW, res.z);
    st_st(out + 2 * UW, oa);
    st_st(out + 2 * UW + FW, oz);
  }
}

template <int OP, class PR>
__device__ __forceinline__ void devop_run(const uint32_t* in, uint32_t* out, uint32_t lane) {
  using F = Fp<PR>;
  using U = FpU<PR>;
  [[maybe_unused]] auto u = [&](int i) { return st_ld<U>(in + 9 * i); };
  [[maybe_unused]] auto f2u = [&](int i) { return st_ld<Fq2U>(in + 18 * i); };
  if constexpr (OP == MI355ZK_DEVOP_FP_MUL) st_st(out, mul(st_ld<F>(in), st_ld<F>(in + 8)));
  else if constexpr (OP == MI355ZK_DEVOP_FP_SQR) st_st(out, sqr(st_ld<F>(in)));
  else if constexpr (OP == MI355ZK_DEVOP_FP_ADD) st_st(out, add(st_ld<F>(in), st_ld<F>(in + 8)));
  else if constexpr (OP == MI355ZK_DEVOP_FP_SUB) st_st(out, sub(st_ld<F>(in), st_ld<F>(in + 8)));
  else if constexpr (OP == MI355ZK_DEVOP_FP_DBL) st_st(out, dbl(st_ld<F>(in)));
  else if constexpr (OP == MI355ZK_DEVOP_FP_NEG) st_st(out, neg(st_ld<F>(in)));
  else if constexpr (OP == MI355ZK_DEVOP_FP_REDUCE_ONCE) st_st(out, reduce_once(st_ld<F>(in)));
  else if constexpr (OP == MI355ZK_DEVOP_FP_INV) st_st(out, inv(st_ld<F>(in)));
  else if constexpr (OP == MI355ZK_DEVOP_FQ2_MUL) st_st(out, mul(st_ld<Fq2>(in), st_ld<Fq2>(in + 16)));
  else if constexpr (OP == MI355ZK_DEVOP_FQ2_SQR) st_st(out, sqr(st_ld<Fq2>(in)));
  else if constexpr (OP == MI355ZK_DEVOP_FQ2_INV) st_st(out, inv(st_ld<Fq2>(in)));
  else if constexpr (OP == MI355ZK_DEVOP_FQ2_ADD) st_st(out, add(st_ld<Fq2>(in), st_ld<Fq2>(in + 16)));
  else if constexpr (OP == MI355ZK_DEVOP_FQ2_SUB) st_st(out, sub(st_ld<Fq2>(in), st_ld<Fq2>(in + 16)));
  else if constexpr (OP == MI355ZK_DEVOP_FQ2_NEG) st_st(out, neg(st_ld<Fq2>(in)));
  else if constexpr (OP == MI355ZK_DEVOP_U_FROM_STD) st_st(out, u_from_std(st_ld<F>(in)));
  else if constexpr (OP == MI355ZK_DEVOP_U_CARRY) st_st(out, u_carry(u(0)));
  else if constexpr (OP == MI355ZK_DEVOP_U_TO_STD_LT2P) st_st(out, u_to_std_lt2p(u(0)));
  else if constexpr (OP == MI355ZK_DEVOP_U_TO_STD_LT32P) st_st(out, u_to_std_lt32p(u(0)));
  else if constexpr (OP == MI355ZK_DEVOP_U_ADD) st_st(out, u_add(u(0), u(1)));
  else if constexpr (OP == MI355ZK_DEVOP_U_DBL) st_st(out, u_dbl(u(0)));
  else if constexpr (OP == MI355ZK_DEVOP_U_SUB_1_1) st_st(out, u_sub<1, 1>(u(0), u(1)));
  else if constexpr (OP == MI355ZK_DEVOP_U_SUB_2_1) st_st(out, u_sub<2, 1>(u(0), u(1)));
  else if constexpr (OP == MI355ZK_DEVOP_U_SUB_3_1) st_st(out, u_sub<3, 1>(u(0), u(1)));
  else if constexpr (OP == MI355ZK_DEVOP_U_SUB_4_1) st_st(out, u_sub<4, 1>(u(0), u(1)));
  else if constexpr (OP == MI355ZK_DEVOP_U_SUB_4_2) st_st(out, u_sub<4, 2>(u(0), u(1)));
  else if constexpr (OP == MI355ZK_DEVOP_U_SUB_4_3) st_st(out, u_sub<4, 3>(u(0), u(1)));
  else if constexpr (OP == MI355ZK_DEVOP_U_SUB_8_1) st_st(out, u_sub<8, 1>(u(0), u(1)));
  else if constexpr (OP == MI355ZK_DEVOP_U_SUB_16_1) st_st(out, u_sub<16, 1>(u(0), u(1)));
  else if constexpr (OP == MI355ZK_DEVOP_U_MUL) st_st(out, u_mul(u(0), u(1)));
  else if constexpr (OP == MI355ZK_DEVOP_U_SQR) st_st(out, u_sqr(u(0)));
  else if constexpr (OP == MI355ZK_DEVOP_U_MUL2) st_st(out, u_mul2(u(0), u(1), u(2), u(3)));
  else if constexpr (OP == MI355ZK_DEVOP_U_MUL3) st_st(out, u_mul3(u(0), u(1), u(2), u(3), u(4), u(5)));
  else if constexpr (OP == MI355ZK_DEVOP_U_MUL4) st_st(out, u_mul4(u(0), u(1), u(2), u(3), u(4), u(5), u(6), u(7)));
  else if constexpr (OP == MI355ZK_DEVOP_U_MUL_SHOUP) {
    const F c = st_ld<F>(in + 9);                                   // the plain integer w < p, as ntt.hip's table builder holds it
    const U wq = u_shoup_quotient<PR>(c.l);
    st_st(out, u_mul_shoup(u(0), u_from_std(c), wq));
    st_st(out + 9, wq);
  } else if constexpr (OP == MI355ZK_DEVOP_U_IS_ZERO_LT2P) out[0] = u_is_zero_lt2p(u(0)) ? 1u : 0u;
  else if constexpr (OP == MI355ZK_DEVOP_U_IS_ZERO_LT8P) out[0] = u_is_zero_lt8p(u(0)) ? 1u : 0u;
  else if constexpr (OP == MI355ZK_DEVOP_F2U_MUL_2) st_st(out, f2u_mul<2>(f2u(0), f2u(1)));
  else if constexpr (OP == MI355ZK_DEVOP_F2U_MUL_4) st_st(out, f2u_mul<4>(f2u(0), f2u(1)));
  else if constexpr (OP == MI355ZK_DEVOP_F2U_MUL_8) st_st(out, f2u_mul<8>(f2u(0), f2u(1)));
  else if constexpr (OP == MI355ZK_DEVOP_F2U_SQR_2) st_st(out, f2u_sqr<2>(f2u(0)));
  else if constexpr (OP == MI355ZK_DEVOP_F2U_SQR_4) st_st(out, f2u_sqr<4>(f2u(0)));
  else if constexpr (OP == MI355ZK_DEVOP_F2U_SQR_6) st_st(out, f2u_sqr<6>(f2u(0)));
  else if constexpr (OP == MI355ZK_DEVOP_F2U_SQR_8) st_st(out, f2u_sqr<8>(f2u(0)));
  else if constexpr (OP == MI355ZK_DEVOP_F2U_SUB_2) st_st(out, f2u_sub<2>(f2u(0), f2u(1)));
  else if constexpr (OP == MI355ZK_DEVOP_F2U_SUB_3) st_st(out, f2u_sub<3>(f2u(0), f2u(1)));
  else if constexpr (OP == MI355ZK_DEVOP_F2U_SUB_8) st_st(out, f2u_sub<8>(f2u(0), f2u(1)));
  else if constexpr (OP >= MI355ZK_DEVOP_G1_DOUBLE_AFFINE && OP <= MI355ZK_DEVOP_G1_PAIR_ADD_MIXED)
    group_op<G1Ops, OP - MI355ZK_DEVOP_G1_DOUBLE_AFFINE>(in, out, lane);
  else if constexpr (OP >= MI355ZK_DEVOP_G2_DOUBLE_AFFINE && OP <= MI355ZK_DEVOP_G2_PAIR_ADD_MIXED)
    group_op<G2Ops, OP - MI355ZK_DEVOP_G2_DOUBLE_AFFINE>(in, out, lane);
  else if constexpr (OP == MI355ZK_DEVOP_G1_ADD_AFFINE_PAIR) {
    const XYZZU<FqParams> acc = xyzzu_from_affine_pair(st_ld<Fq>(in), st_ld<Fq>(in + 8), in[32] != 0, st_ld<Fq>(in + 16), st_ld<Fq>(in + 24), in[33] != 0);
    st_st(out, acc);
    st_st(out + 36, xyzzu_to_r(acc));
  } else if constexpr (OP == MI355ZK_DEVOP_G1_JAC_DOUBLE) jac_op<G1Ops, 0>(in, out);
  else if constexpr (OP == MI355ZK_DEVOP_G1_JAC_ADD_MIXED) jac_op<G1Ops, 1>(in, out);
  else if constexpr (OP == MI355ZK_DEVOP_G1_JAC_ADD_TAB) jac_op<G1Ops, 2>(in, out);
  else if constexpr (OP == MI355ZK_DEVOP_G2_JAC_DOUBLE) jac_op<G2Ops, 0>(in, out);
  else if constexpr (OP == MI355ZK_DEVOP_G2_JAC_ADD_TAB) jac_op<G2Ops, 2>(in, out);
  else if constexpr (OP == MI355ZK_DEVOP_G2_JAC_TAB_PSI) jac_op<G2Ops, 3>(in, out);
  else static_assert(OP < 0, "op without a body");
}

// n_lanes is a multiple of 256 (the launcher pads): every lane of every wave is active and in bounds
template <int OP, class PR>
__global__ __launch_bounds__(256) void selftest_dev_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  constexpr DevOpShape S = devop_shape(OP);
  const uint32_t lane = blockIdx.x * 256u + threadIdx.x;
  devop_run<OP, PR>(in + (size_t)lane * S.in_words, out + (size_t)lane * S.out_words, lane);
}

template <int OP>
int devop_launch_one(int which, const uint32_t* d_in, uint32_t* d_out, uint32_t blocks) {
  constexpr DevOpShape S = devop_shape(OP);
  if constexpr (ZK_ST_CHAIN && !S.chain) {
    return ZK_ERR_BAD_ARGS;
  } else {
    if (which == 0) hipLaunchKernelGGL((selftest_dev_kernel<OP, FqParams>), dim3(blocks), dim3(256), 0, 0, d_in, d_out);
    else if constexpr (S.fr) hipLaunchKernelGGL((selftest_dev_kernel<OP, FrParams>), dim3(blocks), dim3(256), 0, 0, d_in, d_out);
    else return ZK_ERR_BAD_ARGS;
    ZK_HIP(hipGetLastError());
    return ZK_OK;
  }
}

template <int... OPS>
int devop_dispatch(int op, int which, const uint32_t* d_in, uint32_t* d_out, uint32_t blocks, std::integer_sequence<int, OPS...>) {
  int rc = ZK_ERR_BAD_ARGS;
  (void)((op == OPS ? (rc = devop_launch_one<OPS>(which, d_in, d_out, blocks), true) : false) || ...);
  return rc;
}

// d_in: blocks * 256 cases, d_out: room for as many results
inline int devop_launch(int op, int which, const uint32_t* d_in, uint32_t* d_out, uint32_t blocks) {
  return devop_dispatch(op, which, d_in, d_out, blocks, std::make_integer_sequence<int, MI355ZK_DEVOP_END>{});
}

}  // namespace ZK_ST_NS
}  // namespace zk
