// ark355_diag_field_ops: every field primitive of field.cuh / field28.cuh on its own, one lane per element.
//
// A TEST entry (include/ark355.h): the suite drives the production arithmetic through whole operations -- MSMs, transforms,
// proofs -- whose multiplications see pseudo-random intermediates only.  The kernels here load operands the caller designed
// (raw limb words, non-canonical forms included), call the VERY functions the production kernels call -- Fp<P> / Fp2<P> / Fp28<P>
// on the production parameter classes, nothing copied -- and store what comes back.  One kernel per field TYPE with the operation
// as a run-time switch keeps the build short; the out-of-line (`_ni`) bodies are used where the production code has them.
// Included by capi.hip only: the kernels are compiled once.
#pragma once
#include "common.h"
#include "field28.cuh"

namespace ark355 {

// ---- operation codes (include/ark355.h: ARK355_FOP_*) -------------------------------------------------------------------------
enum : int32_t {
  FOP_ADD = 0, FOP_SUB = 1, FOP_NEG = 2, FOP_DBL = 3, FOP_MUL = 4, FOP_MUL_NI = 5, FOP_SQR = 6, FOP_MUL2SUM = 7, FOP_MUL_SUB = 8,
  FOP_INV = 9, FOP_TO_MONT = 10, FOP_FROM_MONT = 11, FOP_SQR_NI = 12,
  FOP28_FROM_FP = 32, FOP28_TO_FP = 33, FOP28_TO_FP_LT8 = 34, FOP28_NORM = 35, FOP28_CANON = 36, FOP28_IS_ZERO = 37,
  FOP28_IS_ZERO_INL = 38, FOP28_HINT = 39, FOP28_ADD = 40, FOP28_MUL = 41, FOP28_SQR = 42, FOP28_MUL2SUM = 43, FOP28_MUL4SUM = 44,
  FOP28_COND_SUB = 48,        // + log2 K, K = 1, 2, 4, 8, 16
  FOP28_SUB = 0x100,          // + 16 K + BETA
  FOP28_NEG = 0x200,          // + 16 K + BETA
};
enum : int32_t { FLD_BLS_FQ = 0, FLD_BLS_FR = 1, FLD_BN_FQ = 2, FLD_BN_FR = 3, FLD_BLS_FQ2 = 4, FLD_BN_FQ2 = 5, FLD_BLS_FQ28 = 6, FLD_BN_FQ28 = 7 };

// every (K, BETA) with which msm28_impl.cuh / tails28_impl.cuh instantiate Fp28::sub / Fp28::neg, directly or through Pair28
// (sqr / sqr_x<KA>: sub<KA, 1>;  mul<KA, B> / mul2<KA, BA, KC, BC> / both_of / both_with: neg<K, B>)
#define ARK_DIAG_SUB_CLASSES(X) X(3, 1) X(5, 1) X(6, 1) X(8, 1) X(11, 1)
#define ARK_DIAG_NEG_CLASSES(X) X(2, 1) X(3, 1) X(3, 3) X(4, 2) X(4, 3) X(5, 1) X(5, 4) X(6, 1) X(8, 1)

struct FieldOpShape {
  int arity;          // operand arrays
  int in_words;       // 32-bit words per operand element
  int out_words;      // 32-bit words per result element
};

// The shape of (field, op), or false for a combination the library cannot instantiate (host code: no HIP call)
static inline bool diag_field_op_shape(int32_t field, int32_t op, FieldOpShape& s) {
  if (field >= FLD_BLS_FQ && field <= FLD_BN_FR) {
    const int nb = field == FLD_BLS_FQ ? BlsFq::N : field == FLD_BLS_FR ? BlsFr::N : field == FLD_BN_FQ ? BnFq::N : BnFr::N;
    const int bits = field == FLD_BLS_FQ ? BlsFqParams::BITS : field == FLD_BLS_FR ? BlsFrParams::BITS
                     : field == FLD_BN_FQ ? BnFqParams::BITS : BnFrParams::BITS;
    int arity;
    switch (op) {
      case FOP_ADD: case FOP_SUB: case FOP_MUL: case FOP_MUL_NI: arity = 2; break;
      case FOP_NEG: case FOP_DBL: case FOP_SQR: case FOP_INV: case FOP_TO_MONT: case FOP_FROM_MONT: arity = 1; break;
      case FOP_MUL2SUM: case FOP_MUL_SUB:
        if (bits > 32 * nb - 2) return false;        // Fp::mul2sum: "needs two spare top bits"
        arity = 4;
        break;
      default: return false;
    }
    s = FieldOpShape{arity, nb, nb};
    return true;
  }
  if (field == FLD_BLS_FQ2 || field == FLD_BN_FQ2) {
    const int nw = 2 * (field == FLD_BLS_FQ2 ? BlsFq::N : BnFq::N);
    int arity;
    switch (op) {
      case FOP_ADD: case FOP_SUB: case FOP_MUL: case FOP_MUL_NI: arity = 2; break;
      case FOP_NEG: case FOP_SQR: case FOP_SQR_NI: case FOP_INV: arity = 1; break;
      case FOP_MUL_SUB: arity = 4; break;
      default: return false;         // Fp2 has no dbl entry here, no mul2sum, no Montgomery conversions
    }
    s = FieldOpShape{arity, nw, nw};
    return true;
  }
  if (field == FLD_BLS_FQ28 || field == FLD_BN_FQ28) {
    const int nb = field == FLD_BLS_FQ28 ? BlsFq::N : BnFq::N;
    const int n = field == FLD_BLS_FQ28 ? BlsFq28::N : BnFq28::N;
    switch (op) {
      case FOP28_FROM_FP: s = FieldOpShape{1, nb, n}; return true;
      case FOP28_TO_FP: case FOP28_TO_FP_LT8: s = FieldOpShape{1, n, nb}; return true;
      case FOP28_NORM: case FOP28_CANON: case FOP28_SQR: s = FieldOpShape{1, n, n}; return true;
      case FOP28_IS_ZERO: case FOP28_IS_ZERO_INL: case FOP28_HINT: s = FieldOpShape{1, n, 1}; return true;
      case FOP28_ADD: case FOP28_MUL: s = FieldOpShape{2, n, n}; return true;
      case FOP28_MUL2SUM: s = FieldOpShape{4, n, n}; return true;
      case FOP28_MUL4SUM: s = FieldOpShape{8, n, n}; return true;
      default: break;
    }
    if (op >= FOP28_COND_SUB && op <= FOP28_COND_SUB + 4) {
      s = FieldOpShape{1, n, n};
      return true;
    }
#define ARK_X(K, B) if (op == FOP28_SUB + 16 * K + B) { s = FieldOpShape{2, n, n}; return true; }
    ARK_DIAG_SUB_CLASSES(ARK_X)
#undef ARK_X
#define ARK_X(K, B) if (op == FOP28_NEG + 16 * K + B) { s = FieldOpShape{1, n, n}; return true; }
    ARK_DIAG_NEG_CLASSES(ARK_X)
#undef ARK_X
    return false;
  }
  return false;
}

struct FieldOpArgs {
  const uint32_t* in[8];
  uint32_t* out;
  uint32_t* flavour;
  uint64_t n;
  int32_t op;
  int32_t arity;
};

// which multiplier this very kernel was compiled with: 1 = the inline-assembly column chain of field.cuh
#if defined(__HIP_DEVICE_COMPILE__) && !defined(ARK_NO_ASM_MUL)
#define ARK_DIAG_FLAVOUR 1u
#else
#define ARK_DIAG_FLAVOUR 0u
#endif

template <class T, int W>
ARK_D T diag_load_words(const uint32_t* p, uint64_t i) {
  T r;
#pragma unroll
  for (int k = 0; k < W; k++) r.l[k] = p[i * W + k];
  return r;
}

template <class F>
static __global__ void __launch_bounds__(256) diag_fp_kernel(FieldOpArgs a) {
  constexpr int N = F::N;
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i == 0) *a.flavour = ARK_DIAG_FLAVOUR;
  if (i >= a.n) return;
  F x[4];
#pragma unroll
  for (int j = 0; j < 4; j++) x[j] = j < a.arity ? diag_load_words<F, N>(a.in[j], i) : F::zero();
  F r = F::zero();
  switch (a.op) {
    case FOP_ADD: r = F::add(x[0], x[1]); break;
    case FOP_SUB: r = F::sub(x[0], x[1]); break;
    case FOP_NEG: r = F::neg(x[0]); break;
    case FOP_DBL: r = F::dbl(x[0]); break;
    case FOP_MUL: r = F::mul(x[0], x[1]); break;
    case FOP_MUL_NI: r = F::mul_ni(x[0], x[1]); break;
    case FOP_SQR: r = F::sqr(x[0]); break;
    case FOP_INV: r = F::inv(x[0]); break;
    case FOP_TO_MONT: r = F::to_mont(x[0]); break;
    case FOP_FROM_MONT: r = F::from_mont(x[0]); break;
    default:
      if constexpr (F::Params::BITS <= 32 * N - 2) {
        if (a.op == FOP_MUL2SUM) r = F::mul2sum(x[0], x[1], x[2], x[3]);
        else if (a.op == FOP_MUL_SUB) r = F::mul_sub(x[0], x[1], x[2], x[3]);
      }
      break;
  }
#pragma unroll
  for (int k = 0; k < N; k++) a.out[i * N + k] = r.l[k];
}

template <class F2>
static __global__ void __launch_bounds__(256) diag_fp2_kernel(FieldOpArgs a) {
  using B = typename F2::Base;
  constexpr int N = B::N;
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i == 0) *a.flavour = ARK_DIAG_FLAVOUR;
  if (i >= a.n) return;
  F2 x[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    if (j < a.arity) {
      x[j].c0 = diag_load_words<B, N>(a.in[j], 2 * i);
      x[j].c1 = diag_load_words<B, N>(a.in[j], 2 * i + 1);
    } else {
      x[j] = F2::zero();
    }
  }
  F2 r = F2::zero();
  switch (a.op) {
    case FOP_ADD: r = F2::add(x[0], x[1]); break;
    case FOP_SUB: r = F2::sub(x[0], x[1]); break;
    case FOP_NEG: r = F2::neg(x[0]); break;
    case FOP_MUL: r = F2::mul(x[0], x[1]); break;
    case FOP_MUL_NI: r = F2::mul_ni(x[0], x[1]); break;
    case FOP_SQR: r = F2::sqr(x[0]); break;
    case FOP_SQR_NI: r = F2::sqr_ni(x[0]); break;
    case FOP_INV: r = F2::inv(x[0]); break;
    case FOP_MUL_SUB: r = F2::mul_sub(x[0], x[1], x[2], x[3]); break;
    default: break;
  }
#pragma unroll
  for (int k = 0; k < N; k++) {
    a.out[(2 * i) * N + k] = r.c0.l[k];
    a.out[(2 * i + 1) * N + k] = r.c1.l[k];
  }
}

template <class F>
static __global__ void __launch_bounds__(256) diag_fp28_kernel(FieldOpArgs a) {
  using B = typename F::Base;
  constexpr int N = F::N, NB = F::NB;
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i == 0) *a.flavour = ARK_DIAG_FLAVOUR;
  if (i >= a.n) return;
  const int32_t op = a.op;
  if (op == FOP28_FROM_FP) {
    const F r = F::from_fp(diag_load_words<B, NB>(a.in[0], i));
#pragma unroll
    for (int k = 0; k < N; k++) a.out[i * N + k] = r.l[k];
    return;
  }
  const F x0 = diag_load_words<F, N>(a.in[0], i);
  if (op == FOP28_TO_FP || op == FOP28_TO_FP_LT8) {
    const B r = op == FOP28_TO_FP ? F::to_fp(x0) : F::to_fp_lt8(x0);
#pragma unroll
    for (int k = 0; k < NB; k++) a.out[i * NB + k] = r.l[k];
    return;
  }
  if (op == FOP28_IS_ZERO || op == FOP28_IS_ZERO_INL || op == FOP28_HINT) {
    a.out[i] = op == FOP28_IS_ZERO ? (F::is_zero_mod_p(x0) ? 1u : 0u)
               : op == FOP28_IS_ZERO_INL ? (F::is_zero_mod_p_inl(x0) ? 1u : 0u) : x0.multiple_hint();
    return;
  }
  F r = F::zero();
  if (a.arity == 1) {
    switch (op) {
      case FOP28_NORM: r = F::norm(x0); break;
      case FOP28_CANON: r = F::canon(x0); break;
      case FOP28_SQR: r = F::sqr(x0); break;
      case FOP28_COND_SUB + 0: r = F::template cond_sub<1>(x0); break;
      case FOP28_COND_SUB + 1: r = F::template cond_sub<2>(x0); break;
      case FOP28_COND_SUB + 2: r = F::template cond_sub<4>(x0); break;
      case FOP28_COND_SUB + 3: r = F::template cond_sub<8>(x0); break;
      case FOP28_COND_SUB + 4: r = F::template cond_sub<16>(x0); break;
#define ARK_X(K, BETA) case FOP28_NEG + 16 * K + BETA: r = F::template neg<K, BETA>(x0); break;
      ARK_DIAG_NEG_CLASSES(ARK_X)
#undef ARK_X
      default: break;
    }
  } else {
    const F x1 = diag_load_words<F, N>(a.in[1], i);
    if (a.arity == 2) {
      switch (op) {
        case FOP28_ADD: r = F::add(x0, x1); break;
        case FOP28_MUL: r = F::mul(x0, x1); break;
#define ARK_X(K, BETA) case FOP28_SUB + 16 * K + BETA: r = F::template sub<K, BETA>(x0, x1); break;
        ARK_DIAG_SUB_CLASSES(ARK_X)
#undef ARK_X
        default: break;
      }
    } else {
      const F x2 = diag_load_words<F, N>(a.in[2], i), x3 = diag_load_words<F, N>(a.in[3], i);
      if (a.arity == 4) {
        if (op == FOP28_MUL2SUM) r = F::mul2sum(x0, x1, x2, x3);
      } else if (op == FOP28_MUL4SUM) {
        const F x4 = diag_load_words<F, N>(a.in[4], i), x5 = diag_load_words<F, N>(a.in[5], i);
        const F x6 = diag_load_words<F, N>(a.in[6], i), x7 = diag_load_words<F, N>(a.in[7], i);
        r = F::mul4sum(x0, x1, x2, x3, x4, x5, x6, x7);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < N; k++) a.out[i * N + k] = r.l[k];
}

// operands up, one launch on `st`, result and flavour word back.  The arguments were checked by the caller (capi.hip).
static inline void diag_field_ops_run(hipStream_t st, int32_t field, int32_t op, const FieldOpShape& s, const uint32_t* const* operands,
                                      uint64_t n, uint32_t* result, uint32_t* flavour) {
  const size_t in_bytes = (size_t)n * s.in_words * 4, out_bytes = (size_t)n * s.out_words * 4;
  DevBuf buf((size_t)s.arity * in_bytes + out_bytes + 16);
  FieldOpArgs a{};
  char* base = buf.as<char>();
  for (int j = 0; j < s.arity; j++) {
    a.in[j] = reinterpret_cast<const uint32_t*>(base + (size_t)j * in_bytes);
    if (n) ARK_CHECK_HIP(hipMemcpyAsync(base + (size_t)j * in_bytes, operands[j], in_bytes, hipMemcpyHostToDevice, st));
  }
  a.out = reinterpret_cast<uint32_t*>(base + (size_t)s.arity * in_bytes);
  a.flavour = reinterpret_cast<uint32_t*>(base + (size_t)s.arity * in_bytes + out_bytes);
  a.n = n;
  a.op = op;
  a.arity = s.arity;
  const dim3 grid((uint32_t)(n ? (n + 255) / 256 : 1)), block(256);
  switch (field) {
    case FLD_BLS_FQ: ARK_LAUNCH((diag_fp_kernel<BlsFq>), grid, block, 0, st, a); break;
    case FLD_BLS_FR: ARK_LAUNCH((diag_fp_kernel<BlsFr>), grid, block, 0, st, a); break;
    case FLD_BN_FQ: ARK_LAUNCH((diag_fp_kernel<BnFq>), grid, block, 0, st, a); break;
    case FLD_BN_FR: ARK_LAUNCH((diag_fp_kernel<BnFr>), grid, block, 0, st, a); break;
    case FLD_BLS_FQ2: ARK_LAUNCH((diag_fp2_kernel<BlsFq2>), grid, block, 0, st, a); break;
    case FLD_BN_FQ2: ARK_LAUNCH((diag_fp2_kernel<BnFq2>), grid, block, 0, st, a); break;
    case FLD_BLS_FQ28: ARK_LAUNCH((diag_fp28_kernel<BlsFq28>), grid, block, 0, st, a); break;
    default: ARK_LAUNCH((diag_fp28_kernel<BnFq28>), grid, block, 0, st, a); break;
  }
  ARK_CHECK_LAUNCH();
  if (n) ARK_CHECK_HIP(hipMemcpyAsync(result, a.out, out_bytes, hipMemcpyDeviceToHost, st));
  ARK_CHECK_HIP(hipMemcpyAsync(flavour, a.flavour, 4, hipMemcpyDeviceToHost, st));
  ARK_CHECK_HIP(hipStreamSynchronize(st));
}

}  // namespace ark355
