// Column polynomials of any GR1CS predicate at a point, on the device: the generator's half of a resident system.  For the t
// matrices M_0 .. M_{t-1} (n rows, m = num_instance + num_witness columns) of one predicate and a vector y of n Fr
//     out[k][j] = sum over the STORED entries (i, j, c) of M_k of c * y[i]          (= (M_k^T y)_j, mat_vec_mul transposed)
// and, with y = (L_i(tau))_i over H_N, out[k][j] = sum_i M_k[i][j] L_i(tau): the column polynomials of the predicate at tau,
// R1CSToQAP::instance_map_with_evaluation's a, b, c for any arity (rows n .. N-1 are zero rows and contribute nothing).
// setup_impl.cuh computes the same sums for Groth16 only (R1csDev, three matrices, the instance rows u_j += L_{n+j}, canonical
// output and the alpha/beta/gamma/delta combination behind them), and with the same kernels: the column gather of
// colgather_impl.cuh (C1 column-major order, C2 gather with a heavy list; the one host wait reads the heavy counter) over
// FrTerms.  Here the resident Gr1csPred arrays are read where they lie (the Gr1csMat table, the shared pool), the output is
// Montgomery, y is any vector, the longest column one lane sums is a policy (COLS_LANE_MAX), and the scratch is the context's
// and grows only -- no allocation, no free and no wait for one inside a call.
//
//   C3  Lagrange vector for columns_at / lagrange_fr: lagrange_run of setup_impl.cuh; it stays in the scratch and never visits
//       the host.
//
// Scratch of one call (ColumnsScratch, bytes): the gather's (colgather_impl.cuh), and
//     32 N         Lagrange vector (columns_at)
//     32 (y_len + t m)  staging of y and of the output (host variants only)
#pragma once
#include <string>
#include "common.h"
#include "msm_impl.cuh"
#include "gr1cs_impl.cuh"
#include "colgather_impl.cuh"
#include "setup_impl.cuh"

namespace ark355 {

constexpr uint32_t COLS_LANE_MAX_DEFAULT = COLGATHER_LANE_MAX;  // 64: the generator's measured choice
constexpr uint32_t COLS_LANE_MAX_LIMIT = 1u << 20;

// policy COLS_LANE_MAX -> the longest column one lane sums: <= 0 selects the default, anything else is clamped to the limit
static inline uint32_t cols_lane_max(int32_t policy) {
  if (policy <= 0) return COLS_LANE_MAX_DEFAULT;
  return (uint32_t)policy > COLS_LANE_MAX_LIMIT ? COLS_LANE_MAX_LIMIT : (uint32_t)policy;
}

// grow-only scratch of a context
struct ColumnsScratch {
  ColGatherScratch gather;
  DevBuf lag;            // the Lagrange vector of columns_at / the host variant of lagrange_fr
  DevBuf y, out;         // staging of the host variants
};

struct ColumnsDims {
  uint64_t n = 0, cols = 0, nnz = 0, max_nnz = 0;
  uint32_t log_domain = 0;          // columns_at only
};

// What one call needs and what refuses it; no HIP call.  with_domain: the domain rule of ark355_gr1cs_quotient.
static inline int32_t columns_dims(const Gr1csDev& g, const Gr1csPred& P, bool with_domain, uint32_t log_n, uint32_t two_adicity,
                                   ColumnsDims* d, std::string* why) {
  d->n = P.n;
  d->cols = (uint64_t)P.arity * g.m;
  d->nnz = 0;
  d->max_nnz = 0;
  for (uint32_t k = 0; k < P.arity; k++) {
    d->nnz += P.nnz[k];
    d->max_nnz = std::max(d->max_nnz, P.nnz[k]);
  }
  if (with_domain) {
    uint32_t log_domain = log_n;
    if (log_n == 0) {
      log_domain = 1;
      while ((1ull << log_domain) < P.n) log_domain++;
    }
    d->log_domain = log_domain;
    if (log_domain > two_adicity) {
      *why = "the evaluation domain exceeds the largest radix-2 domain of Fr";
      return ARK355_E_POLY_DEGREE_TOO_LARGE;
    }
    if ((1ull << log_domain) < P.n) {
      *why = "2^log_n is below the predicate's row count";
      return ARK355_EINVAL;
    }
  }
  if (d->cols + 1 >= (1ull << 32)) {
    *why = "arity * (num_instance + num_witness) + 1 must stay below 2^32";
    return ARK355_EINVAL;
  }
  if (d->nnz >= (1ull << 32)) {
    *why = "the non-zeros of the predicate's matrices together must stay below 2^32";
    return ARK355_EINVAL;
  }
  return ARK355_OK;
}

// every buffer of columns_run at its size for this call: the one place that may allocate, before the first launch
template <class Fr>
static void columns_reserve(ColumnsScratch& cs, const ColumnsDims& d, uint32_t lane_max) {
  colgather_reserve(cs.gather, d.cols, d.nnz, lane_max, sizeof(Fr));
}

// d_out (t m Fr, Montgomery, matrix-major) = the transposed products with d_y (n Fr) on `st`; every element is written.  The
// scratch was reserved by columns_reserve with the same d and lane_max.  One host wait (the heavy counter); the last kernels
// are queued, not waited for.
template <class Curve>
static void columns_run(const Gr1csDev& g, const Gr1csPred& P, const ColumnsDims& d, const void* d_y, void* d_out,
                        ColumnsScratch& cs, uint32_t lane_max, hipStream_t st) {
  using Fr = typename Curve::Fr;
  ColGatherIn in;
  in.mats = P.mats.as<Gr1csMat>();
  in.t = P.arity;
  in.n = (uint32_t)d.n;
  in.m = (uint32_t)g.m;
  in.nnz = d.nnz;
  in.max_nnz = d.max_nnz;
  colgather_run<FrTerms<Fr>>(in, (const Fr*)d_y, (const Fr*)g.pool.as<Fr>(), (Fr*)d_out, cs.gather, lane_max, st);
}

}  // namespace ark355
