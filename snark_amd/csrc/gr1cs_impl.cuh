// GR1CS on the device: every predicate of a constraint system, not only "R1CS".
//
// ark-relations keeps a BTreeMap<Label, PredicateConstraintSystem> (gr1cs/constraint_system.rs:44-97); a predicate is a
// sparse multivariate polynomial P of arity t over t matrices (gr1cs/predicate/polynomial_constraint.rs), row i is
// satisfied iff P(<M_0[i], z>, .., <M_{t-1}[i], z>) == 0, and which_is_unsatisfied (constraint_system.rs:652-687) walks
// the labels in BTreeMap order, the rows ascending.
//
//   gr1cs_spmv_kernel   M_k z for the t matrices of one predicate: the row-per-lane SpMV of witness_impl.cuh with the
//                       matrix selected by blockIdx.y through a device table (any t, no pointer arguments per matrix)
//   gr1cs_pred_kernel   one lane per row: the row's t inner products, then the polynomial.
//                         EVAL = false: a failing row folds (rank of the label << 40 | row) into ONE 64-bit word with
//                                       atomicMin -- the whole system costs one 8-byte copy back and writes no vector;
//                         EVAL = true:  the residual P(..)_i is written instead.
//
// The polynomial is a small program of 32-bit words, the same for every lane, in device memory behind a kernel-argument
// pointer and read at wave-uniform addresses (scalar loads; the loops over terms, factors and exponent bits are
// wave-uniform, no lane diverges on them):
//     n_terms, then per term: pool index of the coefficient, n_factors, n_factors x (variable, exponent).
// A factor names its variable at RUN time, and a per-lane register array indexed at run time would live in scratch; the t
// values therefore sit in LDS, limb-major ([argument][limb][lane] as 32-bit words: consecutive lanes hit consecutive
// banks) and a factor reads its own lane's eight words back.  No lane reads another lane's words: no barrier.  The
// workgroup is sized by the arity so that the values take at most 32 KiB (gr1cs_block_size): several workgroups per CU
// at every arity and no need to raise the dynamic-LDS limit.
#pragma once
#include <algorithm>
#include <string>
#include "common.h"
#include "witness_impl.cuh"

namespace ark355 {

struct Gr1csPred {
  std::string label;
  uint32_t arity = 0;
  uint32_t rank = 0;             // position of the label in byte-wise lexicographic order
  uint64_t n = 0;
  bool r1cs_shape = false;       // arity 3 and the polynomial is x0 x1 - x2
  uint64_t degree = 0;           // total degree of the polynomial as written (gr1cs_program_degree): quotient_impl.cuh
  std::vector<uint64_t> nnz;
  std::vector<DevBuf> row_ptr, col, cidx;
  DevBuf mats;                   // arity x Gr1csMat
  DevBuf prog;
};

struct Gr1csDev {
  int curve = 0;
  int device = -1;                         // the device of the context that built it (capi.hip); -1: not recorded
  uint64_t ell = 0, w = 0, m = 0, total = 0;
  std::vector<Gr1csPred> preds;            // in the caller's order
  DevBuf pool;                             // interned coefficients of all matrices and polynomials; pool[0] == 1
  size_t pool_count = 0;
};

constexpr uint32_t GR1CS_LDS_BYTES = 32u << 10;
// lanes per workgroup of gr1cs_pred_kernel: the largest of 256 / 128 / 64 whose values fit GR1CS_LDS_BYTES
static inline uint32_t gr1cs_block_size(uint32_t arity, uint32_t fr_bytes) {
  uint32_t b = 256;
  while (b > 64 && b * arity * fr_bytes > GR1CS_LDS_BYTES) b >>= 1;
  return b;
}

// <M[i], z>: mat_vec_mul (utils/matrix.rs:26-36); a coefficient equal to one (pool index 0) skips the multiply
template <class Fr>
ARK_D Fr gr1cs_row_dot(const Gr1csMat m, const Fr* __restrict__ pool, const Fr* __restrict__ z, uint64_t i) {
  Fr acc = Fr::zero();
  const uint32_t lo = m.rp[i], hi = m.rp[i + 1];
  for (uint32_t k = lo; k < hi; k++) {
    Fr v = z[m.col[k]];
    const uint32_t c = m.ci[k];
    if (c != 0) v = Fr::mul(v, pool[c]);
    acc = Fr::add(acc, v);
  }
  return acc;
}

template <class Fr>
__global__ void __launch_bounds__(256)
gr1cs_spmv_kernel(const Gr1csMat* __restrict__ mats, const Fr* __restrict__ pool, const Fr* __restrict__ z, uint64_t n,
                  Fr* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Gr1csMat m = mats[blockIdx.y];
  out[(uint64_t)blockIdx.y * n + i] = gr1cs_row_dot<Fr>(m, pool, z, i);
}

// x^e for a wave-uniform e >= 1: square-and-multiply from the top bit
template <class Fr>
ARK_D Fr gr1cs_pow(const Fr& x, uint32_t e) {
  uint32_t b = 31;
  while (!((e >> b) & 1u)) b--;
  Fr r = x;
  while (b--) {
    r = Fr::sqr(r);
    if ((e >> b) & 1u) r = Fr::mul(r, x);
  }
  return r;
}

template <class Fr, bool EVAL>
__global__ void __launch_bounds__(256)
gr1cs_pred_kernel(const Gr1csMat* __restrict__ mats, uint32_t arity, const uint32_t* __restrict__ prog,
                  const Fr* __restrict__ pool, const Fr* __restrict__ z, uint64_t n, unsigned long long key_hi,
                  unsigned long long* __restrict__ first_bad, Fr* __restrict__ out) {
  ARK_DYN_SMEM(uint32_t, vals);            // [arity][Fr::N][blockDim.x]
  const uint32_t lane = threadIdx.x, stride = blockDim.x;
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + lane;
  if (i >= n) return;                      // no barrier below: a lane touches its own words only
  for (uint32_t k = 0; k < arity; k++) {
    const Gr1csMat m = mats[k];
    const Fr v = gr1cs_row_dot<Fr>(m, pool, z, i);
#pragma unroll
    for (int l = 0; l < Fr::N; l++) vals[(k * Fr::N + l) * stride + lane] = v.l[l];
  }
  Fr acc = Fr::zero();
  const uint32_t n_terms = prog[0];
  uint32_t pc = 1;
  for (uint32_t t = 0; t < n_terms; t++) {
    const uint32_t ci = prog[pc], n_factors = prog[pc + 1];
    pc += 2;
    bool have = false;
    Fr prod = Fr::zero();
    for (uint32_t f = 0; f < n_factors; f++) {
      const uint32_t var = prog[pc], e = prog[pc + 1];
      pc += 2;
      if (e == 0) continue;                // x^0 = 1
      Fr x;
#pragma unroll
      for (int l = 0; l < Fr::N; l++) x.l[l] = vals[(var * Fr::N + l) * stride + lane];
      const Fr pw = gr1cs_pow<Fr>(x, e);
      prod = have ? Fr::mul(prod, pw) : pw;
      have = true;
    }
    Fr term = pool[ci];                    // a term without factors is the constant term
    if (have) term = ci ? Fr::mul(prod, term) : prod;
    acc = Fr::add(acc, term);
  }
  if (EVAL) {
    out[i] = acc;
  } else if (!acc.is_zero()) {
    atomicMin(first_bad, key_hi | (unsigned long long)i);
  }
}

constexpr int GR1CS_ROW_BITS = 40;         // key = rank << 40 | row: rows < 2^32, ranks < 2^24

// x0 x1 - x2, however the host wrote it (term order, factor order, x^0 factors)
template <class Fr>
static bool gr1cs_is_r1cs_polynomial(const ark355_predicate_desc& d) {
  if (d.arity != 3) return false;
  // monomial = exponent vector; coefficient sums by monomial
  std::map<std::vector<uint64_t>, Fr> sum;
  for (uint32_t k = 0; k < d.n_terms; k++) {
    std::vector<uint64_t> mono(3, 0);
    for (uint32_t j = d.term_ptr[k]; j < d.term_ptr[k + 1]; j++) mono[d.term_var[j]] += d.term_exp[j];
    Fr c;
    memcpy(c.l, d.term_coeff + (size_t)k * sizeof(Fr), sizeof(Fr));
    auto it = sum.find(mono);
    if (it == sum.end()) sum.emplace(mono, c);
    else it->second = Fr::add(it->second, c);
  }
  size_t nonzero = 0;
  for (auto& kv : sum) {
    if (kv.second.is_zero()) continue;
    nonzero++;
    if (kv.first == std::vector<uint64_t>{1, 1, 0}) {
      if (kv.second != Fr::one()) return false;
    } else if (kv.first == std::vector<uint64_t>{0, 0, 1}) {
      if (kv.second != Fr::neg(Fr::one())) return false;
    } else {
      return false;
    }
  }
  return nonzero == 2;
}

// what ark355_gr1cs_load and ark355_gr1cs_from_lcs refuse about the head and the polynomial of a predicate
static inline void gr1cs_validate_polynomial(const std::string& who, uint32_t arity, uint64_t n_constraints, uint32_t n_terms,
                                             const uint8_t* term_coeff, const uint32_t* term_ptr, const uint32_t* term_var,
                                             const uint32_t* term_exp) {
  ARK_REQUIRE(arity >= 1, ARK355_EINVAL, who + "arity 0");
  ARK_REQUIRE(arity <= ARK355_GR1CS_MAX_ARITY, ARK355_EINVAL, who + "arity above ARK355_GR1CS_MAX_ARITY");
  ARK_REQUIRE(n_terms <= ARK355_GR1CS_MAX_TERMS, ARK355_EINVAL, who + "more terms than ARK355_GR1CS_MAX_TERMS");
  ARK_REQUIRE(n_constraints <= ARK355_GR1CS_MAX_ROWS, ARK355_EINVAL, who + "more rows than ARK355_GR1CS_MAX_ROWS");
  ARK_REQUIRE(n_terms == 0 || (term_ptr && term_coeff), ARK355_EINVAL, who + "term_ptr / term_coeff is NULL");
  ARK_REQUIRE(n_terms == 0 || term_ptr[0] == 0, ARK355_EINVAL, who + "term_ptr must start at 0");
  for (uint32_t k = 0; k < n_terms; k++) {
    ARK_REQUIRE(term_ptr[k + 1] >= term_ptr[k], ARK355_EINVAL, who + "term_ptr must be non-decreasing");
    ARK_REQUIRE(term_ptr[k + 1] <= ARK355_GR1CS_MAX_FACTORS, ARK355_EINVAL, who + "more factors than ARK355_GR1CS_MAX_FACTORS");
  }
  const uint32_t n_factors = n_terms ? term_ptr[n_terms] : 0;
  ARK_REQUIRE(n_factors == 0 || (term_var && term_exp), ARK355_EINVAL, who + "term_var / term_exp is NULL");
  for (uint32_t j = 0; j < n_factors; j++)
    ARK_REQUIRE(term_var[j] < arity, ARK355_EINVAL, who + "term_var names a variable >= arity");
}

// the polynomial as the program gr1cs_pred_kernel reads; its coefficients are interned into `pool`
template <class Fr>
static std::vector<uint32_t> gr1cs_program(FrInterner<Fr>& pool, uint32_t n_terms, const uint8_t* term_coeff, const uint32_t* term_ptr,
                                           const uint32_t* term_var, const uint32_t* term_exp) {
  std::vector<uint32_t> prog;
  prog.push_back(n_terms);
  for (uint32_t k = 0; k < n_terms; k++) {
    prog.push_back(pool.intern(term_coeff + (size_t)k * sizeof(Fr)));
    prog.push_back(term_ptr[k + 1] - term_ptr[k]);
    for (uint32_t j = term_ptr[k]; j < term_ptr[k + 1]; j++) {
      prog.push_back(term_var[j]);
      prog.push_back(term_exp[j]);
    }
  }
  return prog;
}

// total degree of a program: the maximum over its terms of the sum of the exponents, in 64 bits (an exponent is any uint32_t);
// a term counts whatever its coefficient, x^0 contributes 0
static inline uint64_t gr1cs_program_degree(const std::vector<uint32_t>& prog) {
  uint64_t degree = 0;
  size_t pc = 1;
  for (uint32_t t = 0; t < prog[0]; t++) {
    const uint32_t n_factors = prog[pc + 1];
    pc += 2;
    uint64_t sum = 0;
    for (uint32_t f = 0; f < n_factors; f++, pc += 2) sum += prog[pc + 1];
    degree = std::max(degree, sum);
  }
  return degree;
}

// the labels in byte-wise lexicographic order, as BTreeMap<String, _> iterates: order[rank] = the caller's index
static inline std::vector<uint32_t> gr1cs_label_order(const std::vector<const char*>& labels) {
  std::vector<uint32_t> order(labels.size());
  for (uint32_t p = 0; p < order.size(); p++) order[p] = p;
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    const size_t la = strlen(labels[a]), lb = strlen(labels[b]);
    const int c = memcmp(labels[a], labels[b], la < lb ? la : lb);
    return c != 0 ? c < 0 : la < lb;
  });
  return order;
}

template <class Curve>
static Gr1csDev* gr1cs_upload(uint64_t ell, uint64_t w, const ark355_predicate_desc* preds, uint32_t n_preds) {
  using Fr = typename Curve::Fr;
  std::unique_ptr<Gr1csDev> g(new Gr1csDev());
  g->curve = Curve::ID;
  g->ell = ell;
  g->w = w;
  g->m = ell + w;
  ARK_REQUIRE(ell >= 1, ARK355_EINVAL, "num_instance must include the constant One");
  ARK_REQUIRE(ell < (1ull << 31) && w < (1ull << 31) && g->m < (1ull << 31), ARK355_EINVAL, "too many variables");
  ARK_REQUIRE(n_preds <= ARK355_GR1CS_MAX_PREDICATES, ARK355_EINVAL, "more predicates than ARK355_GR1CS_MAX_PREDICATES");
  ARK_REQUIRE(n_preds == 0 || preds, ARK355_EINVAL, "preds is NULL");
  // ---- everything is validated before the first device allocation ---------------------------------------------------
  for (uint32_t p = 0; p < n_preds; p++) {
    const ark355_predicate_desc& d = preds[p];
    ARK_REQUIRE(d.label, ARK355_EINVAL, "predicate " + std::to_string(p) + ": label is NULL");
    const std::string who = "predicate \"" + std::string(d.label) + "\": ";
    gr1cs_validate_polynomial(who, d.arity, d.n_constraints, d.n_terms, d.term_coeff, d.term_ptr, d.term_var, d.term_exp);
    ARK_REQUIRE(d.row_ptr && d.col && d.coeff, ARK355_EINVAL, who + "row_ptr / col / coeff is NULL");
    for (uint32_t k = 0; k < d.arity; k++) {
      const std::string mat = who + "matrix " + std::to_string(k) + ": ";
      ARK_REQUIRE(d.row_ptr[k], ARK355_EINVAL, mat + "row_ptr is NULL");
      const uint64_t* rp = d.row_ptr[k];
      ARK_REQUIRE(rp[0] == 0, ARK355_EINVAL, mat + "row_ptr must start at 0");
      for (uint64_t i = 0; i < d.n_constraints; i++) {
        ARK_REQUIRE(rp[i + 1] >= rp[i], ARK355_EINVAL, mat + "row_ptr must be non-decreasing");
        ARK_REQUIRE(rp[i + 1] <= ARK355_GR1CS_MAX_ROWS, ARK355_EINVAL, mat + "more entries than ARK355_GR1CS_MAX_ROWS");
      }
      const uint64_t nnz = rp[d.n_constraints];
      ARK_REQUIRE(nnz == 0 || (d.col[k] && d.coeff[k]), ARK355_EINVAL, mat + "col / coeff is NULL");
      for (uint64_t e = 0; e < nnz; e++) ARK_REQUIRE(d.col[k][e] < g->m, ARK355_EINVAL, mat + "column index out of range");
    }
    for (uint32_t q = 0; q < p; q++)
      ARK_REQUIRE(strcmp(preds[q].label, d.label) != 0, ARK355_EINVAL, who + "duplicate label");
  }
  // ---- ranks of the labels: byte-wise lexicographic, as BTreeMap<String, _> iterates -----------------------------------
  std::vector<const char*> labels(n_preds);
  for (uint32_t p = 0; p < n_preds; p++) labels[p] = preds[p].label;
  const std::vector<uint32_t> order = gr1cs_label_order(labels);
  // ---- upload ------------------------------------------------------------------------------------------------------------
  FrInterner<Fr> pool;
  g->preds.resize(n_preds);
  for (uint32_t r = 0; r < n_preds; r++) g->preds[order[r]].rank = r;
  for (uint32_t p = 0; p < n_preds; p++) {
    const ark355_predicate_desc& d = preds[p];
    Gr1csPred& P = g->preds[p];
    P.label = d.label;
    P.arity = d.arity;
    P.n = d.n_constraints;
    P.r1cs_shape = gr1cs_is_r1cs_polynomial<Fr>(d);
    g->total += P.n;
    const std::vector<uint32_t> prog = gr1cs_program<Fr>(pool, d.n_terms, d.term_coeff, d.term_ptr, d.term_var, d.term_exp);
    P.degree = gr1cs_program_degree(prog);
    P.prog.alloc(prog.size() * 4);
    ARK_CHECK_HIP(hipMemcpy(P.prog.p, prog.data(), prog.size() * 4, hipMemcpyHostToDevice));
    P.nnz.resize(d.arity);
    P.row_ptr.resize(d.arity);
    P.col.resize(d.arity);
    P.cidx.resize(d.arity);
    std::vector<Gr1csMat> mats(d.arity);
    for (uint32_t k = 0; k < d.arity; k++) {
      const uint64_t n = P.n, nnz = d.row_ptr[k][n];
      P.nnz[k] = nnz;
      std::vector<uint32_t> rp(n + 1), ci(nnz);
      for (uint64_t i = 0; i <= n; i++) rp[i] = (uint32_t)d.row_ptr[k][i];
      for (uint64_t e = 0; e < nnz; e++) ci[e] = pool.intern(d.coeff[k] + e * sizeof(Fr));
      P.row_ptr[k].alloc((n + 1) * 4);
      P.col[k].alloc(nnz * 4);
      P.cidx[k].alloc(nnz * 4);
      ARK_CHECK_HIP(hipMemcpy(P.row_ptr[k].p, rp.data(), (n + 1) * 4, hipMemcpyHostToDevice));
      if (nnz) {
        ARK_CHECK_HIP(hipMemcpy(P.col[k].p, d.col[k], nnz * 4, hipMemcpyHostToDevice));
        ARK_CHECK_HIP(hipMemcpy(P.cidx[k].p, ci.data(), nnz * 4, hipMemcpyHostToDevice));
      }
      mats[k] = Gr1csMat{P.row_ptr[k].as<uint32_t>(), P.col[k].as<uint32_t>(), P.cidx[k].as<uint32_t>()};
    }
    P.mats.alloc(d.arity * sizeof(Gr1csMat));
    ARK_CHECK_HIP(hipMemcpy(P.mats.p, mats.data(), d.arity * sizeof(Gr1csMat), hipMemcpyHostToDevice));
  }
  g->pool_count = pool.elems.size();
  g->pool.alloc(g->pool_count * sizeof(Fr));
  ARK_CHECK_HIP(hipMemcpy(g->pool.p, pool.elems.data(), g->pool_count * sizeof(Fr), hipMemcpyHostToDevice));
  return g.release();
}

// the fused check of every predicate with rows; *first_bad (device) = the smallest (rank << 40 | row) that fails, or ~0
template <class Curve>
static void gr1cs_check_run(const Gr1csDev& g, const void* d_z, unsigned long long* d_first_bad, hipStream_t stream) {
  using Fr = typename Curve::Fr;
  ARK_CHECK_HIP(hipMemsetAsync(d_first_bad, 0xFF, 8, stream));
  for (const Gr1csPred& P : g.preds) {
    if (!P.n) continue;
    const uint32_t block = gr1cs_block_size(P.arity, sizeof(Fr));
    const uint32_t grid = (uint32_t)((P.n + block - 1) / block);
    ARK_LAUNCH((gr1cs_pred_kernel<Fr, false>), dim3(grid), dim3(block), (size_t)block * P.arity * sizeof(Fr), stream,
               (const Gr1csMat*)P.mats.as<Gr1csMat>(), P.arity, (const uint32_t*)P.prog.as<uint32_t>(), (const Fr*)g.pool.as<Fr>(),
               (const Fr*)d_z, P.n, (unsigned long long)P.rank << GR1CS_ROW_BITS, d_first_bad, (Fr*)nullptr);
    ARK_CHECK_LAUNCH();
  }
}

// residual of every row of one predicate -> d_out (n Fr)
template <class Curve>
static void gr1cs_eval_run(const Gr1csDev& g, const Gr1csPred& P, const void* d_z, void* d_out, hipStream_t stream) {
  using Fr = typename Curve::Fr;
  if (!P.n) return;
  const uint32_t block = gr1cs_block_size(P.arity, sizeof(Fr));
  const uint32_t grid = (uint32_t)((P.n + block - 1) / block);
  ARK_LAUNCH((gr1cs_pred_kernel<Fr, true>), dim3(grid), dim3(block), (size_t)block * P.arity * sizeof(Fr), stream,
             (const Gr1csMat*)P.mats.as<Gr1csMat>(), P.arity, (const uint32_t*)P.prog.as<uint32_t>(), (const Fr*)g.pool.as<Fr>(),
             (const Fr*)d_z, P.n, 0ull, (unsigned long long*)nullptr, (Fr*)d_out);
  ARK_CHECK_LAUNCH();
}

// M_k z for the arity matrices of one predicate -> d_out (arity x n Fr, matrix-major)
template <class Curve>
static void gr1cs_spmv_run(const Gr1csDev& g, const Gr1csPred& P, const void* d_z, void* d_out, hipStream_t stream) {
  using Fr = typename Curve::Fr;
  if (!P.n) return;
  const uint32_t grid = (uint32_t)((P.n + 255) / 256);
  ARK_LAUNCH((gr1cs_spmv_kernel<Fr>), dim3(grid, P.arity), dim3(256), 0, stream, (const Gr1csMat*)P.mats.as<Gr1csMat>(),
             (const Fr*)g.pool.as<Fr>(), (const Fr*)d_z, P.n, (Fr*)d_out);
  ARK_CHECK_LAUNCH();
}

// An R1csDev from the predicate labelled "R1CS": device-to-device copies of the resident CSR arrays and of the pool (whose
// indices they carry; the other predicates' coefficients in it are never referenced).  Refuses when that would drop a
// constraint: Groth16 proves R1CS only.
template <class Curve>
static R1csDev* gr1cs_to_r1cs(const Gr1csDev& g, hipStream_t stream) {
  using Fr = typename Curve::Fr;
  const Gr1csPred* R = nullptr;
  for (const Gr1csPred& P : g.preds) {
    if (P.label == "R1CS") {
      R = &P;
    } else {
      ARK_REQUIRE(P.n == 0, ARK355_EINVAL,
                  "predicate \"" + P.label + "\" carries " + std::to_string(P.n) +
                      " constraints: only R1CS can be proved, and they would be dropped");
    }
  }
  ARK_REQUIRE(R, ARK355_EINVAL, "no predicate is labelled \"R1CS\"");
  ARK_REQUIRE(R->r1cs_shape, ARK355_EINVAL, "the predicate labelled \"R1CS\" is not x0 * x1 - x2 of arity 3");
  std::unique_ptr<R1csDev> r(new R1csDev());
  r1cs_set_dims<Curve>(r.get(), R->n, g.ell, g.w);
  for (int k = 0; k < 3; k++) {
    r->nnz[k] = R->nnz[k];
    r->row_ptr[k].alloc(R->row_ptr[k].bytes);
    r->col[k].alloc(R->col[k].bytes);
    r->cidx[k].alloc(R->cidx[k].bytes);
    ARK_CHECK_HIP(hipMemcpyAsync(r->row_ptr[k].p, R->row_ptr[k].p, (R->n + 1) * 4, hipMemcpyDeviceToDevice, stream));
    if (R->nnz[k]) {
      ARK_CHECK_HIP(hipMemcpyAsync(r->col[k].p, R->col[k].p, R->nnz[k] * 4, hipMemcpyDeviceToDevice, stream));
      ARK_CHECK_HIP(hipMemcpyAsync(r->cidx[k].p, R->cidx[k].p, R->nnz[k] * 4, hipMemcpyDeviceToDevice, stream));
    }
  }
  r->pool.alloc(g.pool_count * sizeof(Fr));
  ARK_CHECK_HIP(hipMemcpyAsync(r->pool.p, g.pool.p, g.pool_count * sizeof(Fr), hipMemcpyDeviceToDevice, stream));
  r1cs_upload_mats(r.get());
  r1cs_upload_zinv<Curve>(r.get());
  ARK_CHECK_HIP(hipStreamSynchronize(stream));
  return r.release();
}

// the coefficients of one matrix as field elements
template <class Fr>
__global__ void __launch_bounds__(256)
gr1cs_coeff_kernel(const uint32_t* __restrict__ ci, const Fr* __restrict__ pool, uint64_t nnz, Fr* __restrict__ out) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nnz) return;
  out[e] = pool[ci[e]];
}

// to_matrices() of a resident system (constraint_system.rs:768-774): matrix `which` of one predicate in the CSR convention of
// ark355_r1cs_load; tmp: grow-only scratch for the gathered coefficients
template <class Curve>
static void gr1cs_matrix(const Gr1csDev& g, const Gr1csPred& Q, uint32_t which, uint64_t* row_ptr, uint32_t* col, uint8_t* coeff,
                         DevBuf& tmp, hipStream_t st) {
  using Fr = typename Curve::Fr;
  const uint64_t nnz = Q.nnz[which];
  std::vector<uint32_t> rp(Q.n + 1);
  ARK_CHECK_HIP(hipMemcpyAsync(rp.data(), Q.row_ptr[which].p, (Q.n + 1) * 4, hipMemcpyDeviceToHost, st));
  if (nnz) {
    tmp.ensure(nnz * sizeof(Fr));
    ARK_LAUNCH((gr1cs_coeff_kernel<Fr>), dim3((uint32_t)((nnz + 255) / 256)), dim3(256), 0, st,
               (const uint32_t*)Q.cidx[which].as<uint32_t>(), (const Fr*)g.pool.as<Fr>(), nnz, tmp.as<Fr>());
    ARK_CHECK_LAUNCH();
    ARK_CHECK_HIP(hipMemcpyAsync(col, Q.col[which].p, nnz * 4, hipMemcpyDeviceToHost, st));
    ARK_CHECK_HIP(hipMemcpyAsync(coeff, tmp.p, nnz * sizeof(Fr), hipMemcpyDeviceToHost, st));
  }
  ARK_CHECK_HIP(hipStreamSynchronize(st));
  for (uint64_t i = 0; i <= Q.n; i++) row_ptr[i] = rp[i];
}

}  // namespace ark355
