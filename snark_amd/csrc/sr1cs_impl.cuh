// Square R1CS on the device: Sr1csAdapter (relations/src/sr1cs/mod.rs:124-265) over a resident R1CS.
//
// The adapter rewrites n rows  <A_i,z><B_i,z> = <C_i,z>  into 2n + P rows of the predicate x0^2 - x1:
//     row 2i      (A_i + B_i)^2 = 4 C_i + s_i            s_i: a fresh witness, (<A_i,z> - <B_i,z>)^2
//     row 2i + 1  (A_i - B_i)^2 = s_i
//     row 2n+k-1  (v - x_k)^2   = 0                      one per public variable p_k that occurs: v its witness copy
// and renumbers the variables in the order its two BTreeMaps meet them: rows ascending, A then B then C, entries in stored
// order.  Every old column that occurs (column 0 apart) becomes a witness allocated at its first occurrence, the square
// variable of a row comes after the row's new variables, and the publics that occur become the inputs 1 .. P in ascending
// order of their old column (the BTreeMap's iteration, mod.rs:177-181 / :253-262).
//
// Once per circuit (sr1cs_build), on the context's stream, no matrix data on the host:
//   sr1cs_first_kernel    key[j] = min over the entries of column j of (row << 32 | matrix << 30 | position in row)
//   sr1cs_count_kernel    U_i = entries of row i whose column's key is their own; scan_exclusive -> F
//   sr1cs_pub_flag_kernel the publics that occur; scan_exclusive -> their ranks, P
//   sr1cs_number_kernel   col'(j) = 1 + P + F(i) + i + q(j), and the new input of a public
//   sr1cs_fill_kernel     row pointers (closed forms of the source's), remapped columns, coefficient indices
//   sr1cs_pool_kernel     pool' = pool || -pool || 4 pool: an entry keeps its source index ci (plus), or becomes ci + c
//                         (minus) or ci + 2c (times four) -- no interning, and index 0 stays one
// The result is an ordinary Gr1csDev (one predicate "SR1CS", rank 0): everything of gr1cs_impl.cuh runs on it.
//
// Once per proof (sr1cs_assign_run): sr1cs_assign_kernel, one lane per source row, computes <A_i,z> and <B_i,z>, their
// difference and its square, and stores it to z'[s_i]; it writes no Az or Bz vector.  sr1cs_scatter_kernel, one lane per
// old column, copies z[j] to col'(j) and, for a public that occurs, to its input as well.  No LDS, no barrier.
#pragma once
#include "common.h"
#include "msm_impl.cuh"
#include "gr1cs_impl.cuh"

namespace ark355 {

constexpr uint32_t SR1CS_UNUSED = 0xFFFFFFFFu;
constexpr uint32_t SR1CS_POS_BITS = 30;      // position of an entry in its row: rows of 2^30 entries and more are refused

struct Sr1csDev {
  int curve = 0, device = 0;
  uint64_t n = 0, ell = 0, w = 0, m = 0;     // the source
  uint64_t P = 0, U = 0;
  Gr1csDev sys;                              // the resident SR1CS system (borrowed by ark355_sr1cs_system)
  DevBuf rp[2], col[2], ci[2];               // A and B of the source: the assignment pass is independent of the r1cs handle
  DevBuf F;                                  // n + 1: F(i), F(n) = U
  DevBuf wit_col;                            // m: col'(j), 0 for column 0, SR1CS_UNUSED
  DevBuf inst_col;                           // ell: k for p_k, SR1CS_UNUSED
};

struct Sr1csSrc {
  const uint32_t* rp[3];
  const uint32_t* col[3];
  const uint32_t* ci[3];
};

ARK_D unsigned long long sr1cs_key(uint64_t row, uint32_t mat, uint32_t pos) {
  return (unsigned long long)row << 32 | (unsigned long long)mat << SR1CS_POS_BITS | pos;
}

// grid.y = matrix; flags[0] |= 1 when a row is too long for the key
static __global__ void __launch_bounds__(256)
sr1cs_first_kernel(const Sr1csSrc s, uint64_t n, unsigned long long* key, uint32_t* __restrict__ flags) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t mat = blockIdx.y;
  const uint32_t lo = s.rp[mat][i], hi = s.rp[mat][i + 1];
  if (hi - lo >= (1u << SR1CS_POS_BITS)) {
    atomicOr(flags, 1u);
    return;
  }
  for (uint32_t k = lo; k < hi; k++) {
    const uint32_t j = s.col[mat][k];
    if (j == 0) continue;
    const unsigned long long mine = sr1cs_key(i, mat, k - lo);
    // a column of every row (the bench circuits have them) settles after its first rows: read before the atomic
    if (mine < key[j]) atomicMin(&key[j], mine);
  }
}

static __global__ void __launch_bounds__(256)
sr1cs_count_kernel(const Sr1csSrc s, uint64_t n, const unsigned long long* __restrict__ key, uint32_t* __restrict__ count) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t u = 0;
  for (uint32_t mat = 0; mat < 3; mat++) {
    const uint32_t lo = s.rp[mat][i], hi = s.rp[mat][i + 1];
    for (uint32_t k = lo; k < hi; k++) {
      const uint32_t j = s.col[mat][k];
      if (j != 0 && key[j] == sr1cs_key(i, mat, k - lo)) u++;
    }
  }
  count[i] = u;
}

static __global__ void __launch_bounds__(256)
sr1cs_pub_flag_kernel(const unsigned long long* __restrict__ key, uint64_t ell, uint32_t* __restrict__ flag) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= ell) return;
  flag[j] = (j != 0 && key[j] != ~0ull) ? 1u : 0u;
}

// lanes [0, n): the new variables of row i, in walk order; lanes [n, n + m): the columns that never occur, column 0 and the
// inputs.  pub_rank[ell] = P (the scan's total).
static __global__ void __launch_bounds__(256)
sr1cs_number_kernel(const Sr1csSrc s, uint64_t n, uint64_t ell, uint64_t m, const unsigned long long* __restrict__ key,
                    const uint32_t* __restrict__ F, const uint32_t* __restrict__ pub_flag,
                    const uint32_t* __restrict__ pub_rank, uint32_t* __restrict__ wit_col, uint32_t* __restrict__ inst_col) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n + m) return;
  if (t >= n) {
    const uint64_t j = t - n;
    if (j == 0) wit_col[0] = 0;
    else if (key[j] == ~0ull) wit_col[j] = SR1CS_UNUSED;
    if (j < ell) inst_col[j] = pub_flag[j] ? pub_rank[j] + 1 : SR1CS_UNUSED;
    return;
  }
  const uint64_t i = t;
  uint32_t next = 1 + pub_rank[ell] + F[i] + (uint32_t)i;
  for (uint32_t mat = 0; mat < 3; mat++) {
    const uint32_t lo = s.rp[mat][i], hi = s.rp[mat][i + 1];
    for (uint32_t k = lo; k < hi; k++) {
      const uint32_t j = s.col[mat][k];
      if (j != 0 && key[j] == sr1cs_key(i, mat, k - lo)) wit_col[j] = next++;
    }
  }
}

struct Sr1csOut {
  uint32_t* rp[2];
  uint32_t* col[2];
  uint32_t* ci[2];
};

// lanes [0, n): source row i -> rows 2i and 2i + 1 of both matrices; lanes [n, n + ell): the equality row of a public that
// occurs; lane n + ell: the last row pointers.  c: size of the source pool (minus = + c, times four = + 2c).
static __global__ void __launch_bounds__(256)
sr1cs_fill_kernel(const Sr1csSrc s, uint64_t n, uint64_t ell, uint32_t nnz_ab, uint32_t nnz_c, uint32_t c, uint32_t P,
                  const uint32_t* __restrict__ F, const uint32_t* __restrict__ wit_col,
                  const uint32_t* __restrict__ inst_col, const Sr1csOut o) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t > n + ell) return;
  const uint32_t eq0 = 2 * nnz_ab, eq1 = nnz_c + 2 * (uint32_t)n;      // where the equality rows start
  if (t == n + ell) {
    o.rp[0][2 * n + P] = eq0 + 2 * P;
    o.rp[1][2 * n + P] = eq1;
    return;
  }
  if (t >= n) {
    const uint64_t j = t - n;
    const uint32_t k = inst_col[j];
    if (k == SR1CS_UNUSED) return;
    const uint32_t at = eq0 + 2 * (k - 1);
    o.rp[0][2 * n + k - 1] = at;
    o.rp[1][2 * n + k - 1] = eq1;
    o.col[0][at] = wit_col[j];
    o.ci[0][at] = 0;
    o.col[0][at + 1] = k;
    o.ci[0][at + 1] = c;               // -1
    return;
  }
  const uint64_t i = t;
  const uint32_t a_lo = s.rp[0][i], a_hi = s.rp[0][i + 1], b_lo = s.rp[1][i], b_hi = s.rp[1][i + 1];
  const uint32_t c_lo = s.rp[2][i], c_hi = s.rp[2][i + 1];
  const uint32_t len = (a_hi - a_lo) + (b_hi - b_lo);
  const uint32_t sq = 1 + P + F[i + 1] + (uint32_t)i;
  uint32_t plus = 2 * (a_lo + b_lo), minus = plus + len;
  o.rp[0][2 * i] = plus;
  o.rp[0][2 * i + 1] = minus;
  for (uint32_t k = a_lo; k < a_hi; k++) {
    const uint32_t cl = wit_col[s.col[0][k]], ci = s.ci[0][k];
    o.col[0][plus] = cl;
    o.ci[0][plus++] = ci;
    o.col[0][minus] = cl;
    o.ci[0][minus++] = ci;
  }
  for (uint32_t k = b_lo; k < b_hi; k++) {
    const uint32_t cl = wit_col[s.col[1][k]], ci = s.ci[1][k];
    o.col[0][plus] = cl;
    o.ci[0][plus++] = ci;
    o.col[0][minus] = cl;
    o.ci[0][minus++] = ci + c;
  }
  uint32_t at = c_lo + 2 * (uint32_t)i;
  o.rp[1][2 * i] = at;
  for (uint32_t k = c_lo; k < c_hi; k++) {
    o.col[1][at] = wit_col[s.col[2][k]];
    o.ci[1][at++] = s.ci[2][k] + 2 * c;
  }
  o.col[1][at] = sq;
  o.ci[1][at++] = 0;
  o.rp[1][2 * i + 1] = at;
  o.col[1][at] = sq;
  o.ci[1][at] = 0;
}

template <class Fr>
__global__ void __launch_bounds__(256)
sr1cs_pool_kernel(const Fr* __restrict__ pool, uint32_t c, Fr* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c) return;
  const Fr v = pool[i];
  out[i] = v;
  out[c + i] = Fr::neg(v);
  out[2 * c + i] = Fr::dbl(Fr::dbl(v));
}

// z'[s_i] = (<A_i,z> - <B_i,z>)^2: evaluate_constraint twice (mod.rs:24-56, :214-238)
template <class Fr>
__global__ void __launch_bounds__(256)
sr1cs_assign_kernel(const Gr1csMat A, const Gr1csMat B, const Fr* __restrict__ pool, const Fr* __restrict__ z, uint64_t n,
                    uint32_t ell_new, const uint32_t* __restrict__ F, Fr* __restrict__ z_out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Fr a = gr1cs_row_dot<Fr>(A, pool, z, i);
  const Fr b = gr1cs_row_dot<Fr>(B, pool, z, i);
  z_out[(uint64_t)ell_new + F[i + 1] + i] = Fr::sqr(Fr::sub(a, b));
}

template <class Fr>
__global__ void __launch_bounds__(256)
sr1cs_scatter_kernel(const Fr* __restrict__ z, uint64_t m, uint64_t ell, const uint32_t* __restrict__ wit_col,
                     const uint32_t* __restrict__ inst_col, Fr* __restrict__ z_out) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  if (j == 0) {
    z_out[0] = Fr::one();
    return;
  }
  const uint32_t cl = wit_col[j];
  if (cl == SR1CS_UNUSED) return;
  const Fr v = z[j];
  z_out[cl] = v;
  if (j < ell) z_out[inst_col[j]] = v;       // a public that occurs has an input
}

static inline uint32_t sr1cs_grid(uint64_t lanes) { return (uint32_t)((lanes + 255) / 256); }

template <class Curve>
static Sr1csDev* sr1cs_build(const R1csDev& r, int device, hipStream_t st) {
  using Fr = typename Curve::Fr;
  ARK_REQUIRE(r.curve == Curve::ID, ARK355_EINVAL, "ark355_sr1cs_from_r1cs: the r1cs handle belongs to another curve");
  const uint64_t n = r.n, ell = r.ell, m = r.m;
  const uint64_t nnz_ab = r.nnz[0] + r.nnz[1], nnz_c = r.nnz[2];
  // ---- what the host's numbers already decide, before any device work ------------------------------------------------
  ARK_REQUIRE(1 + n < (1ull << 31), ARK355_EINVAL, "ark355_sr1cs_from_r1cs: 1 + P + U + n reaches 2^31 variables");
  ARK_REQUIRE(2 * nnz_ab <= ARK355_GR1CS_MAX_ROWS, ARK355_EINVAL,
              "ark355_sr1cs_from_r1cs: the first matrix would hold more entries than ARK355_GR1CS_MAX_ROWS");
  ARK_REQUIRE(nnz_c + 2 * n <= ARK355_GR1CS_MAX_ROWS, ARK355_EINVAL,
              "ark355_sr1cs_from_r1cs: the second matrix would hold more entries than ARK355_GR1CS_MAX_ROWS");
  const uint64_t c = r.pool.bytes / sizeof(Fr);
  ARK_REQUIRE(c >= 1 && 3 * c < (1ull << 32), ARK355_EINVAL, "ark355_sr1cs_from_r1cs: coefficient pool too large");

  std::unique_ptr<Sr1csDev> s(new Sr1csDev());
  s->curve = Curve::ID;
  s->device = device;
  s->n = n;
  s->ell = ell;
  s->w = r.w;
  s->m = m;
  Sr1csSrc src;
  for (int k = 0; k < 3; k++) {
    src.rp[k] = r.row_ptr[k].as<uint32_t>();
    src.col[k] = r.col[k].as<uint32_t>();
    src.ci[k] = r.cidx[k].as<uint32_t>();
  }
  // ---- numbering ------------------------------------------------------------------------------------------------------
  DevBuf key(m * 8), count((n + 1) * 4), pub_flag(ell * 4), pub_rank((ell + 1) * 4), flags(4), aux;
  s->F.alloc((n + 1) * 4);
  s->wit_col.alloc(m * 4);
  s->inst_col.alloc(ell * 4);
  ARK_CHECK_HIP(hipMemsetAsync(key.p, 0xFF, m * 8, st));
  ARK_CHECK_HIP(hipMemsetAsync(flags.p, 0, 4, st));
  if (n) {
    ARK_LAUNCH(sr1cs_first_kernel, dim3(sr1cs_grid(n), 3), dim3(256), 0, st, src, n, key.as<unsigned long long>(), flags.as<uint32_t>());
    ARK_CHECK_LAUNCH();
    ARK_LAUNCH(sr1cs_count_kernel, dim3(sr1cs_grid(n)), dim3(256), 0, st, src, n, (const unsigned long long*)key.as<unsigned long long>(),
               count.as<uint32_t>());
    ARK_CHECK_LAUNCH();
  }
  scan_exclusive(st, count.as<const uint32_t>(), s->F.as<uint32_t>(), (uint32_t)n, s->F.as<uint32_t>() + n, aux);
  ARK_LAUNCH(sr1cs_pub_flag_kernel, dim3(sr1cs_grid(ell)), dim3(256), 0, st, (const unsigned long long*)key.as<unsigned long long>(), ell,
             pub_flag.as<uint32_t>());
  ARK_CHECK_LAUNCH();
  scan_exclusive(st, pub_flag.as<const uint32_t>(), pub_rank.as<uint32_t>(), (uint32_t)ell, pub_rank.as<uint32_t>() + ell, aux);
  ARK_LAUNCH(sr1cs_number_kernel, dim3(sr1cs_grid(n + m)), dim3(256), 0, st, src, n, ell, m,
             (const unsigned long long*)key.as<unsigned long long>(), (const uint32_t*)s->F.as<uint32_t>(),
             (const uint32_t*)pub_flag.as<uint32_t>(), (const uint32_t*)pub_rank.as<uint32_t>(), s->wit_col.as<uint32_t>(),
             s->inst_col.as<uint32_t>());
  ARK_CHECK_LAUNCH();
  // three words back: P, U and the long-row flag decide the sizes of everything below
  uint32_t hP = 0, hU = 0, hflags = 0;
  ARK_CHECK_HIP(hipMemcpyAsync(&hP, pub_rank.as<uint32_t>() + ell, 4, hipMemcpyDeviceToHost, st));
  ARK_CHECK_HIP(hipMemcpyAsync(&hU, s->F.as<uint32_t>() + n, 4, hipMemcpyDeviceToHost, st));
  ARK_CHECK_HIP(hipMemcpyAsync(&hflags, flags.p, 4, hipMemcpyDeviceToHost, st));
  ARK_CHECK_HIP(hipStreamSynchronize(st));
  ARK_REQUIRE(!(hflags & 1u), ARK355_EINVAL, "ark355_sr1cs_from_r1cs: a row holds 2^30 entries or more");
  const uint64_t P = hP, U = hU;
  ARK_REQUIRE(1 + P + U + n < (1ull << 31), ARK355_EINVAL, "ark355_sr1cs_from_r1cs: 1 + P + U + n reaches 2^31 variables");
  const uint64_t nnz0 = 2 * nnz_ab + 2 * P, nnz1 = nnz_c + 2 * n, rows = 2 * n + P;
  ARK_REQUIRE(nnz0 <= ARK355_GR1CS_MAX_ROWS, ARK355_EINVAL,
              "ark355_sr1cs_from_r1cs: the first matrix would hold more entries than ARK355_GR1CS_MAX_ROWS");
  s->P = P;
  s->U = U;
  // ---- the system -------------------------------------------------------------------------------------------------------
  Gr1csDev& g = s->sys;
  g.curve = Curve::ID;
  g.device = device;
  g.ell = 1 + P;
  g.w = U + n;
  g.m = g.ell + g.w;
  g.total = rows;
  g.preds.resize(1);
  Gr1csPred& Q = g.preds[0];
  Q.label = "SR1CS";                         // predicate/polynomial_constraint.rs: SR1CS_PREDICATE_LABEL
  Q.arity = 2;
  Q.rank = 0;
  Q.n = rows;
  Q.r1cs_shape = false;
  Q.degree = 2;
  Q.nnz = {nnz0, nnz1};
  Q.row_ptr.resize(2);
  Q.col.resize(2);
  Q.cidx.resize(2);
  Sr1csOut out;
  Gr1csMat mats[2];
  for (int k = 0; k < 2; k++) {
    Q.row_ptr[k].alloc((rows + 1) * 4);
    Q.col[k].alloc(Q.nnz[k] * 4);
    Q.cidx[k].alloc(Q.nnz[k] * 4);
    out.rp[k] = Q.row_ptr[k].as<uint32_t>();
    out.col[k] = Q.col[k].as<uint32_t>();
    out.ci[k] = Q.cidx[k].as<uint32_t>();
    mats[k] = Gr1csMat{out.rp[k], out.col[k], out.ci[k]};
  }
  ARK_LAUNCH(sr1cs_fill_kernel, dim3(sr1cs_grid(n + ell + 1)), dim3(256), 0, st, src, n, ell, (uint32_t)nnz_ab, (uint32_t)nnz_c,
             (uint32_t)c, (uint32_t)P, (const uint32_t*)s->F.as<uint32_t>(), (const uint32_t*)s->wit_col.as<uint32_t>(),
             (const uint32_t*)s->inst_col.as<uint32_t>(), out);
  ARK_CHECK_LAUNCH();
  g.pool_count = 3 * c;
  g.pool.alloc(g.pool_count * sizeof(Fr));
  ARK_LAUNCH((sr1cs_pool_kernel<Fr>), dim3(sr1cs_grid(c)), dim3(256), 0, st, (const Fr*)r.pool.as<Fr>(), (uint32_t)c, g.pool.as<Fr>());
  ARK_CHECK_LAUNCH();
  // x0^2 - x1: n_terms, then (coefficient, n_factors, (variable, exponent)..) per term; -1 is pool'[c]
  const uint32_t prog[9] = {2, 0, 1, 0, 2, (uint32_t)c, 1, 1, 1};
  Q.prog.alloc(sizeof(prog));
  ARK_CHECK_HIP(hipMemcpyAsync(Q.prog.p, prog, sizeof(prog), hipMemcpyHostToDevice, st));
  Q.mats.alloc(sizeof(mats));
  ARK_CHECK_HIP(hipMemcpyAsync(Q.mats.p, mats, sizeof(mats), hipMemcpyHostToDevice, st));
  // A and B for the assignment pass (their coefficient indices address the first block of pool')
  for (int k = 0; k < 2; k++) {
    s->rp[k].alloc((n + 1) * 4);
    s->col[k].alloc(r.nnz[k] * 4);
    s->ci[k].alloc(r.nnz[k] * 4);
    ARK_CHECK_HIP(hipMemcpyAsync(s->rp[k].p, r.row_ptr[k].p, (n + 1) * 4, hipMemcpyDeviceToDevice, st));
    if (r.nnz[k]) {
      ARK_CHECK_HIP(hipMemcpyAsync(s->col[k].p, r.col[k].p, r.nnz[k] * 4, hipMemcpyDeviceToDevice, st));
      ARK_CHECK_HIP(hipMemcpyAsync(s->ci[k].p, r.cidx[k].p, r.nnz[k] * 4, hipMemcpyDeviceToDevice, st));
    }
  }
  ARK_CHECK_HIP(hipStreamSynchronize(st));   // prog and mats leave this frame
  return s.release();
}

// z (device, ell + w) -> z' (device, ell' + w'); every slot of z' is written exactly once
template <class Curve>
static void sr1cs_assign_run(const Sr1csDev& s, const void* d_z, void* d_z_out, hipStream_t st) {
  using Fr = typename Curve::Fr;
  if (s.n) {
    const Gr1csMat A{s.rp[0].as<uint32_t>(), s.col[0].as<uint32_t>(), s.ci[0].as<uint32_t>()};
    const Gr1csMat B{s.rp[1].as<uint32_t>(), s.col[1].as<uint32_t>(), s.ci[1].as<uint32_t>()};
    ARK_LAUNCH((sr1cs_assign_kernel<Fr>), dim3(sr1cs_grid(s.n)), dim3(256), 0, st, A, B, (const Fr*)s.sys.pool.as<Fr>(), (const Fr*)d_z,
               s.n, (uint32_t)s.sys.ell, (const uint32_t*)s.F.as<uint32_t>(), (Fr*)d_z_out);
    ARK_CHECK_LAUNCH();
  }
  ARK_LAUNCH((sr1cs_scatter_kernel<Fr>), dim3(sr1cs_grid(s.m)), dim3(256), 0, st, (const Fr*)d_z, s.m, s.ell,
             (const uint32_t*)s.wit_col.as<uint32_t>(), (const uint32_t*)s.inst_col.as<uint32_t>(), (Fr*)d_z_out);
  ARK_CHECK_LAUNCH();
}

// z' from a host or a device assignment into host or device memory; zx / zo: grow-only scratch of the context
template <class Curve>
static void sr1cs_assignment(const Sr1csDev& s, const void* z, void* z_out, bool on_dev, DevBuf& zx, DevBuf& zo, hipStream_t st) {
  using Fr = typename Curve::Fr;
  ARK_REQUIRE(s.curve == Curve::ID, ARK355_EINVAL, "ark355_sr1cs_assignment: the handle belongs to another curve");
  if (on_dev) {
    sr1cs_assign_run<Curve>(s, z, z_out, st);
    ARK_CHECK_HIP(hipStreamSynchronize(st));
    return;
  }
  zx.ensure((s.m + 4) * sizeof(Fr));
  zo.ensure(s.sys.m * sizeof(Fr));
  ARK_CHECK_HIP(hipMemcpyAsync(zx.p, z, s.m * sizeof(Fr), hipMemcpyHostToDevice, st));
  sr1cs_assign_run<Curve>(s, zx.p, zo.p, st);
  ARK_CHECK_HIP(hipMemcpyAsync(z_out, zo.p, s.sys.m * sizeof(Fr), hipMemcpyDeviceToHost, st));
  ARK_CHECK_HIP(hipStreamSynchronize(st));
}

// per old column: col'(j) (0 for column 0, -1 unused) and the new input (k for p_k, -1 otherwise); either may be null
static inline void sr1cs_var_map(const Sr1csDev& s, int64_t* witness_col, int64_t* instance_col, hipStream_t st) {
  std::vector<uint32_t> h(s.m);
  auto widen = [&](const DevBuf& d, uint64_t count, int64_t* out) {
    if (!out) return;
    ARK_CHECK_HIP(hipMemcpyAsync(h.data(), d.p, count * 4, hipMemcpyDeviceToHost, st));
    ARK_CHECK_HIP(hipStreamSynchronize(st));
    for (uint64_t j = 0; j < count; j++) out[j] = h[j] == SR1CS_UNUSED ? -1 : (int64_t)h[j];
  };
  widen(s.wit_col, s.m, witness_col);
  widen(s.inst_col, s.ell, instance_col);
  if (instance_col)
    for (uint64_t j = s.ell; j < s.m; j++) instance_col[j] = -1;
}

// matrix `which` in the CSR convention of ark355_r1cs_load; tmp: grow-only scratch for the gathered coefficients
template <class Curve>
static void sr1cs_matrix(const Sr1csDev& s, int which, uint64_t* row_ptr, uint32_t* col, uint8_t* coeff, DevBuf& tmp, hipStream_t st) {
  ARK_REQUIRE(s.curve == Curve::ID, ARK355_EINVAL, "ark355_sr1cs_matrix: the handle belongs to another curve");
  gr1cs_matrix<Curve>(s.sys, s.sys.preds[0], (uint32_t)which, row_ptr, col, coeff, tmp, st);
}

}  // namespace ark355
