// finalize() on the device against the route a host has without it, on the same systems and the same box:
//   (dev)   ark355_gr1cs_from_lcs from the host's flat arrays: upload, inlining, CSR and handle construction
//   (host)  the C++ mirror's inline_all_lcs + to_matrices (host_mirror/relations.hpp, one thread), the rows flattened to CSR, then
//           ark355_gr1cs_load
// Both read one constraint system, generated once; the host route works on a copy made outside the clock.  The readings are
// interleaved (dev, host, dev, ...) after a warm-up; median, minimum and max - min over the repeats, host clock.
// Circuits: "bench" -- relations/examples/bench.rs:22-83 (unit coefficients, an extra symbolic LC on every other row: depth 1);
// "deep" -- chains of 32 running sums s_k = s_{k-1} + w, one new_lc and one row per step, the shape field-gadget additions
// produce (depth 31, rows of 2 .. 33 entries once compacted).
//   g++ -O2 -std=c++17 tools/lcmap_host_route.cpp -o tools/lcmap_host_route.bin -Lsnark_amd -lark355 -Wl,-rpath,$PWD/snark_amd
//   tools/lcmap_host_route.bin <bls12_381|bn254> <bench|deep> <log_n> <reps> <warmup>        (tools/lcmap_bench.py drives it)
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../host_mirror/snark.hpp"

using namespace ark_relations;
using namespace ark_relations::gr1cs;

struct SplitMix64 {
  uint64_t s;
  explicit SplitMix64(uint64_t seed) : s(seed) {}
  uint64_t next() {
    s += 0x9E3779B97F4A7C15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
};

template <class F>
static void bench_rs_circuit(ConstraintSystemRef<F> cs, size_t n) {
  using L = LinearCombination<F>;
  const F a = F::from_u64(0x1234567);
  std::vector<Variable> vars;
  for (int i = 0; i < 3; i++) vars.push_back(cs.new_witness_variable([&] { return a; }));
  vars.reserve(3 * n + 3);
  SplitMix64 ra(0), rb(1), rc(2);
  for (size_t i = 0; i < n; i++) {
    const size_t cur = vars.size() < 10 ? vars.size() : 10, lower = vars.size() - cur;
    const size_t ka = 1 + ra.next() % 10, kb = 1 + rb.next() % 10;
    auto pick = [&](SplitMix64& r, size_t k) {
      L lc;
      for (size_t j = 0; j < k; j++) lc.terms.emplace_back(F::one(), vars[lower + r.next() % cur]);   // LinearCombination(vec): as drawn
      return lc;
    };
    const Variable ci = vars[lower + rc.next() % cur];
    if (i % 2 == 0) {
      const Variable extra = cs.new_lc([&] { return pick(rc, ka); });
      cs.enforce_r1cs_constraint([&] { return pick(ra, ka) + extra; }, [&] { return pick(rb, kb); }, [&] { return L() + ci; });
    } else {
      cs.enforce_r1cs_constraint([&] { return pick(ra, ka); }, [&] { return pick(rb, kb); }, [&] { return L() + ci; });
    }
    for (int j = 0; j < 3; j++) vars.push_back(cs.new_witness_variable([&] { return a; }));
  }
}

template <class F>
static void deep_chain_circuit(ConstraintSystemRef<F> cs, size_t n) {
  using L = LinearCombination<F>;
  const F a = F::from_u64(0x7654321);
  Variable sum = Variable::Zero();
  for (size_t i = 0; i < n; i++) {
    const Variable x = cs.new_witness_variable([&] { return a; }), y = cs.new_witness_variable([&] { return a; });
    if (i % 32 == 0) sum = cs.new_lc([&] { return L() + x + y; });
    else sum = cs.new_lc([&] { return L() + sum + x; });
    cs.enforce_r1cs_constraint([&] { return L() + sum; }, [&] { return L() + y; }, [&] { return L() + x; });
  }
}

static double ms(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
  return std::chrono::duration<double, std::milli>(b - a).count();
}

struct Series {
  std::vector<double> v;
  void report(const char* label) const {
    std::vector<double> s = v;
    std::sort(s.begin(), s.end());
    const double med = s.size() % 2 ? s[s.size() / 2] : 0.5 * (s[s.size() / 2 - 1] + s[s.size() / 2]);
    printf("  %-58s median %9.3f  min %9.3f  max-min %8.3f\n", label, med, s.front(), s.back() - s.front());
  }
  double median() const {
    std::vector<double> s = v;
    std::sort(s.begin(), s.end());
    return s.size() % 2 ? s[s.size() / 2] : 0.5 * (s[s.size() / 2 - 1] + s[s.size() / 2]);
  }
};

template <class Tag>
static int run(const std::string& curve, const std::string& circuit, size_t n, int reps, int warmup) {
  using F = ark_snark::Field<typename Tag::FrP>;
  auto ref = ConstraintSystemRef<F>::new_ref();
  ref.set_mode(SynthesisMode::prove(true, false));
  auto g0 = std::chrono::steady_clock::now();
  if (circuit == "deep") deep_chain_circuit<F>(ref, n);
  else bench_rs_circuit<F>(ref, n);
  const double generate_ms = ms(g0, std::chrono::steady_clock::now());
  const ConstraintSystem<F>& master = ref.borrow();
  // ---- the flat arrays, as the reference holds them ----------------------------------------------------------------------
  const LcMap<F>& map = master.lcs();
  const size_t n_lcs = map.num_lcs(), T = map.total_lc_size();
  std::vector<uint64_t> offsets(n_lcs + 1), vars(T);
  std::vector<uint32_t> coeffs(T);
  for (size_t k = 0; k < n_lcs; k++) offsets[k + 1] = map.end(k);
  size_t references = 0;
  for (size_t e = 0; e < T; e++) {
    const Variable v = map.var(e);
    vars[e] = (uint64_t)v.kind() << Variable::TAG_SHIFT | v.payload();
    coeffs[e] = map.coeff(e);
    references += v.is_lc();
  }
  std::vector<F> pool(master.interner().len());
  for (size_t i = 0; i < pool.size(); i++) pool[i] = master.interner().value((uint32_t)i);
  std::vector<uint64_t> args[3];
  const uint64_t* arg_ptr[3];
  for (int k = 0; k < 3; k++) {
    for (const Variable& v : master.r1cs_arguments()[k]) args[k].push_back((uint64_t)v.kind() << Variable::TAG_SHIFT | v.payload());
    arg_ptr[k] = args[k].data();
  }
  const F poly_coeff[2] = {F::one(), -F::one()};
  const uint32_t term_ptr[3] = {0, 2, 3}, term_var[3] = {0, 1, 2}, term_exp[3] = {1, 1, 1};
  ark355_lc_system_desc sys{};
  sys.num_instance = master.num_instance_variables;
  sys.num_witness = master.num_witness_variables;
  sys.n_lcs = n_lcs;
  sys.lc_offsets = offsets.data();
  sys.lc_vars = vars.data();
  sys.lc_coeffs = coeffs.data();
  sys.n_pool = pool.size();
  sys.pool = reinterpret_cast<const uint8_t*>(pool.data());
  ark355_predicate_lcs_desc pl{};
  pl.label = "R1CS";
  pl.arity = 3;
  pl.n_constraints = master.num_constraints();
  pl.n_terms = 2;
  pl.term_coeff = reinterpret_cast<const uint8_t*>(poly_coeff);
  pl.term_ptr = term_ptr;
  pl.term_var = term_var;
  pl.term_exp = term_exp;
  pl.args = arg_ptr;

  ark355_ctx* ctx = nullptr;
  if (ark355_ctx_create(0, &ctx) != ARK355_OK) {
    fprintf(stderr, "no device\n");
    return 2;
  }
  auto must = [&](int32_t rc, const char* what) {
    if (rc != ARK355_OK) {
      fprintf(stderr, "%s failed (%d): %s\n", what, rc, ark355_last_error(ctx));
      exit(3);
    }
  };
  Series dev, host_total, host_inline, host_matrices, host_flatten, host_load;
  uint64_t dev_nnz[3] = {0, 0, 0}, host_nnz[3] = {0, 0, 0};
  for (int it = 0; it < warmup + reps; it++) {
    // ---- (dev) -----------------------------------------------------------------------------------------------------------
    ark355_gr1cs* g = nullptr;
    auto t0 = std::chrono::steady_clock::now();
    must(ark355_gr1cs_from_lcs(ctx, Tag::ID, &sys, &pl, 1, &g), "ark355_gr1cs_from_lcs");
    auto t1 = std::chrono::steady_clock::now();
    must(ark355_gr1cs_pred_dims(g, 0, nullptr, nullptr, dev_nnz), "ark355_gr1cs_pred_dims");
    ark355_gr1cs_free(g);
    // ---- (host) ------------------------------------------------------------------------------------------------------------
    ConstraintSystem<F> cs = master;                                    // outside the clock
    auto h0 = std::chrono::steady_clock::now();
    cs.finalize();
    auto h1 = std::chrono::steady_clock::now();
    const auto all = cs.to_matrices();
    const auto& m = all.at("R1CS");
    auto h2 = std::chrono::steady_clock::now();
    std::vector<uint64_t> rp[3];
    std::vector<uint32_t> col[3];
    std::vector<F> cf[3];
    const uint64_t* rp_ptr[3];
    const uint32_t* col_ptr[3];
    const uint8_t* cf_ptr[3];
    for (int k = 0; k < 3; k++) {
      rp[k].reserve(m[k].size() + 1);
      rp[k].push_back(0);
      for (const auto& row : m[k]) {
        for (const auto& cj : row) {
          cf[k].push_back(cj.first);
          col[k].push_back((uint32_t)cj.second);
        }
        rp[k].push_back(col[k].size());
      }
      host_nnz[k] = col[k].size();
      rp_ptr[k] = rp[k].data();
      col_ptr[k] = col[k].data();
      cf_ptr[k] = reinterpret_cast<const uint8_t*>(cf[k].data());
    }
    auto h3 = std::chrono::steady_clock::now();
    ark355_predicate_desc pd{};
    pd.label = "R1CS";
    pd.arity = 3;
    pd.n_constraints = cs.num_constraints();
    pd.n_terms = 2;
    pd.term_coeff = pl.term_coeff;
    pd.term_ptr = term_ptr;
    pd.term_var = term_var;
    pd.term_exp = term_exp;
    pd.row_ptr = rp_ptr;
    pd.col = col_ptr;
    pd.coeff = cf_ptr;
    ark355_gr1cs* gl = nullptr;
    must(ark355_gr1cs_load(ctx, Tag::ID, cs.num_instance_variables, cs.num_witness_variables, &pd, 1, &gl), "ark355_gr1cs_load");
    auto h4 = std::chrono::steady_clock::now();
    ark355_gr1cs_free(gl);
    if (it < warmup) continue;
    dev.v.push_back(ms(t0, t1));
    host_inline.v.push_back(ms(h0, h1));
    host_matrices.v.push_back(ms(h1, h2));
    host_flatten.v.push_back(ms(h2, h3));
    host_load.v.push_back(ms(h3, h4));
    host_total.v.push_back(ms(h0, h4));
  }
  printf("%s %s: %zu rows, %zu + %zu variables, %zu LCs, %zu entries, %zu LC references; generate_constraints %.1f ms (not compared)\n",
         curve.c_str(), circuit.c_str(), (size_t)master.num_constraints(), (size_t)master.num_instance_variables,
         (size_t)master.num_witness_variables, n_lcs, T, references, generate_ms);
  printf("  non-zeros of A, B, C: device (canonical rows) %llu %llu %llu, host %llu %llu %llu\n", (unsigned long long)dev_nnz[0],
         (unsigned long long)dev_nnz[1], (unsigned long long)dev_nnz[2], (unsigned long long)host_nnz[0],
         (unsigned long long)host_nnz[1], (unsigned long long)host_nnz[2]);
  dev.report("(dev)  ark355_gr1cs_from_lcs");
  host_total.report("(host) inline_all_lcs + to_matrices + CSR + ark355_gr1cs_load");
  host_inline.report("         inline_all_lcs");
  host_matrices.report("         to_matrices");
  host_flatten.report("         rows -> CSR arrays");
  host_load.report("         ark355_gr1cs_load");
  printf("  host route / device entry = %.2f\n", host_total.median() / dev.median());
  ark355_ctx_destroy(ctx);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 6) {
    fprintf(stderr, "usage: %s <bls12_381|bn254> <bench|deep> <log_n> <reps> <warmup>\n", argv[0]);
    return 1;
  }
  const std::string curve = argv[1], circuit = argv[2];
  const size_t n = (size_t)1 << atoi(argv[3]);
  const int reps = atoi(argv[4]), warmup = atoi(argv[5]);
  if (curve == "bn254") return run<ark_snark::BnCurveTag>(curve, circuit, n, reps, warmup);
  return run<ark_snark::BlsCurveTag>(curve, circuit, n, reps, warmup);
}
