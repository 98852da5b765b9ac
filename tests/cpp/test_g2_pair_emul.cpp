// TEST INFRASTRUCTURE (CPU tier): the lane-pair Fq2 arithmetic of the G2 bucket accumulation (Pair28, msm28_impl.cuh) on an
// emulated lane pair.
//   1. Pair28::mul / sqr / mul2 and the "both components" forms they are built on (both_of / both_with / mulb / mul2b / sqr_x,
//      i.e. ark_pair_bcast0 / ark_pair_bcast1 / ark_pair_xchg) against the single-lane Fq2 reference, at every (KA, BETA) class
//      the library instantiates: random operands, 0, 1, -1, p - 1 and operands whose limbs and value sit at the top of the class.
//   2. madd28_g2z through long chains with the exceptional cases forced in (P + P, P - P, a base at infinity, the opening of an
//      empty accumulator, negated digits), with zz / zzz / x / y in registers (ZzRegs) and in LDS (ZzLds: the partner lane's
//      column is read directly), two lane pairs per block on different chains.
// Built with -DARK_EMUL: every 64-bit column and every lazy limb operation traps on overflow / wrap-around (field28.cuh).
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "msm_impl.cuh"

using namespace ark355;

#define CHECK(cond)                                                            \
  do {                                                                         \
    if (!(cond)) {                                                             \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
      exit(1);                                                                 \
    }                                                                          \
  } while (0)

struct Rng {
  uint64_t s;
  uint64_t next() {
    s += 0x9E3779B97F4A7C15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
};

// ---- operands ----------------------------------------------------------------------------------------------------------------
// An operand class is (K, BETA): value < (K - 1) p, every limb <= BETA (2^28 - 1) (the top limb carries what is left).
enum Kind { RANDOM = 0, ZERO, ONE, MINUS_ONE, P_MINUS_1, TOP, KINDS };

template <class F>
static F gen(Rng& rng, int kind, uint32_t K, uint32_t BETA) {
  constexpr int N = F::N;
  const uint32_t ptop = F::template kp<1>(N - 1);                 // (K - 1) ptop 2^(28 (N - 1)) <= (K - 1) p
  const uint32_t top_room = (K - 1) * ptop - BETA - 1;            // top limb below this: value < (K - 1) p whatever the low limbs
  F r = F::zero();
  switch (kind) {
    case ZERO:
      break;
    case ONE:
      r = F::from_fp(F::Base::one());
      break;
    case MINUS_ONE:
      r = F::from_fp(F::Base::neg(F::Base::one()));
      break;
    case P_MINUS_1:
      for (int i = 0; i < N; i++) r.l[i] = F::template kp<1>(i);
      r.l[0] -= 1;                                                 // p is odd
      break;
    case TOP:
      for (int i = 0; i < N - 1; i++) r.l[i] = BETA * F::MASK;
      r.l[N - 1] = top_room;
      break;
    default:
      for (int i = 0; i < N - 1; i++) r.l[i] = (uint32_t)(rng.next() % ((uint64_t)BETA * F::MASK + 1));
      r.l[N - 1] = (uint32_t)(rng.next() % (top_room + 1));
  }
  return r;
}

template <class Curve>
struct PairOps {
  using Fq = typename Curve::Fq;
  using Fq2 = typename Curve::Fq2;
  using P = typename Fq::Params;
  using F = Fp28<P>;
  using L = Pair28<P>;
  struct Cls {
    uint32_t K, BETA;
  };
  struct Case {
    F v[4][2];       // operand, component
  };

  // `apply` runs on both lanes of a pair with this lane's components; `ref` is the Fq2 value it must produce
  template <class Apply, class Ref>
  static void run(const char* what, int nargs, const Cls (&cls)[4], Apply apply, Ref ref) {
    Rng rng{0x9a17 + (uint64_t)nargs * 77 + cls[0].K * 1000 + cls[0].BETA};
    std::vector<Case> cases;
    auto push = [&](auto kind_of) {
      Case c;
      for (int a = 0; a < 4; a++)
        for (int h = 0; h < 2; h++) c.v[a][h] = a < nargs ? gen<F>(rng, kind_of(a, h), cls[a].K, cls[a].BETA) : F::zero();
      cases.push_back(c);
    };
    for (int k = 0; k < KINDS; k++) push([&](int, int) { return k; });                  // every operand the same edge
    for (int k = 0; k < KINDS; k++)
      for (int j = 0; j < KINDS; j++) push([&](int a, int h) { return (a + h) % 2 ? k : j; });
    for (int t = 0; t < 1500; t++) push([&](int, int) { return (int)(rng.next() % KINDS); });
    for (int t = 0; t < 1500; t++) push([&](int, int) { return (int)RANDOM; });
    std::vector<F> out(2 * cases.size());
    constexpr unsigned LANES = 4;                                                         // two pairs, alternate cases
    emu::launch(dim3(1), dim3(LANES), 0, [&]() {
      const uint32_t par = threadIdx.x & 1u, pair = threadIdx.x >> 1;
      for (size_t i = pair; i < cases.size(); i += LANES / 2) {
        const Case& c = cases[i];
        out[2 * i + par] = apply(c.v[0][par], c.v[1][par], c.v[2][par], c.v[3][par]);
      }
    });
    for (size_t i = 0; i < cases.size(); i++) {
      Fq2 v[4];
      for (int a = 0; a < 4; a++) v[a] = Fq2{F::to_fp(cases[i].v[a][0]), F::to_fp(cases[i].v[a][1])};
      const Fq2 want = ref(v[0], v[1], v[2], v[3]);
      const Fq2 got{F::to_fp(out[2 * i]), F::to_fp(out[2 * i + 1])};
      if (!(got == want)) {
        fprintf(stderr, "FAILED %s: case %zu\n", what, i);
        exit(1);
      }
      // results are products: normalised limbs
      for (int h = 0; h < 2; h++)
        for (int k = 0; k < F::N - 1; k++) CHECK(out[2 * i + h].l[k] <= F::MASK);
    }
  }

  // a (K, BETA) first factor against a normalised second factor of value < KB p
  template <uint32_t KA, uint32_t BETA, uint32_t KB>
  static void mul_class() {
    const Cls cls[4] = {{KA, BETA}, {KB + 1, 1}, {2, 1}, {2, 1}};
    auto ref = [](const Fq2& a, const Fq2& b, const Fq2&, const Fq2&) { return Fq2::mul(a, b); };
    run("mul", 2, cls, [](const F& a, const F& b, const F&, const F&) { return L::template mul<KA, BETA>(a, b); }, ref);
    run("mulb(both_of)", 2, cls,
        [](const F& a, const F& b, const F&, const F&) { return L::mulb(L::template both_of<KA, BETA>(a), b, L::xchg(b)); }, ref);
    run("mulb(both_with)", 2, cls,
        [](const F& a, const F& b, const F&, const F&) {
          return L::mulb(L::template both_with<KA, BETA>(a, L::xchg(a)), b, L::xchg(b));
        },
        ref);
  }
  template <uint32_t KA>
  static void sqr_class() {
    const Cls cls[4] = {{KA, 1}, {2, 1}, {2, 1}, {2, 1}};
    auto ref = [](const Fq2& a, const Fq2&, const Fq2&, const Fq2&) { return Fq2::sqr(a); };
    run("sqr", 1, cls, [](const F& a, const F&, const F&, const F&) { return L::template sqr<KA>(a); }, ref);
    run("sqr_x", 1, cls, [](const F& a, const F&, const F&, const F&) { return L::template sqr_x<KA>(a, L::xchg(a)); }, ref);
  }
  // a b + c d: a (KA, BA) against b normalised < KB p, c (KC, BC) against d normalised < KD p
  template <uint32_t KA, uint32_t BA, uint32_t KB, uint32_t KC, uint32_t BC, uint32_t KD>
  static void mul2_class() {
    const Cls cls[4] = {{KA, BA}, {KB + 1, 1}, {KC, BC}, {KD + 1, 1}};
    auto ref = [](const Fq2& a, const Fq2& b, const Fq2& c, const Fq2& d) { return Fq2::add(Fq2::mul(a, b), Fq2::mul(c, d)); };
    run("mul2", 4, cls, [](const F& a, const F& b, const F& c, const F& d) { return L::template mul2<KA, BA, KC, BC>(a, b, c, d); },
        ref);
  }
  // the fused Y3 pass as the mixed addition issues it: R (6, 1) against T, PPP (2, 1) against NY = 3p - Y1 (limbs <= 2 (2^28 - 1))
  static void y3_class() {
    const Cls cls[4] = {{6, 1}, {10, 1}, {2, 1}, {4, 2}};
    auto ref = [](const Fq2& a, const Fq2& b, const Fq2& c, const Fq2& d) { return Fq2::add(Fq2::mul(a, b), Fq2::mul(c, d)); };
    run("mul2b", 4, cls,
        [](const F& a, const F& b, const F& c, const F& d) {
          return L::mul2b(L::template both_with<6, 1>(a, L::xchg(a)), b, L::xchg(b), L::template both_of<2, 1>(c), d, L::xchg(d));
        },
        ref);
  }

  static void all(const char* name) {
    // the broadcasts themselves
    {
      std::vector<uint32_t> got(3 * 8);
      emu::launch(dim3(1), dim3(8), 0, [&]() {
        const uint32_t v = 100u + threadIdx.x;
        got[3 * threadIdx.x + 0] = ark_pair_bcast0(v);
        got[3 * threadIdx.x + 1] = ark_pair_bcast1(v);
        got[3 * threadIdx.x + 2] = ark_pair_xchg(v);
      });
      for (uint32_t t = 0; t < 8; t++) {
        CHECK(got[3 * t + 0] == 100u + (t & ~1u));
        CHECK(got[3 * t + 1] == 100u + (t | 1u));
        CHECK(got[3 * t + 2] == 100u + (t ^ 1u));
      }
    }
    // every class the mixed addition, the doubling and the tail additions instantiate
    mul_class<2, 1, 2>();        // px zz, PP against zz / zzz / Pd / x (second factor up to 10 p below)
    mul_class<2, 1, 10>();
    mul_class<3, 3, 2>();        // py' zzz
    mul_class<3, 1, 2>();
    mul_class<6, 1, 2>();
    mul_class<8, 1, 2>();
    mul_class<11, 1, 2>();
    sqr_class<3>();
    sqr_class<5>();
    sqr_class<6>();
    sqr_class<11>();
    mul2_class<6, 1, 9, 4, 3, 2>();
    mul2_class<5, 1, 9, 4, 3, 2>();
    y3_class();
    printf("%s Pair28 mul / sqr / mul2 == Fq2: ok\n", name);
  }
};

// ---- madd28_g2z chains -------------------------------------------------------------------------------------------------------
template <class Curve, bool LDS>
static void run_chain(const char* name) {
  using Fq = typename Curve::Fq;
  using Fq2 = typename Curve::Fq2;
  using P = typename Fq::Params;
  using F28 = Fp28<P>;
  using Consts = typename Curve::Consts;
  using Zt = typename std::conditional<LDS, ZzLds<P>, ZzRegs<P>>::type;
  Rng rng{LDS ? 0x1d5u : 0x4e6u};
  Affine<Fq2> g;
  for (int i = 0; i < Fq::N; i++) {
    g.x.c0.l[i] = Consts::g2_gen_x0(i);
    g.x.c1.l[i] = Consts::g2_gen_x1(i);
    g.y.c0.l[i] = Consts::g2_gen_y0(i);
    g.y.c1.l[i] = Consts::g2_gen_y1(i);
  }
  const size_t NP = 12;
  std::vector<Affine<Fq2>> pts;
  for (size_t i = 0; i < NP; i++) {
    uint32_t k[2] = {(uint32_t)rng.next() | 1u, (uint32_t)rng.next()};
    pts.push_back(xyzz_to_affine(xyzz_mul_scalar(XYZZ<Fq2>::from_affine(g), k, 2)));
  }
  // the chains are generated up front (both lanes of a pair must see the same steps); one chain per pair
  constexpr unsigned PAIRS = 2;
  const size_t LEN = 2500;
  std::vector<Affine<Fq2>> chain_p[PAIRS];
  std::vector<char> chain_neg[PAIRS];
  std::vector<XYZZ<Fq2>> ref_after[PAIRS];
  size_t forced[PAIRS][4] = {};
  for (unsigned q = 0; q < PAIRS; q++) {
    XYZZ<Fq2> ref = XYZZ<Fq2>::inf();
    for (size_t s = 0; s < LEN; s++) {
      bool ng = rng.next() & 1;                                     // a negated digit
      const uint32_t kind = rng.next() % 32;
      Affine<Fq2> p = pts[rng.next() % NP];
      if (kind == 0 && !ref.is_inf()) {                             // P + P
        p = xyzz_to_affine(ref);
        ng = false;
        forced[q][0]++;
      } else if (kind == 1 && !ref.is_inf()) {                      // P - P: the next step opens an empty accumulator
        p = xyzz_to_affine(ref);
        ng = true;
        forced[q][1]++;
      } else if (kind == 2) {                                       // a base at infinity
        p = Affine<Fq2>::inf();
        forced[q][2]++;
      }
      if (ref.is_inf() && !p.is_inf()) forced[q][3]++;
      chain_p[q].push_back(p);
      chain_neg[q].push_back(ng);
      if (!p.is_inf()) {
        Affine<Fq2> a = p;
        if (ng) a.y = Fq2::neg(a.y);
        xyzz_madd_ni(ref, a);
      }
      ref_after[q].push_back(ref);
    }
    for (int k = 0; k < 4; k++) CHECK(forced[q][k] >= 20);
  }
  std::vector<XYZZ<Fq2>> got_after[PAIRS];
  std::vector<char> got_empty[PAIRS];
  for (unsigned q = 0; q < PAIRS; q++) {
    got_after[q].resize(LEN);
    got_empty[q].resize(LEN);
  }
  const unsigned threads = 2 * PAIRS;
  emu::launch(dim3(1), dim3(threads), LDS ? ZzLds<P>::bytes(threads) : 0, [&]() {
    const uint32_t par = threadIdx.x & 1u, q = threadIdx.x >> 1;
    Acc28<P> acc;
    acc.x = acc.y = acc.zz = acc.zzz = F28::zero();
    ARK_DYN_SMEM(uint4, zlds);
    const Zt z = [&]() {
      if constexpr (LDS) return ZzLds<P>{acc, ZzLds<P>::column(zlds)};
      else return ZzRegs<P>{acc};
    }();
    bool empty = true;
    for (size_t s = 0; s < LEN; s++) {
      const Affine<Fq2>& p = chain_p[q][s];
      F28 px = F28::zero(), py = F28::zero();                       // a table row at infinity is all zero
      if (!p.is_inf()) {
        px = F28::from_fp(par ? p.x.c1 : p.x.c0);
        py = F28::from_fp(par ? p.y.c1 : p.y.c0);
      }
      uint32_t any = 0;
      for (int k = 0; k < F28::N; k++) any |= px.l[k] | py.l[k];
      if ((any | ark_pair_xchg(any)) != 0) madd28_g2z<P, Zt>(acc, z, empty, px, py, chain_neg[q][s] != 0);   // (as the kernels do)
      if (par == 0) got_empty[q][s] = empty;
      Fq* d = reinterpret_cast<Fq*>(&got_after[q][s]);
      if (!empty) {
        d[0 + par] = F28::to_fp(z.x());
        d[2 + par] = F28::to_fp(z.y());
        d[4 + par] = F28::to_fp(z.zz());
        d[6 + par] = F28::to_fp(z.zzz());
      }
    }
  });
  for (unsigned q = 0; q < PAIRS; q++)
    for (size_t s = 0; s < LEN; s++) {
      CHECK((got_empty[q][s] != 0) == ref_after[q][s].is_inf());
      if (!ref_after[q][s].is_inf() && ((s % 11) == 0 || s + 1 == LEN)) {
        const Affine<Fq2> a = xyzz_to_affine(got_after[q][s]), b = xyzz_to_affine(ref_after[q][s]);
        CHECK(a.x == b.x && a.y == b.y);
      }
    }
  printf("%s madd28_g2z chains (%s): ok\n", name, LDS ? "ZzLds" : "ZzRegs");
}

int main() {
  PairOps<BlsCurve>::all("bls12_381");
  PairOps<BnCurve>::all("bn254");
  run_chain<BlsCurve, false>("bls12_381");
  run_chain<BlsCurve, true>("bls12_381");
  run_chain<BnCurve, false>("bn254");
  run_chain<BnCurve, true>("bn254");
  printf("g2 pair: all cases agree with the single-lane Fq2 formulas\n");
  return 0;
}
