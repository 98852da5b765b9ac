// Device pairing: multi-Miller loop, elementwise G1 scalar multiplication and the on-curve check of batch verification.
//
// One Miller loop is a sequential chain of tower-field arithmetic; a BATCH of n loops is n independent chains, one lane each.
// The work is split the way ark-ec splits it (G2Prepared / multi_miller_loop):
//
//   pass A  pairing_lines_kernel       one lane per pair walks T = [k]Q on the twist in homogeneous projective coordinates
//                                      (no inversion: doubling and mixed addition of Costello-Lange-Naehrig as ark-ec has
//                                      them), evaluates each line at P and writes its three F_q2 coefficients to HBM.
//   pass B  pairing_accumulate_kernel  one lane per pair squares f and multiplies it by the sparse lines.  f does not fit a
//                                      lane's registers (144 dwords for BLS12-381), so every lane keeps f and one product
//                                      buffer in LDS (2 x 576 B x 64 lanes = 72 KiB per workgroup, two workgroups per CU) and
//                                      the register-level unit is ONE F_q2 product whose operands are read from LDS by a
//                                      run-time coefficient index: the loops over coefficients stay rolled, so the kernel
//                                      holds a handful of inlined F_q2 multiplications instead of ~40 and nothing spills.
//                                      The workgroup then multiplies its 64 values with a product tree in LDS.
//   pass C  pairing_product_kernel     one workgroup multiplies the per-workgroup partial products (second launch).
//
//   per group (ark355_pairing_groups, ark355_verify_each): pass B leaves every pair's f in HBM instead of the workgroup
//   product, and  pairing_final_exp_kernel  multiplies the Miller values of a group and raises the product to
//   (q^12 - 1) / r, one lane per group; see "final exponentiation" below.
//
// F_q12 is held as F_q2[w] / (w^6 - xi), six F_q2 coefficients c_k of w^k.  That is the tower of pairing_host.hpp read
// differently (v = w^2: c0.c0, c1.c0, c0.c1, c1.c1, c0.c2, c1.c2 are the coefficients of w^0 .. w^5), and it makes every
// product one double loop: out_k = sum_{i+j=k} a_i b_j + xi sum_{i+j=k+6} a_i b_j.  A line has three non-zero coefficients,
// at w^0, w^2, w^3 (BLS12-381, M-type twist) or w^0, w^1, w^3 (BN254, D-type twist), as in pairing_host.hpp.  The lines
// differ from the host's affine ones by a factor in F_q2, which the final exponentiation removes.
//
// Memory layout: everything a lane touches repeatedly is stored dword-transposed, element [dword][lane], so that the 64
// lanes of a wave read 64 consecutive dwords (one 256 B line of HBM, 64 distinct banks of LDS).
#pragma once
#include "common.h"
#include "wire_impl.cuh"

namespace ark355 {

constexpr uint32_t PAIR_LANES = 64;          // lanes per workgroup of the Miller-loop kernels (one wave)

template <class Curve>
struct PairingDev {
  using Fq = typename Curve::Fq;
  using Fq2 = typename Curve::Fq2;
  using Fr = typename Curve::Fr;
  using W = Wire<Curve>;
  static constexpr bool BN = Curve::ID == ARK355_BN254;
  static constexpr uint32_t W2 = 2 * Fq::N;              // dwords of one F_q2
  static constexpr uint32_t W12 = 6 * W2;                // dwords of one F_q12
  // loop count: |x| (BLS12-381) or 6x + 2 = 2^64 + LOOP_LO (BN254); most significant bit first, top bit skipped
  static constexpr uint64_t LOOP_LO = BN ? 0x9D797039BE763BA8ull : 0xd201000000010000ull;
  static constexpr int LOOP_TOP = BN ? 64 : 63;
  // w-powers of the second and third line coefficient (the first sits at w^0)
  static constexpr int LP1 = BN ? 1 : 2, LP2 = 3;

  struct Consts {
    Fq two_inv;               // 1/2
    Fq2 frob_x, frob_y;       // BN254: xi^((q-1)/3), xi^((q-1)/2)
    uint64_t sqr_mask[2];     // bit s: line s belongs to a doubling step (f is squared before it is multiplied in)
    uint32_t steps;           // lines per pair
  };

  // the schedule both passes follow, one bit per line
  static void schedule(Consts* k) {
    uint32_t s = 0;
    k->sqr_mask[0] = k->sqr_mask[1] = 0;
    for (int i = LOOP_TOP - 1; i >= 0; i--) {
      k->sqr_mask[s >> 6] |= 1ull << (s & 63);
      s++;
      if ((LOOP_LO >> i) & 1ull) s++;
    }
    if (BN) s += 2;
    k->steps = s;
  }

  ARK_HD static Fq2 mul_fq(const Fq2& a, const Fq& k) { return Fq2{Fq::mul(a.c0, k), Fq::mul(a.c1, k)}; }
  ARK_HD static Fq2 mul_xi(const Fq2& a) {
    if (BN) {
      const Fq a0_8 = Fq::dbl(Fq::dbl(Fq::dbl(a.c0))), a1_8 = Fq::dbl(Fq::dbl(Fq::dbl(a.c1)));
      return Fq2{Fq::sub(Fq::add(a0_8, a.c0), a.c1), Fq::add(Fq::add(a1_8, a.c1), a.c0)};
    }
    return Fq2{Fq::sub(a.c0, a.c1), Fq::add(a.c0, a.c1)};
  }

  // ---- dword-transposed F_q2: dword d of the element at p[d * st] ---------------------------------------------------
  ARK_D static Fq2 ld(const uint32_t* p, size_t st) {
    Fq2 r;
#pragma unroll
    for (int i = 0; i < Fq::N; i++) {
      r.c0.l[i] = p[(size_t)i * st];
      r.c1.l[i] = p[(size_t)(Fq::N + i) * st];
    }
    return r;
  }
  ARK_D static void st(uint32_t* p, size_t stride, const Fq2& v) {
#pragma unroll
    for (int i = 0; i < Fq::N; i++) {
      p[(size_t)i * stride] = v.c0.l[i];
      p[(size_t)(Fq::N + i) * stride] = v.c1.l[i];
    }
  }

  // ---- F_q12 in a lane's LDS column: coefficient k at f + k * W2 * PAIR_LANES, dword stride PAIR_LANES ----------------
  static constexpr uint32_t CK = W2 * PAIR_LANES;
  ARK_D static Fq2 ldc(const uint32_t* f, int k) { return ld(f + (uint32_t)k * CK, PAIR_LANES); }
  ARK_D static void stc(uint32_t* f, int k, const Fq2& v) { st(f + (uint32_t)k * CK, PAIR_LANES, v); }
  ARK_D static void set_one(uint32_t* f) {
    stc(f, 0, Fq2::one());
    for (int k = 1; k < 6; k++) stc(f, k, Fq2::zero());
  }
  ARK_D static void copy12(uint32_t* o, const uint32_t* a) {
    for (uint32_t d = 0; d < W12; d++) o[d * PAIR_LANES] = a[d * PAIR_LANES];
  }

  // o = a^2 (o and a distinct): 21 products, one multiplication site
  ARK_D static void sqr12(uint32_t* o, const uint32_t* a) {
#pragma unroll 1
    for (int k = 0; k < 6; k++) {
      Fq2 lo = Fq2::zero(), hi = Fq2::zero();
#pragma unroll 1
      for (int i = 0; i < 6; i++) {
        int j = k - i;
        const bool wrap = j < 0;
        if (wrap) j += 6;
        if (i > j) continue;
        Fq2 p = Fq2::mul(ldc(a, i), ldc(a, j));
        if (i < j) p = Fq2::dbl(p);
        if (wrap) hi = Fq2::add(hi, p);
        else lo = Fq2::add(lo, p);
      }
      stc(o, k, Fq2::add(lo, mul_xi(hi)));
    }
  }

  // o = a * b (o distinct from both); b is any dword-transposed F_q12: coefficient stride cb, dword stride sb
  ARK_D static void mul12(uint32_t* o, const uint32_t* a, const uint32_t* b, size_t cb, size_t sb) {
#pragma unroll 1
    for (int k = 0; k < 6; k++) {
      Fq2 lo = Fq2::zero(), hi = Fq2::zero();
#pragma unroll 1
      for (int i = 0; i < 6; i++) {
        int j = k - i;
        const bool wrap = j < 0;
        if (wrap) j += 6;
        const Fq2 p = Fq2::mul(ldc(a, i), ld(b + (size_t)j * cb, sb));
        if (wrap) hi = Fq2::add(hi, p);
        else lo = Fq2::add(lo, p);
      }
      stc(o, k, Fq2::add(lo, mul_xi(hi)));
    }
  }

  // o = a * (l0 + l1 w^LP1 + l2 w^LP2): 18 products
  ARK_D static void mul12_sparse(uint32_t* o, const uint32_t* a, const Fq2& l0, const Fq2& l1, const Fq2& l2) {
#pragma unroll 1
    for (int k = 0; k < 6; k++) {
      Fq2 lo = Fq2::mul(l0, ldc(a, k)), hi = Fq2::zero();
      {
        int j = k - LP1;
        const bool wrap = j < 0;
        if (wrap) j += 6;
        const Fq2 p = Fq2::mul(l1, ldc(a, j));
        if (wrap) hi = p;
        else lo = Fq2::add(lo, p);
      }
      {
        int j = k - LP2;
        const bool wrap = j < 0;
        if (wrap) j += 6;
        const Fq2 p = Fq2::mul(l2, ldc(a, j));
        if (wrap) hi = Fq2::add(hi, p);
        else lo = Fq2::add(lo, p);
      }
      stc(o, k, Fq2::add(lo, mul_xi(hi)));
    }
  }

  // product of the workgroup's 64 values (each lane's at f, scratch at g) -> lane 0's f
  ARK_D static void block_product(uint32_t* f, uint32_t* g, uint32_t lane) {
#pragma unroll 1
    for (uint32_t s = PAIR_LANES / 2; s >= 1; s >>= 1) {
      __syncthreads();
      if (lane < s) mul12(g, f, f + s, CK, PAIR_LANES);
      __syncthreads();
      if (lane < s) copy12(f, g);
    }
  }

  // ---- final exponentiation: one lane per GT value ------------------------------------------------------------------
  // The lane keeps FE_BUFS values of F_q12 in LDS and follows a PROGRAM of three-address instructions over them, formed once
  // on the host (FeProgram below) and read from HBM by the whole wave at once.  The kernel so holds ONE squaring and ONE
  // multiplication site, like pass B, however long the exponent chain is.  36 KiB (BLS12-381) / 24 KiB (BN254) per
  // buffer and workgroup: 4 / 6 buffers are 144 KiB of the 160 KiB a workgroup may declare, one wave per CU.
  static constexpr uint32_t FE_BUFS = BN ? 6 : 4;
  static constexpr uint32_t B12 = W12 * PAIR_LANES;       // dwords of one buffer of a workgroup
  // instruction word: op | d << 4 | a << 8 | b << 12
  enum FeOp : uint32_t {
    FE_SQR = 0,     // d = a^2
    FE_MUL = 1,     // d = a * b
    FE_COPY = 2,    // d = a
    FE_CONJ = 3,    // d = conj(d)  (w -> -w; the inverse once the easy part is done)
    FE_FROB = 4,    // d = d^(q^a), a = 1 .. 3
    FE_INV6 = 5     // d in F_q6 (odd coefficients zero) -> 1 / d
  };
  static constexpr uint32_t fe_ins(uint32_t op, uint32_t d, uint32_t a = 0, uint32_t b = 0) {
    return op | d << 4 | a << 8 | b << 12;
  }

  // The program pairing_final_exp_kernel follows, built on the host (host code: never called from a kernel).  Buffer 0 holds
  // f on entry and f^((q^12 - 1) / r) on exit; the buffers in between are handed out here, so that the kernel needs no more than FE_BUFS.
  struct FeProgram {
    std::vector<uint32_t> code;
    uint32_t free_mask = (1u << FE_BUFS) - 1u;
    uint32_t take() {
      for (uint32_t b = 0; b < FE_BUFS; b++)
        if ((free_mask >> b) & 1u) {
          free_mask &= ~(1u << b);
          return b;
        }
      throw HipError{ARK355_EINVAL, "final exponentiation program: out of buffers"};
    }
    void drop(uint32_t b) { free_mask |= 1u << b; }
    void drop(uint32_t a, uint32_t b) { drop(a), drop(b); }
    uint32_t sqr(uint32_t a) {
      const uint32_t d = take();
      code.push_back(fe_ins(FE_SQR, d, a));
      return d;
    }
    uint32_t mul(uint32_t a, uint32_t b) {
      const uint32_t d = take();
      code.push_back(fe_ins(FE_MUL, d, a, b));
      return d;
    }
    uint32_t copy(uint32_t a) {
      const uint32_t d = take();
      code.push_back(fe_ins(FE_COPY, d, a));
      return d;
    }
    void conj(uint32_t d) { code.push_back(fe_ins(FE_CONJ, d)); }
    void frob(uint32_t d, uint32_t n) { code.push_back(fe_ins(FE_FROB, d, n)); }
    void inv6(uint32_t d) { code.push_back(fe_ins(FE_INV6, d)); }
    // a new buffer with base^e (e > 0), square-and-multiply from the top bit; base stays.  Base, result and one more buffer.
    uint32_t pow(uint32_t base, unsigned __int128 e) {
      int top = 127;
      while (!((e >> top) & 1)) top--;
      uint32_t acc = copy(base);
      for (int i = top - 1; i >= 0; i--) {
        uint32_t t = sqr(acc);
        drop(acc);
        acc = t;
        if ((e >> i) & 1) {
          t = mul(acc, base);
          drop(acc);
          acc = t;
        }
      }
      return acc;
    }
  };

  static const std::vector<uint32_t>& fe_program() {
    static const std::vector<uint32_t> prog = [] {
      FeProgram p;
      const uint32_t f = p.take();                       // buffer 0: the conjugated Miller product
      // easy part: f^(q^6 - 1) = conj(f) / f with 1 / f = conj(f) / (f conj(f)) and f conj(f) in F_q6; then ^(q^2 + 1)
      const uint32_t c = p.copy(f);
      p.conj(c);
      const uint32_t n = p.mul(f, c);
      p.drop(f);
      p.inv6(n);
      const uint32_t fi = p.mul(c, n);
      p.drop(n);
      const uint32_t f1 = p.mul(c, fi);
      p.drop(c, fi);
      const uint32_t g = p.copy(f1);
      p.frob(g, 2);
      const uint32_t m = p.mul(g, f1);
      p.drop(g, f1);
      // hard part: the exact exponent (q^4 - q^2 + 1) / r; from here on an inverse is a conjugation
      uint32_t res;
      if (!BN) {
        // ((x - 1)^2 / 3) (x + q) (x^2 + q^2 - 1) + 1,  x = -X
        const unsigned __int128 X = 0xd201000000010000ull, C3 = (X + 1) * (X + 1) / 3;
        const uint32_t y0 = p.pow(m, C3);
        uint32_t t = p.pow(y0, X);
        p.conj(t);                                       // y0^x
        p.frob(y0, 1);
        const uint32_t y1 = p.mul(t, y0);                // y0^(x + q)
        p.drop(t, y0);
        const uint32_t u = p.copy(y1);
        p.frob(u, 2);
        p.conj(y1);
        const uint32_t v = p.mul(u, y1);                 // y1^(q^2 - 1)
        p.conj(y1);
        p.drop(u);
        const uint32_t vm = p.mul(v, m);
        p.drop(v, m);
        t = p.pow(y1, X);
        p.drop(y1);
        const uint32_t t2 = p.pow(t, X);                 // y1^(x^2): the two signs cancel
        p.drop(t);
        res = p.mul(t2, vm);
        p.drop(t2, vm);
      } else {
        // q^3 + (6 x^2 + 1) q^2 + (-36 x^3 - 18 x^2 - 12 x + 1) q + (-36 x^3 - 30 x^2 - 18 x - 2), by Horner in x:
        // ((-36 (q + 1) x + (6 q^2 - 18 q - 30)) x + (-12 q - 18)) x + (q^3 + q^2 + q - 2)
        const unsigned __int128 X = 4965661367192848881ull;
        uint32_t u = p.copy(m);
        p.frob(u, 1);
        uint32_t t = p.mul(u, m);
        p.drop(u);
        uint32_t r = p.pow(t, 36);
        p.drop(t);
        p.conj(r);                                       // m^(-36 (q + 1))
        uint32_t P = p.pow(r, X);
        p.drop(r);
        {                                                // * (m^(q^2) / (m^(3 q) m^5))^6
          u = p.copy(m);
          p.frob(u, 1);
          const uint32_t u3 = p.pow(u, 3);
          p.drop(u);
          const uint32_t m5 = p.pow(m, 5);
          const uint32_t v = p.mul(u3, m5);
          p.drop(u3, m5);
          p.conj(v);
          const uint32_t w = p.copy(m);
          p.frob(w, 2);
          const uint32_t s = p.mul(w, v);
          p.drop(w, v);
          const uint32_t s6 = p.pow(s, 6);
          p.drop(s);
          r = p.mul(P, s6);
          p.drop(P, s6);
        }
        P = p.pow(r, X);
        p.drop(r);
        {                                                // / (m^(2 q) m^3)^6
          u = p.copy(m);
          p.frob(u, 1);
          const uint32_t u2 = p.sqr(u);
          p.drop(u);
          const uint32_t m3 = p.pow(m, 3);
          const uint32_t v = p.mul(u2, m3);
          p.drop(u2, m3);
          const uint32_t s6 = p.pow(v, 6);
          p.drop(v);
          p.conj(s6);
          r = p.mul(P, s6);
          p.drop(P, s6);
        }
        P = p.pow(r, X);
        p.drop(r);
        {                                                // * m^(q^3) m^(q^2) m^q / m^2
          const uint32_t a = p.copy(m);
          p.frob(a, 1);
          const uint32_t b = p.copy(m);
          p.frob(b, 2);
          const uint32_t ab = p.mul(a, b);
          p.drop(a, b);
          const uint32_t c3 = p.copy(m);
          p.frob(c3, 3);
          const uint32_t abc = p.mul(ab, c3);
          p.drop(ab, c3);
          const uint32_t m2 = p.sqr(m);
          p.drop(m);
          p.conj(m2);
          const uint32_t s0 = p.mul(abc, m2);
          p.drop(abc, m2);
          res = p.mul(P, s0);
          p.drop(P, s0);
        }
      }
      if (res != 0) p.code.push_back(fe_ins(FE_COPY, 0, res));
      return p.code;
    }();
    return prog;
  }

  ARK_D static void conj12(uint32_t* f) {
    for (int k = 1; k < 6; k += 2) stc(f, k, Fq2::neg(ldc(f, k)));
  }
  // f^(q^n) coefficient-wise: c_k -> c_k^(q^n) * xi^(k (q^n - 1) / 6); frob[(n - 1) * 6 + k] holds the constants
  ARK_D static void frob12(uint32_t* f, uint32_t n, const Fq2* __restrict__ frob) {
#pragma unroll 1
    for (int k = 0; k < 6; k++) {
      Fq2 c = ldc(f, k);
      if (n != 2) c.c1 = Fq::neg(c.c1);
      stc(f, k, Fq2::mul(c, frob[(n - 1) * 6 + k]));
    }
  }
  // the even coefficients of f are an element of F_q6 = F_q2[v] / (v^3 - xi), v = w^2: invert it in place (one Fq::inv)
  ARK_D static void inv6(uint32_t* f) {
    const Fq2 a0 = ldc(f, 0), a1 = ldc(f, 2), a2 = ldc(f, 4);
    const Fq2 c0 = Fq2::sub(Fq2::sqr_ni(a0), mul_xi(Fq2::mul_ni(a1, a2)));
    const Fq2 c1 = Fq2::sub(mul_xi(Fq2::sqr_ni(a2)), Fq2::mul_ni(a0, a1));
    const Fq2 c2 = Fq2::sub(Fq2::sqr_ni(a1), Fq2::mul_ni(a0, a2));
    const Fq2 t = Fq2::add(Fq2::mul_ni(a0, c0), mul_xi(Fq2::add(Fq2::mul_ni(a2, c1), Fq2::mul_ni(a1, c2))));
    const Fq2 ti = Fq2::inv(t);
    stc(f, 0, Fq2::mul_ni(c0, ti));
    stc(f, 2, Fq2::mul_ni(c1, ti));
    stc(f, 4, Fq2::mul_ni(c2, ti));
    for (int k = 1; k < 6; k += 2) stc(f, k, Fq2::zero());
  }

  // ---- pass A: the lines ---------------------------------------------------------------------------------------------
  struct Proj {
    Fq2 x, y, z;
  };
  // line s of this lane: three F_q2, coefficient c at out + (3 s + c) * W2 * stride
  ARK_D static void put_line(uint32_t* out, size_t stride, uint32_t s, const Fq2& l0, const Fq2& l1, const Fq2& l2) {
    uint32_t* p = out + (size_t)(3 * s) * W2 * stride;
    st(p, stride, l0);
    st(p + (size_t)W2 * stride, stride, l1);
    st(p + (size_t)2 * W2 * stride, stride, l2);
  }
  // Where a line is evaluated.  AtP: at the G1 point of the pair, the x-term times xp and the y-term times yp (pass A per pair).
  // Unevaluated: not yet -- the P-independent coefficients of a prepared G2 point (ark-ec G2Prepared), which
  // pairing_accumulate_key_kernel multiplies by xp and yp when it reads them.
  struct AtP {
    const Fq& xp;
    const Fq& yp;
    ARK_D Fq2 x(const Fq2& a) const { return mul_fq(a, xp); }
    ARK_D Fq2 y(const Fq2& a) const { return mul_fq(a, yp); }
  };
  struct Unevaluated {
    ARK_D Fq2 x(const Fq2& a) const { return a; }
    ARK_D Fq2 y(const Fq2& a) const { return a; }
  };
  // T <- 2T, tangent at T: (i, 3 x^2 . xp, -(h . yp)) in the coefficient order of the curve
  template <class Eval>
  ARK_D static void dbl_step(Proj& T, const Eval& at, const Fq& two_inv, uint32_t* out, size_t stride, uint32_t s) {
    const Fq2 a = mul_fq(Fq2::mul(T.x, T.y), two_inv);
    const Fq2 b = Fq2::sqr(T.y);
    const Fq2 c = Fq2::sqr(T.z);
    const Fq2 e = Fq2::mul(W::g2_b(), Fq2::mul3(c));
    const Fq2 f = Fq2::mul3(e);
    const Fq2 g = mul_fq(Fq2::add(b, f), two_inv);
    const Fq2 h = Fq2::sub(Fq2::sqr(Fq2::add(T.y, T.z)), Fq2::add(b, c));
    const Fq2 i = Fq2::sub(e, b);
    const Fq2 j3 = at.x(Fq2::mul3(Fq2::sqr(T.x)));
    const Fq2 hy = Fq2::neg(at.y(h));
    if (BN) put_line(out, stride, s, hy, j3, i);
    else put_line(out, stride, s, i, j3, hy);
    const Fq2 e2 = Fq2::sqr(e);
    T.x = Fq2::mul(a, Fq2::sub(b, f));
    T.y = Fq2::sub(Fq2::sqr(g), Fq2::mul3(e2));
    T.z = Fq2::mul(b, h);
  }
  // T <- T + Q (Q affine), line through T and Q: (j, -(theta . xp), lambda . yp)
  template <class Eval>
  ARK_D static void add_step(Proj& T, const Fq2& qx, const Fq2& qy, const Eval& at, uint32_t* out, size_t stride, uint32_t s) {
    const Fq2 theta = Fq2::sub(T.y, Fq2::mul(qy, T.z));
    const Fq2 lambda = Fq2::sub(T.x, Fq2::mul(qx, T.z));
    {
      const Fq2 j = Fq2::sub(Fq2::mul(theta, qx), Fq2::mul(lambda, qy));
      const Fq2 tx = Fq2::neg(at.x(theta));
      const Fq2 ly = at.y(lambda);
      if (BN) put_line(out, stride, s, ly, tx, j);
      else put_line(out, stride, s, j, tx, ly);
    }
    const Fq2 c = Fq2::sqr(theta);
    const Fq2 d = Fq2::sqr(lambda);
    const Fq2 e = Fq2::mul(lambda, d);
    const Fq2 f = Fq2::mul(T.z, c);
    const Fq2 g = Fq2::mul(T.x, d);
    const Fq2 h = Fq2::sub(Fq2::add(e, f), Fq2::dbl(g));
    T.x = Fq2::mul(lambda, h);
    T.y = Fq2::sub(Fq2::mul(theta, Fq2::sub(g, h)), Fq2::mul(e, T.y));
    T.z = Fq2::mul(T.z, e);
  }
};

// A pair with either point at infinity contributes 1: it writes no lines and pass B leaves its f at one.
template <class Curve>
__global__ void __launch_bounds__(PAIR_LANES)
pairing_lines_kernel(const Affine<typename Curve::Fq>* __restrict__ g1, const Affine<typename Curve::Fq2>* __restrict__ g2,
                     uint32_t n, uint32_t stride, typename PairingDev<Curve>::Consts k, uint32_t* __restrict__ lines) {
  using D = PairingDev<Curve>;
  using Fq = typename Curve::Fq;
  using Fq2 = typename Curve::Fq2;
  const uint32_t i = blockIdx.x * PAIR_LANES + threadIdx.x;
  if (i >= n) return;
  const Affine<Fq> P = g1[i];
  const Affine<Fq2> Q = g2[i];
  if (P.is_inf() || Q.is_inf()) return;
  // The walk stays in the body of this kernel and pairing_key_lines_kernel repeats it: moved into a shared function it is laid
  // out differently (BN254: other branch polarities around the loop), and this kernel's code object is to stay what it was.
  const typename D::AtP at{P.x, P.y};
  typename D::Proj T{Q.x, Q.y, Fq2::one()};
  uint32_t* out = lines + i;
  uint32_t s = 0;
#pragma unroll 1
  for (int b = D::LOOP_TOP - 1; b >= 0; b--) {
    D::dbl_step(T, at, k.two_inv, out, stride, s++);
    if ((D::LOOP_LO >> b) & 1ull) D::add_step(T, Q.x, Q.y, at, out, stride, s++);
  }
  if (D::BN) {
    // Q1 = pi(Q), Q2 = -pi^2(Q)
    Fq2 x = Q.x, y = Q.y;
#pragma unroll 1
    for (int r = 0; r < 2; r++) {
      x = Fq2::mul(Fq2{x.c0, Fq::neg(x.c1)}, k.frob_x);
      y = Fq2::mul(Fq2{y.c0, Fq::neg(y.c1)}, k.frob_y);
      D::add_step(T, x, r ? Fq2::neg(y) : y, at, out, stride, s++);
    }
  }
}

// f_i = prod over the lines of pair i (squaring before every doubling line); partial[block] = prod of the block's f_i,
// W12 plain dwords each.  PER_PAIR: no workgroup product; every pair's f_i stays in HBM instead, dword-transposed with the
// stride of the lines (partial[d * stride + i]), for pairing_final_exp_kernel.
template <class Curve, bool PER_PAIR = false>
__global__ void __launch_bounds__(PAIR_LANES)
pairing_accumulate_kernel(const Affine<typename Curve::Fq>* __restrict__ g1, const Affine<typename Curve::Fq2>* __restrict__ g2,
                          uint32_t n, uint32_t stride, typename PairingDev<Curve>::Consts k,
                          const uint32_t* __restrict__ lines, uint32_t* __restrict__ partial) {
  using D = PairingDev<Curve>;
  __shared__ uint32_t lds[2 * D::W12 * PAIR_LANES];
  const uint32_t lane = threadIdx.x, i = blockIdx.x * PAIR_LANES + lane;
  uint32_t* f = lds + lane;
  uint32_t* g = lds + D::W12 * PAIR_LANES + lane;
  D::set_one(f);
  bool live = i < n;
  if (live) live = !g1[i].is_inf() && !g2[i].is_inf();
  if (live) {
    const uint32_t* in = lines + i;
#pragma unroll 1
    for (uint32_t s = 0; s < k.steps; s++) {
      if ((k.sqr_mask[s >> 6] >> (s & 63)) & 1ull) {
        D::sqr12(g, f);
        uint32_t* t = f;
        f = g;
        g = t;
      }
      const uint32_t* p = in + (size_t)(3 * s) * D::W2 * stride;
      const auto l0 = D::ld(p, stride), l1 = D::ld(p + (size_t)D::W2 * stride, stride),
                 l2 = D::ld(p + (size_t)2 * D::W2 * stride, stride);
      D::mul12_sparse(g, f, l0, l1, l2);
      uint32_t* t = f;
      f = g;
      g = t;
    }
    if (f != lds + lane) {
      D::copy12(g, f);
      f = lds + lane;
      g = lds + D::W12 * PAIR_LANES + lane;
    }
  }
  if constexpr (PER_PAIR) {
    if (i < n)
      for (uint32_t d = 0; d < D::W12; d++) partial[(size_t)d * stride + i] = f[d * PAIR_LANES];
  } else {
    D::block_product(f, g, lane);
    if (lane == 0)
      for (uint32_t d = 0; d < D::W12; d++) partial[(size_t)blockIdx.x * D::W12 + d] = f[d * PAIR_LANES];
  }
}

// ---- a prepared G2 point (ark-ec G2Prepared; the gamma and delta of a processed verifying key) ----------------------------
// Pass A without a P: lane i < n walks T = [k]q[i] and writes the P-independent coefficients of its lines, (i, 3 x^2, -h)
// and (j, -theta, lambda) in the coefficient order of the curve, PLAIN (not lane-transposed): point i at
// lines + i * steps * 3 * W2, line s at + 3 s W2, three F_q2 as they lie in memory.  Every lane of pass B reads the same
// address, so one address per wave-load is what is wanted.  Cold: one launch per key.  A point at infinity writes nothing.
template <class Curve>
__global__ void __launch_bounds__(PAIR_LANES)
pairing_key_lines_kernel(const Affine<typename Curve::Fq2>* __restrict__ q, uint32_t n, typename PairingDev<Curve>::Consts k,
                         uint32_t* __restrict__ lines) {
  using D = PairingDev<Curve>;
  using Fq = typename Curve::Fq;
  using Fq2 = typename Curve::Fq2;
  const uint32_t i = blockIdx.x * PAIR_LANES + threadIdx.x;
  if (i >= n) return;
  const Affine<Fq2> Q = q[i];
  if (Q.is_inf()) return;
  // the walk of pairing_lines_kernel with the lines left unevaluated, plain layout (stride 1)
  const typename D::Unevaluated at{};
  typename D::Proj T{Q.x, Q.y, Fq2::one()};
  uint32_t* out = lines + (size_t)i * k.steps * 3 * D::W2;
  uint32_t s = 0;
#pragma unroll 1
  for (int b = D::LOOP_TOP - 1; b >= 0; b--) {
    D::dbl_step(T, at, k.two_inv, out, 1, s++);
    if ((D::LOOP_LO >> b) & 1ull) D::add_step(T, Q.x, Q.y, at, out, 1, s++);
  }
  if (D::BN) {
    Fq2 x = Q.x, y = Q.y;
#pragma unroll 1
    for (int r = 0; r < 2; r++) {
      x = Fq2::mul(Fq2{x.c0, Fq::neg(x.c1)}, k.frob_x);
      y = Fq2::mul(Fq2{y.c0, Fq::neg(y.c1)}, k.frob_y);
      D::add_step(T, x, r ? Fq2::neg(y) : y, at, out, 1, s++);
    }
  }
}

// Pass B against prepared points: the PER_PAIR form of pairing_accumulate_kernel for pairs (P_i, Q) whose Q is one of two
// prepared points.  The first blocks_a workgroups take the na points pa[i] against the lines la, the others the nb points
// pb[i] against lb: the selector is uniform over a workgroup, so a wave loads one address per coefficient.  A NULL la / lb
// says that the prepared point is at infinity (every pair of that range contributes one).  Per line the lane multiplies
// the x-term by xp and the y-term by yp -- both fully reduced, and (-h) yp = -(h yp) in the field, so f_i is bit for bit what
// pass A per pair followed by pairing_accumulate_kernel leaves.  xp and yp are read again at every line (96 B from L2
// against 18 F_q2 products) instead of living in 24 registers across the loop.
// f_i goes to mill[d * stride + i * omul + ooff_a / ooff_b]: where pairing_final_exp_kernel expects a member of group i.
template <class Curve>
__global__ void __launch_bounds__(PAIR_LANES)
pairing_accumulate_key_kernel(const Affine<typename Curve::Fq>* __restrict__ pa, uint32_t na, const uint32_t* __restrict__ la,
                              const Affine<typename Curve::Fq>* __restrict__ pb, uint32_t nb, const uint32_t* __restrict__ lb,
                              uint32_t blocks_a, uint32_t stride, uint32_t omul, uint32_t ooff_a, uint32_t ooff_b,
                              typename PairingDev<Curve>::Consts k, uint32_t* __restrict__ mill) {
  using D = PairingDev<Curve>;
  using Fq = typename Curve::Fq;
  __shared__ uint32_t lds[2 * D::W12 * PAIR_LANES];
  const bool second = blockIdx.x >= blocks_a;
  const uint32_t lane = threadIdx.x, i = (blockIdx.x - (second ? blocks_a : 0u)) * PAIR_LANES + lane;
  const uint32_t n = second ? nb : na;
  const Affine<Fq>* __restrict__ g1 = second ? pb : pa;
  const uint32_t* __restrict__ in = second ? lb : la;
  uint32_t* f = lds + lane;
  uint32_t* g = lds + D::W12 * PAIR_LANES + lane;
  D::set_one(f);
  bool live = i < n && in != nullptr;
  if (live) live = !g1[i].is_inf();
  if (live) {
#pragma unroll 1
    for (uint32_t s = 0; s < k.steps; s++) {
      if ((k.sqr_mask[s >> 6] >> (s & 63)) & 1ull) {
        D::sqr12(g, f);
        uint32_t* t = f;
        f = g;
        g = t;
      }
      const uint32_t* p = in + (size_t)(3 * s) * D::W2;
      auto l0 = D::ld(p, 1), l1 = D::ld(p + D::W2, 1), l2 = D::ld(p + 2 * D::W2, 1);
      l1 = D::mul_fq(l1, g1[i].x);
      if (D::BN) l0 = D::mul_fq(l0, g1[i].y);
      else l2 = D::mul_fq(l2, g1[i].y);
      D::mul12_sparse(g, f, l0, l1, l2);
      uint32_t* t = f;
      f = g;
      g = t;
    }
    if (f != lds + lane) {
      D::copy12(g, f);
      f = lds + lane;
    }
  }
  if (i < n) {
    uint32_t* o = mill + (size_t)i * omul + (second ? ooff_b : ooff_a);
    for (uint32_t d = 0; d < D::W12; d++) o[(size_t)d * stride] = f[d * PAIR_LANES];
  }
}

// mill[d * stride + i * omul] = src[d * src_stride + i], i < n: the Miller values pairing_accumulate_kernel<Curve, true>
// left for n pairs, moved to where member 0 of group i belongs (the other members come from pairing_accumulate_key_kernel)
template <class Curve>
__global__ void __launch_bounds__(256)
miller_spread_kernel(const uint32_t* __restrict__ src, uint32_t src_stride, uint32_t n, uint32_t stride, uint32_t omul,
                     uint32_t* __restrict__ mill) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  for (uint32_t d = 0; d < PairingDev<Curve>::W12; d++)
    mill[(size_t)d * stride + (size_t)i * omul] = src[(size_t)d * src_stride + i];
}

// out (W12 plain dwords) = prod of `count` partial products; one workgroup
template <class Curve>
__global__ void __launch_bounds__(PAIR_LANES)
pairing_product_kernel(const uint32_t* __restrict__ partial, uint32_t count, uint32_t* __restrict__ out) {
  using D = PairingDev<Curve>;
  __shared__ uint32_t lds[2 * D::W12 * PAIR_LANES];
  const uint32_t lane = threadIdx.x;
  uint32_t* f = lds + lane;
  uint32_t* g = lds + D::W12 * PAIR_LANES + lane;
  D::set_one(f);
#pragma unroll 1
  for (uint32_t j = lane; j < count; j += PAIR_LANES) {
    D::mul12(g, f, partial + (size_t)j * D::W12, D::W2, 1);
    D::copy12(f, g);
  }
  D::block_product(f, g, lane);
  if (lane == 0)
    for (uint32_t d = 0; d < D::W12; d++) out[d] = f[d * PAIR_LANES];
}

// GT of `groups` groups of group_len consecutive pairs, one lane per group: the product of the group's Miller values
// (mill[d * stride + pair], as pairing_accumulate_kernel<Curve, true> leaves them), conjugated on BLS12-381 (x < 0), taken
// through the program (easy part, then the exact hard exponent (q^4 - q^2 + 1) / r); the result is in buffer 0.
// out_gt (may be NULL): W12 plain dwords per group in the order of ark355_multi_pairing (w^0, w^2, w^4, w^1, w^3, w^5);
// verdict (may be NULL): 1 where the value equals target (W12 dwords, w^0 .. w^5) and bad (may be NULL) is not raised.
template <class Curve>
__global__ void __launch_bounds__(PAIR_LANES)
pairing_final_exp_kernel(const uint32_t* __restrict__ mill, uint32_t stride, uint32_t groups, uint32_t group_len,
                         const uint32_t* __restrict__ prog, uint32_t nsteps, const typename Curve::Fq2* __restrict__ frob,
                         const uint32_t* __restrict__ target, const uint8_t* __restrict__ bad, uint32_t* __restrict__ out_gt,
                         uint8_t* __restrict__ verdict) {
  using D = PairingDev<Curve>;
  __shared__ uint32_t lds[D::FE_BUFS * D::B12];
  const uint32_t lane = threadIdx.x, grp = blockIdx.x * PAIR_LANES + lane;
  if (grp >= groups) return;
  uint32_t* const b0 = lds + lane;
  {
    uint32_t* f = b0;
    uint32_t* g = b0 + D::B12;
    D::set_one(f);
    const uint32_t* in = mill + (size_t)grp * group_len;
#pragma unroll 1
    for (uint32_t j = 0; j < group_len; j++) {
      D::mul12(g, f, in + j, (size_t)D::W2 * stride, stride);
      uint32_t* t = f;
      f = g;
      g = t;
    }
    if (f != b0) D::copy12(b0, f);
    if (!D::BN) D::conj12(b0);
  }
#pragma unroll 1
  for (uint32_t s = 0; s < nsteps; s++) {
    const uint32_t ins = prog[s], a = (ins >> 8) & 15u;
    uint32_t* const pd = b0 + ((ins >> 4) & 15u) * D::B12;
    const uint32_t* const pa = b0 + a * D::B12;
    switch (ins & 15u) {
      case D::FE_SQR: D::sqr12(pd, pa); break;
      case D::FE_MUL: D::mul12(pd, pa, b0 + ((ins >> 12) & 15u) * D::B12, D::CK, PAIR_LANES); break;
      case D::FE_COPY: D::copy12(pd, pa); break;
      case D::FE_CONJ: D::conj12(pd); break;
      case D::FE_FROB: D::frob12(pd, a, frob); break;
      default: D::inv6(pd); break;
    }
  }
  bool same = true;
  for (uint32_t d = 0; d < D::W12; d++) same = same && b0[d * PAIR_LANES] == target[d];
  if (verdict) verdict[grp] = same && !(bad && bad[grp]) ? 1 : 0;
  if (out_gt) {
    uint32_t* o = out_gt + (size_t)grp * D::W12;
    for (uint32_t sl = 0; sl < 6; sl++) {
      const uint32_t k = sl < 3 ? 2 * sl : 2 * (sl - 3) + 1;
      for (uint32_t d = 0; d < D::W2; d++) o[sl * D::W2 + d] = b0[(k * D::W2 + d) * PAIR_LANES];
    }
  }
}

// out[j] = s[j] * P[j] in G1 (canonical scalars), affine: the rho_j A_j of batch verification
template <class Curve>
__global__ void __launch_bounds__(128)
g1_scalar_mul_kernel(const Affine<typename Curve::Fq>* __restrict__ p, const typename Curve::Fr* __restrict__ s, uint64_t n,
                     Affine<typename Curve::Fq>* __restrict__ out) {
  using Fq = typename Curve::Fq;
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const typename Curve::Fr k = s[i];
  out[i] = xyzz_to_affine(xyzz_mul_scalar(XYZZ<Fq>::from_affine(p[i]), k.l, Curve::Fr::N));
}

// y^2 = x^3 + b for n1 points of G1 and n2 points of G2 (infinity passes), one lane per point; *err receives the smallest
// (index + 1) << 4 | group of a failing point (0 = all good), the word wire_decode_kernel reports with
template <class Curve>
__global__ void __launch_bounds__(128)
on_curve_kernel(const Affine<typename Curve::Fq>* __restrict__ g1, uint64_t n1, const Affine<typename Curve::Fq2>* __restrict__ g2,
                uint64_t n2, unsigned long long* __restrict__ err) {
  using W = Wire<Curve>;
  using Fq = typename Curve::Fq;
  using Fq2 = typename Curve::Fq2;
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n1 + n2) return;
  bool good;
  if (i < n1) {
    const Affine<Fq> a = g1[i];
    good = a.is_inf() || Fq::sqr_ni(a.y) == W::curve_rhs(a.x);
  } else {
    const Affine<Fq2> a = g2[i - n1];
    good = a.is_inf() || Fq2::sqr_ni(a.y) == W::curve_rhs(a.x);
  }
  if (!good) {
    const unsigned long long code = i < n1 ? (((i + 1) << 4) | 1ull) : (((i - n1 + 1) << 4) | 2ull);
    unsigned long long cur = *err;
    while (cur == 0 || code < cur) {
      const unsigned long long prev = atomicCAS(err, cur, code);
      if (prev == cur) break;
      cur = prev;
    }
  }
}

// the same equations, one byte per point: flags[i] = 1 where G1 point i / G2 point i - n1 is off its curve
template <class Curve>
__global__ void __launch_bounds__(128)
on_curve_flags_kernel(const Affine<typename Curve::Fq>* __restrict__ g1, uint64_t n1, const Affine<typename Curve::Fq2>* __restrict__ g2,
                      uint64_t n2, uint8_t* __restrict__ flags) {
  using W = Wire<Curve>;
  using Fq = typename Curve::Fq;
  using Fq2 = typename Curve::Fq2;
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n1 + n2) return;
  bool good;
  if (i < n1) {
    const Affine<Fq> a = g1[i];
    good = a.is_inf() || Fq::sqr_ni(a.y) == W::curve_rhs(a.x);
  } else {
    const Affine<Fq2> a = g2[i - n1];
    good = a.is_inf() || Fq2::sqr_ni(a.y) == W::curve_rhs(a.x);
  }
  flags[i] = good ? 0 : 1;
}

// prod[j * m + i] = x_ji * gamma_abc_{i+1}: the terms of the prepared inputs of ark355_verify_each, one lane per product; the
// public inputs arrive in Montgomery form and are made canonical here
template <class Curve>
__global__ void __launch_bounds__(128)
prepared_input_terms_kernel(const Affine<typename Curve::Fq>* __restrict__ gamma_abc, const typename Curve::Fr* __restrict__ x,
                            uint64_t count, uint32_t m, XYZZ<typename Curve::Fq>* __restrict__ prod) {
  using Fq = typename Curve::Fq;
  using Fr = typename Curve::Fr;
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count * m) return;
  const Fr k = Fr::from_mont(x[t]);
  prod[t] = xyzz_mul_scalar(XYZZ<Fq>::from_affine(gamma_abc[1 + t % m]), k.l, Fr::N);
}

// one lane per proof: acc_j = gamma_abc_0 + sum_i prod[j * m + i], then the three pairs of the proof,
// (A_j, B_j), (-acc_j, gamma), (-C_j, delta), at 3 j .. 3 j + 2 of p / q, and bad[j] from the flags of A_j, C_j, B_j
// (ac = A_0 .. A_{count-1}, C_0 .. C_{count-1}; flags in the order on_curve_flags_kernel saw them: ac, then b)
template <class Curve>
__global__ void __launch_bounds__(128)
verify_each_pairs_kernel(const Affine<typename Curve::Fq>* __restrict__ gamma_abc, const XYZZ<typename Curve::Fq>* __restrict__ prod,
                         uint32_t m, const Affine<typename Curve::Fq>* __restrict__ ac, const Affine<typename Curve::Fq2>* __restrict__ b,
                         const Affine<typename Curve::Fq2>* __restrict__ gamma_delta, const uint8_t* __restrict__ flags, uint64_t count,
                         Affine<typename Curve::Fq>* __restrict__ p, Affine<typename Curve::Fq2>* __restrict__ q,
                         uint8_t* __restrict__ bad) {
  using Fq = typename Curve::Fq;
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count) return;
  XYZZ<Fq> acc = XYZZ<Fq>::from_affine(gamma_abc[0]);
  for (uint32_t i = 0; i < m; i++) acc = xyzz_add(acc, prod[j * m + i]);
  const Affine<Fq> s = xyzz_to_affine(acc), c = ac[count + j];
  p[3 * j] = ac[j];
  p[3 * j + 1] = s.is_inf() ? s : Affine<Fq>::neg(s);
  p[3 * j + 2] = c.is_inf() ? c : Affine<Fq>::neg(c);
  q[3 * j] = b[j];
  q[3 * j + 1] = gamma_delta[0];
  q[3 * j + 2] = gamma_delta[1];
  bad[j] = flags[j] | flags[count + j] | flags[2 * count + j];
}

// ark355_verify_each_pvk, one lane per proof: nacc[j] = -(gamma_abc_0 + sum_i prod[j * m + i]) and negc[j] = -C_j, the first
// arguments of the pairs against the prepared gamma and delta, and bad[j] as verify_each_pairs_kernel forms it.  The pair
// (A_j, B_j) is read where it was staged; nothing of the key is copied next to the proofs.
template <class Curve>
__global__ void __launch_bounds__(128)
verify_each_key_pairs_kernel(const Affine<typename Curve::Fq>* __restrict__ gamma_abc, const XYZZ<typename Curve::Fq>* __restrict__ prod,
                             uint32_t m, const Affine<typename Curve::Fq>* __restrict__ ac, const uint8_t* __restrict__ flags,
                             uint64_t count, Affine<typename Curve::Fq>* __restrict__ nacc, Affine<typename Curve::Fq>* __restrict__ negc,
                             uint8_t* __restrict__ bad) {
  using Fq = typename Curve::Fq;
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count) return;
  XYZZ<Fq> acc = XYZZ<Fq>::from_affine(gamma_abc[0]);
  for (uint32_t i = 0; i < m; i++) acc = xyzz_add(acc, prod[j * m + i]);
  const Affine<Fq> s = xyzz_to_affine(acc), c = ac[count + j];
  nacc[j] = s.is_inf() ? s : Affine<Fq>::neg(s);
  negc[j] = c.is_inf() ? c : Affine<Fq>::neg(c);
  bad[j] = flags[j] | flags[count + j] | flags[2 * count + j];
}

}  // namespace ark355
