// Host drivers of the pairing entry points: ark355_multi_pairing, ark355_pairing_groups, ark355_verify_each and
// ark355_verify_batch, and of the processed verifying key (ark355_vk_process and the ark355_*_pvk entries).  Each has a host
// route (pairing_host.hpp on at most 16 host threads) and a device route (the kernels of pairing_impl.cuh); policy
// PAIRING_DEVICE chooses.  Api<Curve> (api_impl.cuh) forwards here.
#pragma once
#include <chrono>
#include <thread>
#include "common.h"
#include "wire_impl.cuh"
#include "pairing_host.hpp"
#include "pairing_impl.cuh"

namespace ark355 {

// grow-only device buffers of the device routes (a member of GenericScratch)
struct PairingScratch {
  DevBuf pg1, pg2, plines, ppart, pout, psc;      // points, lines, partial products, the Miller product, scalars
  DevBuf pmill, pfe, pgt, pverd;                  // per-group pairings: Miller values of a chunk, program + constants, GT values, verdicts
  DevBuf pabc, pprod, pflags;                     // ark355_verify_each: gamma_abc, the terms of the prepared inputs, per-point flags
  DevBuf pkmill;                                  // the *_pvk entries: Miller values of a chunk, three members per proof
  DevBuf pbytes, ppst, pstatus;                   // the *_bytes entries: the wire bytes, the status of every point, of every proof
};

// ark355_pvk: what SNARK::process_vk computes once per key.  Immutable after ark355_vk_process; the device buffers belong to
// the handle, not to the context that made it, so any context of `device` may use it, the creating one destroyed or not.
struct PvkDev {
  int curve = 0, device = 0;
  uint64_t ell = 0;
  uint32_t steps = 0;                 // lines per prepared point
  bool inf[3] = {false, false, false};   // beta, gamma, delta at infinity: no lines, the pairs contribute one
  std::vector<uint8_t> alpha, g2;     // host: alpha_g1; beta_g2, gamma_g2, delta_g2 (raw images)
  std::vector<uint8_t> abc_host;      // host: gamma_abc_g1, the bases of ark355_verify_batch_pvk's one-shot MSM and of the host route
  std::vector<uint8_t> alpha_beta;    // host: e(alpha, beta), 12 Fq in the layout of ark355_multi_pairing
  DevBuf abc;                         // ell G1
  DevBuf lines;                       // 3 x steps x 3 F_q2, plain: the P-independent line coefficients of beta, gamma, delta
  size_t abc_bytes = 0, lines_bytes = 0;
  size_t resident_bytes() const { return abc_bytes + lines_bytes; }
};

template <class Curve>
struct Verify {
  using Fr = typename Curve::Fr;
  using Fq = typename Curve::Fq;
  using Fq2 = typename Curve::Fq2;
  using G1 = Affine<Fq>;
  using G2 = Affine<Fq2>;
  using W = Wire<Curve>;
  using PH = PairingHost<Curve>;
  using PD = PairingDev<Curve>;
  using Gt = typename PH::Fq12;
  static constexpr bool BN = Curve::ID == ARK355_BN254;
  // At most PAIR_CHUNK pairs have their lines in HBM at a time (about 20 KB per pair).
  static constexpr uint64_t PAIR_CHUNK = 1u << 15;
  // ark355_verify_each_pvk: proofs per chunk.  One pair in three still has lines of its own, so a chunk holds as many proofs
  // as PAIR_CHUNK holds pairs (the same HBM for lines, three Miller values per proof: 56 MB on BLS12-381).
  static constexpr uint64_t PVK_EACH_CHUNK = PAIR_CHUNK;
  // ark355_pvk_pairings: pairs per chunk; no lines at all, the chunk bounds the Miller values in HBM (576 B per pair)
  static constexpr uint64_t PVK_PAIR_CHUNK = 1u << 17;

  ark355_ctx* ctx;
  PairingScratch& s;
  DevBuf& word;            // GenericScratch::c: the 8 bytes on_curve_kernel reports with

  // ---- shared helpers ------------------------------------------------------------------------------------------------
  // policy PAIRING_DEVICE: 0 host threads, 1 device, -1 device from `threshold` units on.  PAIRING_DEVICE_MIN counts pairs
  // (n for multi_pairing, count + 3 for verify_batch); PAIRING_EACH_MIN counts groups / proofs (the host pays one final
  // exponentiation per group there, so the crossover is not that of the two entries with one exponentiation per call).
  bool on_device(int32_t threshold, uint64_t units) const {
    if (ctx->policy.pairing_device == 0) return false;
    if (ctx->policy.pairing_device > 0) return true;
    return units >= (uint64_t)std::max<int64_t>(threshold, 0);
  }
  static double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
  }
  void trace(const char* what, bool device, uint64_t n, double check_ms, double mul_ms, double miller_ms, double fe_ms) const {
    if (ctx->policy.trace_host)
      fprintf(stderr, "[ark355] %s route=%s pairs=%llu check_ms=%.3f scalar_mul_ms=%.3f miller_ms=%.3f final_exp_ms=%.3f\n", what,
              device ? "device" : "host", (unsigned long long)n, check_ms, mul_ms, miller_ms, fe_ms);
  }

  static G1 load_g1(const uint8_t* p) {
    G1 a;
    memcpy(&a, p, sizeof(a));
    return a;
  }
  static G2 load_g2(const uint8_t* p) {
    G2 a;
    memcpy(&a, p, sizeof(a));
    return a;
  }
  // y^2 = x^3 + b (infinity passes).  The raw entry points take Montgomery images, not validated encodings: a point off the
  // curve must not reach the Miller loop (its line functions never use the curve constant, (0, y) / y = 0 cases would divide
  // by zero silently).  Subgroup membership is ark355_proof_from_bytes' job (ARK355_VALIDATE_FULL), as upstream splits it
  // between deserialization and verification.
  template <class F>
  static bool on_curve(const Affine<F>& a) {
    return a.is_inf() || F::sqr_ni(a.y) == W::curve_rhs(a.x);
  }
  [[noreturn]] static void refuse(const std::string& what) { throw HipError{ARK355_EINVAL, what + ": point not on curve"}; }
  static std::string at(const char* array, uint64_t i) { return std::string(array) + "[" + std::to_string(i) + "]"; }
  // the word of on_curve_kernel: (index + 1) << 4 | group of the first failing point
  static void refuse_word(unsigned long long e) { refuse(at((e & 15) == 1 ? "g1" : "g2", (e >> 4) - 1)); }
  static bool exponent_formed() { return !PH::consts().final_exp.l.empty(); }
  static Gt final_exp(const Gt& f) {
    ARK_REQUIRE(exponent_formed(), ARK355_EINVAL, "the final exponent could not be formed");
    return PH::final_exponentiation(f);
  }

  static unsigned host_threads() {
    unsigned nt = std::thread::hardware_concurrency();
    if (nt == 0) nt = 4;
    return nt > 16 ? 16 : nt;
  }
  // `units` independent jobs on at most 16 host threads, thread t of T taking units t, t + T, ...
  template <class Fn>
  static void host_each(uint64_t units, Fn&& fn) {
    const unsigned threads = (unsigned)std::min<uint64_t>(host_threads(), units);
    (void)PH::consts();                               // build the constants before the threads start
    std::vector<std::thread> th;
    for (unsigned t = 0; t < threads; t++)
      th.emplace_back([&, t] {
        for (uint64_t u = t; u < units; u += threads) fn(u);
      });
    for (auto& x : th) x.join();
  }
  // prod_i miller_loop(P_i, Q_i): as many strands as host_each has threads, one partial product each
  static Gt miller_product_host(const std::vector<G1>& Ps, const std::vector<G2>& Qs) {
    const size_t n = Ps.size();
    std::vector<Gt> part(std::min<size_t>(host_threads(), n), Gt::one());
    host_each(part.size(), [&](uint64_t t) {
      for (size_t i = t; i < n; i += part.size()) part[t] = Gt::mul(part[t], PH::miller_loop(Ps[i], Qs[i]));
    });
    Gt f = Gt::one();
    for (const auto& p : part) f = Gt::mul(f, p);
    return f;
  }

  // ---- device stages -------------------------------------------------------------------------------------------------
  // both point arrays of a call into s.pg1 / s.pg2; the first point off its curve is refused by name
  void upload_checked(const uint8_t* g1, const uint8_t* g2, uint64_t n) {
    hipStream_t st = ctx->stream;
    s.pg1.ensure(n * sizeof(G1));
    s.pg2.ensure(n * sizeof(G2));
    ARK_CHECK_HIP(hipMemcpyAsync(s.pg1.p, g1, n * sizeof(G1), hipMemcpyHostToDevice, st));
    ARK_CHECK_HIP(hipMemcpyAsync(s.pg2.p, g2, n * sizeof(G2), hipMemcpyHostToDevice, st));
    if (const unsigned long long e = on_curve_dev(s.pg1.p, n, s.pg2.p, n)) refuse_word(e);
  }
  // the curve equation on the device for n1 + n2 resident points; returns the kernel's word (0: all on their curves)
  unsigned long long on_curve_dev(const void* d_g1, uint64_t n1, const void* d_g2, uint64_t n2) {
    if (n1 + n2 == 0) return 0;
    hipStream_t st = ctx->stream;
    word.ensure(8);
    ARK_CHECK_HIP(hipMemsetAsync(word.p, 0, 8, st));
    ARK_LAUNCH((on_curve_kernel<Curve>), dim3((uint32_t)((n1 + n2 + 127) / 128)), dim3(128), 0, st,
               reinterpret_cast<const G1*>(d_g1), n1, reinterpret_cast<const G2*>(d_g2), n2, word.as<unsigned long long>());
    ARK_CHECK_LAUNCH();
    unsigned long long e = 0;
    ARK_CHECK_HIP(hipMemcpyAsync(&e, word.p, 8, hipMemcpyDeviceToHost, st));
    ARK_CHECK_HIP(hipStreamSynchronize(st));
    return e;
  }

  // The proofs of a call staged as the kernels read them: s.pg1 = A_0 .. A_{count-1}, C_0 .. C_{count-1}, s.pg2 = B_j, with
  // room for cap1 / cap2 points (what the entry puts behind them).  The uploads are asynchronous: the caller keeps the
  // returned host copies until it has synchronised the stream.
  struct StagedProofs {
    std::vector<G1> ac;
    std::vector<G2> bs;
  };
  StagedProofs stage_proofs(const ark355_proof_raw* proofs, uint64_t count, uint64_t cap1, uint64_t cap2) {
    StagedProofs h{std::vector<G1>(2 * count), std::vector<G2>(count)};
    for (uint64_t j = 0; j < count; j++) {
      h.ac[j] = load_g1(proofs[j].a);
      h.ac[count + j] = load_g1(proofs[j].c);
      h.bs[j] = load_g2(proofs[j].b);
    }
    s.pg1.ensure(cap1 * sizeof(G1));
    s.pg2.ensure(cap2 * sizeof(G2));
    ARK_CHECK_HIP(hipMemcpyAsync(s.pg1.p, h.ac.data(), 2 * count * sizeof(G1), hipMemcpyHostToDevice, ctx->stream));
    ARK_CHECK_HIP(hipMemcpyAsync(s.pg2.p, h.bs.data(), count * sizeof(G2), hipMemcpyHostToDevice, ctx->stream));
    return h;
  }

  static typename PD::Consts dev_consts() {
    typename PD::Consts k{};
    PD::schedule(&k);
    k.two_inv = Fq::inv(Fq::add(Fq::one(), Fq::one()));
    k.frob_x = PH::consts().frob_x;
    k.frob_y = PH::consts().frob_y;
    return k;
  }

  // Passes A and B of pairing_impl.cuh over `pairs` resident pairs (every point on its curve), `chunk` <= PAIR_CHUNK at a
  // time.  PER_PAIR: every pair's Miller value of the chunk is left in s.pmill (dword-transposed, stride as handed to
  // per_chunk); otherwise the product of workgroup b of the whole call is left at s.ppart + b * W12.
  // per_chunk(first pair, pairs of the chunk, stride) runs after the two launches of each chunk.
  template <bool PER_PAIR, class PerChunk>
  void miller_chunks(const G1* d1, const G2* d2, uint64_t pairs, uint64_t chunk, PerChunk&& per_chunk) {
    hipStream_t st = ctx->stream;
    const typename PD::Consts k = dev_consts();
    const uint32_t stride = (uint32_t)((std::min(pairs, chunk) + PAIR_LANES - 1) / PAIR_LANES * PAIR_LANES);
    s.plines.ensure((size_t)k.steps * 3 * PD::W2 * stride * sizeof(uint32_t));
    if (PER_PAIR) s.pmill.ensure((size_t)PD::W12 * stride * sizeof(uint32_t));
    else s.ppart.ensure((pairs + PAIR_LANES - 1) / PAIR_LANES * PD::W12 * sizeof(uint32_t));
    for (uint64_t off = 0; off < pairs; off += chunk) {
      const uint32_t m = (uint32_t)std::min(chunk, pairs - off);
      const dim3 grid((m + PAIR_LANES - 1) / PAIR_LANES);
      ARK_LAUNCH((pairing_lines_kernel<Curve>), grid, dim3(PAIR_LANES), 0, st, d1 + off, d2 + off, m, stride, k,
                 s.plines.as<uint32_t>());
      ARK_CHECK_LAUNCH();
      ARK_LAUNCH((pairing_accumulate_kernel<Curve, PER_PAIR>), grid, dim3(PAIR_LANES), 0, st, d1 + off, d2 + off, m, stride, k,
                 (const uint32_t*)s.plines.as<uint32_t>(),
                 PER_PAIR ? s.pmill.as<uint32_t>() : s.ppart.as<uint32_t>() + (off / PAIR_LANES) * PD::W12);
      ARK_CHECK_LAUNCH();
      per_chunk(off, m, stride);
    }
  }

  // prod_i miller_loop(P_i, Q_i) for n resident pairs; the partial products of all chunks meet in one last launch
  Gt multi_miller_dev(const G1* d1, const G2* d2, uint64_t n) {
    if (n == 0) return Gt::one();
    hipStream_t st = ctx->stream;
    s.pout.ensure(PD::W12 * sizeof(uint32_t));
    miller_chunks<false>(d1, d2, n, PAIR_CHUNK, [](uint64_t, uint32_t, uint32_t) {});
    ARK_LAUNCH((pairing_product_kernel<Curve>), dim3(1), dim3(PAIR_LANES), 0, st, (const uint32_t*)s.ppart.as<uint32_t>(),
               (uint32_t)((n + PAIR_LANES - 1) / PAIR_LANES), s.pout.as<uint32_t>());
    ARK_CHECK_LAUNCH();
    Fq2 c[6];
    ARK_CHECK_HIP(hipMemcpyAsync(c, s.pout.p, sizeof(c), hipMemcpyDeviceToHost, st));
    ARK_CHECK_HIP(hipStreamSynchronize(st));
    // coefficients of w^0 .. w^5 -> the tower of pairing_host.hpp (v = w^2)
    Gt f{{c[0], c[2], c[4]}, {c[1], c[3], c[5]}};
    return BN ? f : Gt::conj(f);      // BLS12-381: x < 0
  }

  // GT of `groups` groups of group_len consecutive resident pairs (every point on its curve, or its group marked in d_bad).
  // out_gt: groups x 12 Fq (host, may be NULL); verdict: groups bytes (host), 1 where GT == target and the group is not bad.
  // A chunk holds whole groups; its lines and Miller values are in HBM at a time.
  void groups_dev(const G1* d1, const G2* d2, uint64_t groups, uint32_t group_len, const Gt& target, const uint8_t* d_bad,
                  uint8_t* out_gt, uint8_t* verdict) {
    const FeDev fe = fe_upload(target);
    if (out_gt) s.pgt.ensure(groups * PD::W12 * sizeof(uint32_t));
    s.pverd.ensure(groups);
    miller_chunks<true>(d1, d2, groups * group_len, PAIR_CHUNK / group_len * group_len, [&](uint64_t off, uint32_t m, uint32_t stride) {
      fe_launch(fe, s.pmill.as<uint32_t>(), stride, off / group_len, m / group_len, group_len, d_bad, out_gt != nullptr);
    });
    fe_download(groups, out_gt, verdict);
  }

  // the final exponentiation's program and constants in s.pfe: 18 Frobenius constants, the target (the kernels' order:
  // coefficients of w^0 .. w^5), the instructions
  struct FeDev {
    const Fq2* frob;
    const uint32_t* tgt;
    const uint32_t* prog;
    uint32_t nsteps;
    std::vector<uint8_t> blob;      // the host image: the upload is asynchronous, the caller keeps this until it has synchronised
  };
  FeDev fe_upload(const Gt& target) {
    const std::vector<uint32_t>& prog = PD::fe_program();
    const size_t frob_bytes = 18 * sizeof(Fq2), tgt_bytes = PD::W12 * sizeof(uint32_t);
    std::vector<uint8_t> blob(frob_bytes + tgt_bytes + prog.size() * sizeof(uint32_t));
    memcpy(blob.data(), PH::consts().frob12, frob_bytes);
    const Fq2 tc[6] = {target.c0.c0, target.c1.c0, target.c0.c1, target.c1.c1, target.c0.c2, target.c1.c2};
    memcpy(blob.data() + frob_bytes, tc, tgt_bytes);
    memcpy(blob.data() + frob_bytes + tgt_bytes, prog.data(), prog.size() * sizeof(uint32_t));
    s.pfe.ensure(blob.size());
    ARK_CHECK_HIP(hipMemcpyAsync(s.pfe.p, blob.data(), blob.size(), hipMemcpyHostToDevice, ctx->stream));
    const uint32_t* d_tgt = reinterpret_cast<const uint32_t*>(s.pfe.as<uint8_t>() + frob_bytes);
    return FeDev{s.pfe.as<Fq2>(), d_tgt, d_tgt + PD::W12, (uint32_t)prog.size(), std::move(blob)};
  }
  // groups g0 .. g0 + ng - 1 of the call from the Miller values of a chunk (mill[d * stride + pair]) into s.pgt / s.pverd
  void fe_launch(const FeDev& fe, const uint32_t* mill, uint32_t stride, uint64_t g0, uint32_t ng, uint32_t group_len,
                 const uint8_t* d_bad, bool want_gt) {
    ARK_LAUNCH((pairing_final_exp_kernel<Curve>), dim3((ng + PAIR_LANES - 1) / PAIR_LANES), dim3(PAIR_LANES), 0, ctx->stream, mill,
               stride, ng, group_len, fe.prog, fe.nsteps, fe.frob, fe.tgt, d_bad ? d_bad + g0 : nullptr,
               want_gt ? s.pgt.as<uint32_t>() + g0 * PD::W12 : nullptr, s.pverd.as<uint8_t>() + g0);
    ARK_CHECK_LAUNCH();
  }
  void fe_download(uint64_t groups, uint8_t* out_gt, uint8_t* verdict) {
    hipStream_t st = ctx->stream;
    if (out_gt) ARK_CHECK_HIP(hipMemcpyAsync(out_gt, s.pgt.p, groups * PD::W12 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    ARK_CHECK_HIP(hipMemcpyAsync(verdict, s.pverd.p, groups, hipMemcpyDeviceToHost, st));
    ARK_CHECK_HIP(hipStreamSynchronize(st));
  }

  // the host route's curve checks of two raw point arrays, refused by name like the device route's
  static void check_host(const uint8_t* g1, const uint8_t* g2, uint64_t n) {
    for (uint64_t i = 0; i < n; i++) {
      if (!on_curve(load_g1(g1 + i * sizeof(G1)))) refuse(at("g1", i));
      if (!on_curve(load_g2(g2 + i * sizeof(G2)))) refuse(at("g2", i));
    }
  }

  // ---- the entry points ----------------------------------------------------------------------------------------------
  // ark-ec Pairing::multi_pairing over raw affine images
  void multi_pairing(const uint8_t* g1, const uint8_t* g2, uint64_t n, uint8_t* out_gt, int32_t* is_one) {
    const bool dev = n > 0 && on_device(ctx->policy.pairing_device_min, n);
    const double t0 = now_ms();
    double t1 = t0;
    Gt f = Gt::one();
    if (dev) {
      upload_checked(g1, g2, n);
      t1 = now_ms();
      f = multi_miller_dev(s.pg1.as<G1>(), s.pg2.as<G2>(), n);
    } else if (n > 0) {
      check_host(g1, g2, n);
      std::vector<G1> Ps(n);
      std::vector<G2> Qs(n);
      memcpy(Ps.data(), g1, n * sizeof(G1));
      memcpy(Qs.data(), g2, n * sizeof(G2));
      t1 = now_ms();
      f = miller_product_host(Ps, Qs);
    }
    const double t2 = now_ms();
    const Gt gt = final_exp(f);
    trace("multi_pairing", dev, n, t1 - t0, 0.0, t2 - t1, now_ms() - t2);
    if (out_gt) memcpy(out_gt, &gt, sizeof(gt));
    if (is_one) *is_one = gt == Gt::one() ? 1 : 0;
  }

  // ark-ec Pairing::pairing per group of group_len consecutive pairs
  void pairing_groups(const uint8_t* g1, const uint8_t* g2, uint64_t groups, uint32_t group_len, uint8_t* out_gt, uint8_t* is_one) {
    ARK_REQUIRE(group_len >= 1 && group_len <= ARK355_PAIRING_GROUP_MAX, ARK355_EINVAL,
                "group_len must be 1 .. 64 (one long product is ark355_multi_pairing's)");
    if (groups == 0) return;
    ARK_REQUIRE(groups <= 0xFFFFFFFFull / group_len, ARK355_EINVAL, "groups * group_len must stay below 2^32");
    ARK_REQUIRE(g1 && g2, ARK355_EINVAL, "a point array is NULL");
    ARK_REQUIRE(exponent_formed(), ARK355_EINVAL, "the final exponent could not be formed");
    const uint64_t n = groups * group_len;
    const bool dev = on_device(ctx->policy.pairing_each_min, groups);
    const double t0 = now_ms();
    double t1 = t0;
    std::vector<uint8_t> verdict(groups);
    if (dev) {
      upload_checked(g1, g2, n);
      t1 = now_ms();
      groups_dev(s.pg1.as<G1>(), s.pg2.as<G2>(), groups, group_len, Gt::one(), nullptr, out_gt, verdict.data());
    } else {
      check_host(g1, g2, n);
      t1 = now_ms();
      host_each(groups, [&](uint64_t k) {
        Gt f = Gt::one();
        for (uint64_t i = k * group_len; i < (k + 1) * group_len; i++)
          f = Gt::mul(f, PH::miller_loop(load_g1(g1 + i * sizeof(G1)), load_g2(g2 + i * sizeof(G2))));
        const Gt gt = PH::final_exponentiation(f);
        if (out_gt) memcpy(out_gt + k * sizeof(Gt), &gt, sizeof(gt));
        verdict[k] = gt == Gt::one() ? 1 : 0;
      });
    }
    if (is_one) memcpy(is_one, verdict.data(), groups);
    trace("pairing_groups", dev, n, t1 - t0, 0.0, now_ms() - t1, 0.0);
  }

  // the host route of ark355_verify_each and ark355_verify_each_pvk: one proof per unit of host_each
  static void each_host(const G1* abc, uint32_t m, const G2& gamma, const G2& delta, const Gt& target, const ark355_proof_raw* proofs,
                        const uint8_t* inputs, uint64_t count, uint8_t* ok) {
    host_each(count, [&](uint64_t j) {
      const G1 a = load_g1(proofs[j].a), c = load_g1(proofs[j].c);
      const G2 b = load_g2(proofs[j].b);
      ok[j] = 0;
      if (!on_curve(a) || !on_curve(c) || !on_curve(b)) return;
      XYZZ<Fq> acc = XYZZ<Fq>::from_affine(abc[0]);
      for (uint32_t i = 0; i < m; i++) {
        Fr x;
        memcpy(x.l, inputs + ((size_t)j * m + i) * sizeof(Fr), sizeof(Fr));
        const Fr kx = Fr::from_mont(x);
        acc = xyzz_add(acc, xyzz_mul_scalar(XYZZ<Fq>::from_affine(abc[1 + i]), kx.l, Fr::N));
      }
      const G1 sum = xyzz_to_affine(acc);
      Gt f = PH::miller_loop(a, b);
      f = Gt::mul(f, PH::miller_loop(sum.is_inf() ? sum : G1::neg(sum), gamma));
      f = Gt::mul(f, PH::miller_loop(c.is_inf() ? c : G1::neg(c), delta));
      ok[j] = PH::final_exponentiation(f) == target ? 1 : 0;
    });
  }

  // ark-groth16 verify_proof for every proof of one key on its own: e(A_j, B_j) e(-acc_j, gamma) e(-C_j, delta) == e(alpha, beta)
  void verify_each(const ark355_vk_desc* vk, const ark355_proof_raw* proofs, const uint8_t* inputs, uint64_t count, uint8_t* ok) {
    const uint64_t ell = vk->num_instance;
    ARK_REQUIRE(ell >= 1, ARK355_EINVAL, "empty key");
    if (count == 0) return;
    ARK_REQUIRE(ell == 1 || inputs, ARK355_EINVAL, "public_inputs is NULL");
    ARK_REQUIRE(count <= 0xFFFFFFFFull / 3, ARK355_EINVAL, "3 * count must stay below 2^32");
    ARK_REQUIRE(exponent_formed(), ARK355_EINVAL, "the final exponent could not be formed");
    const uint32_t m = (uint32_t)(ell - 1);
    // the key's own points, once
    const double t0 = now_ms();
    const G1 alpha = load_g1(vk->alpha_g1);
    const G2 beta = load_g2(vk->beta_g2), gamma = load_g2(vk->gamma_g2), delta = load_g2(vk->delta_g2);
    if (!on_curve(alpha)) refuse("vk.alpha_g1");
    if (!on_curve(beta)) refuse("vk.beta_g2");
    if (!on_curve(gamma)) refuse("vk.gamma_g2");
    if (!on_curve(delta)) refuse("vk.delta_g2");
    std::vector<G1> abc(ell);
    memcpy(abc.data(), vk->gamma_abc_g1, ell * sizeof(G1));
    for (uint64_t i = 0; i < ell; i++)
      if (!on_curve(abc[i])) refuse(at("vk.gamma_abc_g1", i));
    const Gt target = PH::final_exponentiation(PH::miller_loop(alpha, beta));
    const double t1 = now_ms();
    const bool dev = on_device(ctx->policy.pairing_each_min, count);
    if (dev) {
      hipStream_t st = ctx->stream;
      // behind the staged proofs: s.pg1 the 3 count first arguments; s.pg2 the 3 count second arguments, gamma, delta
      const StagedProofs staged = stage_proofs(proofs, count, 5 * count, 4 * count + 2);
      const G2 gd[2] = {gamma, delta};
      s.pabc.ensure(ell * sizeof(G1));
      s.pflags.ensure(4 * count);
      G1* d_ac = s.pg1.as<G1>();
      G2* d_b = s.pg2.as<G2>();
      uint8_t* d_flags = s.pflags.as<uint8_t>();
      ARK_CHECK_HIP(hipMemcpyAsync(d_b + 4 * count, gd, sizeof(gd), hipMemcpyHostToDevice, st));
      ARK_CHECK_HIP(hipMemcpyAsync(s.pabc.p, abc.data(), ell * sizeof(G1), hipMemcpyHostToDevice, st));
      ARK_LAUNCH((on_curve_flags_kernel<Curve>), dim3((uint32_t)((3 * count + 127) / 128)), dim3(128), 0, st, (const G1*)d_ac,
                 2 * count, (const G2*)d_b, count, d_flags);
      ARK_CHECK_LAUNCH();
      if (m) {
        s.psc.ensure(count * m * sizeof(Fr));
        s.pprod.ensure(count * m * sizeof(XYZZ<Fq>));
        ARK_CHECK_HIP(hipMemcpyAsync(s.psc.p, inputs, count * m * sizeof(Fr), hipMemcpyHostToDevice, st));
        ARK_LAUNCH((prepared_input_terms_kernel<Curve>), dim3((uint32_t)((count * m + 127) / 128)), dim3(128), 0, st,
                   (const G1*)s.pabc.as<G1>(), (const Fr*)s.psc.as<Fr>(), count, m, s.pprod.as<XYZZ<Fq>>());
        ARK_CHECK_LAUNCH();
      }
      ARK_LAUNCH((verify_each_pairs_kernel<Curve>), dim3((uint32_t)((count + 127) / 128)), dim3(128), 0, st,
                 (const G1*)s.pabc.as<G1>(), (const XYZZ<Fq>*)s.pprod.as<XYZZ<Fq>>(), m, (const G1*)d_ac, (const G2*)d_b,
                 (const G2*)(d_b + 4 * count), (const uint8_t*)d_flags, count, d_ac + 2 * count, d_b + count, d_flags + 3 * count);
      ARK_CHECK_LAUNCH();
      groups_dev(d_ac + 2 * count, d_b + count, count, 3, target, d_flags + 3 * count, nullptr, ok);
    } else {
      each_host(abc.data(), m, gamma, delta, target, proofs, inputs, count, ok);
    }
    trace("verify_each", dev, 3 * count, t1 - t0, 0.0, now_ms() - t1, 0.0);
  }

  // Batch verification:
  // sum_j rho_j [ e(A_j, B_j) = e(alpha, beta) e(acc_j, gamma) e(C_j, delta) ]  <=>
  //   prod_j e(rho_j A_j, B_j) * e(-(sum rho_j) alpha, beta) * e(-sum_i (sum_j rho_j x_ji) gamma_abc_i, gamma)
  //                            * e(-sum_j rho_j C_j, delta) = 1
  // (k + 3 Miller loops and one final exponentiation for k proofs).  The two multi-scalar sums run on the device on both
  // routes: msm(bases, canonical scalars, n, out) is the caller's one-shot G1 MSM.  Three curve equations per proof (see
  // on_curve); a proof off its curve makes the batch false, it is not the caller's error.
  // Device route: the same three equations, rho_j A_j and the count + 3 Miller loops as kernels of pairing_impl.cuh; behind the
  // staged proofs s.pg1 has room for the count + 3 first arguments of the loops.
  template <class Msm>
  bool verify_batch(const ark355_vk_desc* vk, const ark355_proof_raw* proofs, const uint8_t* inputs, const uint8_t* rho,
                    uint64_t count, Msm&& msm) {
    const uint64_t ell = vk->num_instance;
    ARK_REQUIRE(ell >= 1 && count >= 1, ARK355_EINVAL, "empty batch or key");
    ARK_REQUIRE(rho || count == 1, ARK355_EINVAL, "a batch needs one random coefficient per proof");
    const bool dev = on_device(ctx->policy.pairing_device_min, count + 3);
    hipStream_t st = ctx->stream;
    const double t0 = now_ms();
    StagedProofs staged;
    if (dev) {
      staged = stage_proofs(proofs, count, 3 * count + 3, count + 3);
      if (on_curve_dev(s.pg1.p, 2 * count, s.pg2.p, count) != 0) return false;
    } else {
      for (uint64_t j = 0; j < count; j++)
        if (!on_curve(load_g1(proofs[j].a)) || !on_curve(load_g1(proofs[j].c)) || !on_curve(load_g2(proofs[j].b))) return false;
    }
    const double t1 = now_ms();
    std::vector<Fr> r(count), coef(ell, Fr::zero());
    for (uint64_t j = 0; j < count; j++) {
      if (rho) {
        Fr c;
        memcpy(c.l, rho + 32 * j, sizeof(Fr));
        r[j] = Fr::to_mont(c);
        ARK_REQUIRE(!r[j].is_zero(), ARK355_EINVAL, "zero random coefficient");
      } else {
        r[j] = Fr::one();
      }
      coef[0] = Fr::add(coef[0], r[j]);
      for (uint64_t i = 1; i < ell; i++) {
        Fr x;
        memcpy(x.l, inputs + ((size_t)j * (ell - 1) + (i - 1)) * sizeof(Fr), sizeof(Fr));
        coef[i] = Fr::add(coef[i], Fr::mul(r[j], x));
      }
    }
    // device MSMs over canonical scalars
    std::vector<uint8_t> sc(std::max<uint64_t>(ell, count) * sizeof(Fr)), cpts(count * sizeof(G1));
    G1 acc, csum;
    for (uint64_t i = 0; i < ell; i++) {
      const Fr c = Fr::from_mont(coef[i]);
      memcpy(sc.data() + i * sizeof(Fr), c.l, sizeof(Fr));
    }
    msm(vk->gamma_abc_g1, sc.data(), ell, &acc);
    for (uint64_t j = 0; j < count; j++) {
      const Fr c = Fr::from_mont(r[j]);
      memcpy(sc.data() + j * sizeof(Fr), c.l, sizeof(Fr));
      memcpy(cpts.data() + j * sizeof(G1), proofs[j].c, sizeof(G1));
    }
    msm(cpts.data(), sc.data(), count, &csum);
    std::vector<G1> Ps(count + 3);
    std::vector<G2> Qs(count + 3);
    const double t2 = now_ms();
    if (dev) {
      // rho_j A_j: one lane per proof, canonical rho_j (sc holds them since the second sum), into the slots after the C_j
      G1* dP = s.pg1.as<G1>() + 2 * count;
      if (rho) {
        s.psc.ensure(count * sizeof(Fr));
        ARK_CHECK_HIP(hipMemcpyAsync(s.psc.p, sc.data(), count * sizeof(Fr), hipMemcpyHostToDevice, st));
        ARK_LAUNCH((g1_scalar_mul_kernel<Curve>), dim3((uint32_t)((count + 127) / 128)), dim3(128), 0, st,
                   (const G1*)s.pg1.as<G1>(), (const Fr*)s.psc.as<Fr>(), count, dP);
        ARK_CHECK_LAUNCH();
      } else {
        ARK_CHECK_HIP(hipMemcpyAsync(dP, s.pg1.p, count * sizeof(G1), hipMemcpyDeviceToDevice, st));
      }
    } else {
      // rho_j A_j on host threads (one 255-bit scalar multiplication each)
      host_each(count, [&](uint64_t j) {
        const G1 a = load_g1(proofs[j].a);
        const Fr c = Fr::from_mont(r[j]);
        Ps[j] = rho ? xyzz_to_affine(xyzz_mul_scalar(XYZZ<Fq>::from_affine(a), c.l, Fr::N)) : a;
        Qs[j] = load_g2(proofs[j].b);
      });
    }
    const Fr s0 = Fr::from_mont(coef[0]);
    Ps[count] = G1::neg(xyzz_to_affine(xyzz_mul_scalar(XYZZ<Fq>::from_affine(load_g1(vk->alpha_g1)), s0.l, Fr::N)));
    Qs[count] = load_g2(vk->beta_g2);
    Ps[count + 1] = acc.is_inf() ? acc : G1::neg(acc);
    Qs[count + 1] = load_g2(vk->gamma_g2);
    Ps[count + 2] = csum.is_inf() ? csum : G1::neg(csum);
    Qs[count + 2] = load_g2(vk->delta_g2);
    if (dev) {
      ARK_CHECK_HIP(hipMemcpyAsync(s.pg1.as<G1>() + 3 * count, Ps.data() + count, 3 * sizeof(G1), hipMemcpyHostToDevice, st));
      ARK_CHECK_HIP(hipMemcpyAsync(s.pg2.as<G2>() + count, Qs.data() + count, 3 * sizeof(G2), hipMemcpyHostToDevice, st));
      ARK_CHECK_HIP(hipStreamSynchronize(st));
      const double t3 = now_ms();
      const Gt f = multi_miller_dev(s.pg1.as<G1>() + 2 * count, s.pg2.as<G2>(), count + 3);
      const double t4 = now_ms();
      const bool good = final_exp(f) == Gt::one();
      trace("verify_batch", true, count + 3, t1 - t0, t3 - t2, t4 - t3, now_ms() - t4);
      return good;
    }
    if (ctx->policy.trace_host)      // the host route reports the phases up to here only
      fprintf(stderr, "[ark355] verify_batch route=host pairs=%llu check_ms=%.3f scalar_mul_ms=%.3f\n",
              (unsigned long long)(count + 3), t1 - t0, now_ms() - t2);
    const Gt f = miller_product_host(Ps, Qs);
    return exponent_formed() && PH::final_exponentiation(f) == Gt::one();      // no exponent: never accept
  }

  // ---- the processed verifying key (SNARK::process_vk / verify_with_processed_vk, snark/src/lib.rs:36,69-80) ----------------
  // The per-key work of verify_each, once: the curve checks of the 4 + ell points (refused as verify_each refuses them),
  // e(alpha, beta) on the host (cold), gamma_abc into HBM and the P-independent lines of beta, gamma and delta
  // (pairing_key_lines_kernel).  A key point at infinity is legal: it gets no lines and its pairs contribute one.
  PvkDev* vk_process(const ark355_vk_desc* vk) {
    const uint64_t ell = vk->num_instance;
    ARK_REQUIRE(ell >= 1, ARK355_EINVAL, "empty key");
    ARK_REQUIRE(exponent_formed(), ARK355_EINVAL, "the final exponent could not be formed");
    const G1 alpha = load_g1(vk->alpha_g1);
    const G2 q[3] = {load_g2(vk->beta_g2), load_g2(vk->gamma_g2), load_g2(vk->delta_g2)};
    if (!on_curve(alpha)) refuse("vk.alpha_g1");
    if (!on_curve(q[0])) refuse("vk.beta_g2");
    if (!on_curve(q[1])) refuse("vk.gamma_g2");
    if (!on_curve(q[2])) refuse("vk.delta_g2");
    std::unique_ptr<PvkDev> d(new PvkDev());
    d->curve = Curve::ID;
    d->device = ctx->device;
    d->ell = ell;
    d->abc_host.assign(vk->gamma_abc_g1, vk->gamma_abc_g1 + ell * sizeof(G1));
    for (uint64_t i = 0; i < ell; i++)
      if (!on_curve(load_g1(d->abc_host.data() + i * sizeof(G1)))) refuse(at("vk.gamma_abc_g1", i));
    d->alpha.assign(vk->alpha_g1, vk->alpha_g1 + sizeof(G1));
    d->g2.resize(sizeof(q));
    memcpy(d->g2.data(), q, sizeof(q));
    for (int i = 0; i < 3; i++) d->inf[i] = q[i].is_inf();
    const Gt target = PH::final_exponentiation(PH::miller_loop(alpha, q[0]));
    d->alpha_beta.resize(sizeof(Gt));
    memcpy(d->alpha_beta.data(), &target, sizeof(Gt));
    const typename PD::Consts k = dev_consts();
    d->steps = k.steps;
    d->abc_bytes = ell * sizeof(G1);
    d->lines_bytes = (size_t)3 * k.steps * 3 * PD::W2 * sizeof(uint32_t);
    d->abc.alloc(d->abc_bytes);
    d->lines.alloc(d->lines_bytes);
    hipStream_t st = ctx->stream;
    DevBuf dq(sizeof(q));
    ARK_CHECK_HIP(hipMemcpyAsync(d->abc.p, d->abc_host.data(), d->abc_bytes, hipMemcpyHostToDevice, st));
    ARK_CHECK_HIP(hipMemcpyAsync(dq.p, q, sizeof(q), hipMemcpyHostToDevice, st));
    ARK_CHECK_HIP(hipMemsetAsync(d->lines.p, 0, d->lines_bytes, st));
    ARK_LAUNCH((pairing_key_lines_kernel<Curve>), dim3(1), dim3(PAIR_LANES), 0, st, (const G2*)dq.as<G2>(), 3u, k,
               d->lines.as<uint32_t>());
    ARK_CHECK_LAUNCH();
    ARK_CHECK_HIP(hipStreamSynchronize(st));
    return d.release();
  }

  static G2 pvk_point(const PvkDev& pvk, int which) { return load_g2(pvk.g2.data() + (size_t)which * sizeof(G2)); }
  static Gt pvk_target(const PvkDev& pvk) {
    Gt t;
    memcpy(&t, pvk.alpha_beta.data(), sizeof(Gt));
    return t;
  }
  // the lines of prepared point `which` (0 beta, 1 gamma, 2 delta); NULL where the point is at infinity
  static const uint32_t* pvk_lines(const PvkDev& pvk, int which) {
    return pvk.inf[which] ? nullptr : pvk.lines.as<uint32_t>() + (size_t)which * pvk.steps * 3 * PD::W2;
  }
  void pvk_usable(const PvkDev& pvk) const {
    ARK_REQUIRE(pvk.device == ctx->device, ARK355_EINVAL, "the processed key is resident on another device than this context's");
  }

  // ark-ec Pairing::pairing against one G2Prepared: GT_i = e(P_i, Q_which), byte for byte ark355_pairing_groups' value
  void pvk_pairings(const PvkDev& pvk, int which, const uint8_t* g1, uint64_t n, uint8_t* out_gt, uint8_t* is_one) {
    pvk_usable(pvk);
    ARK_REQUIRE(which >= 0 && which <= 2, ARK355_EINVAL, "which must be 0 (beta), 1 (gamma) or 2 (delta)");
    if (n == 0) return;
    ARK_REQUIRE(n <= 0xFFFFFFFFull, ARK355_EINVAL, "n must stay below 2^32");
    ARK_REQUIRE(g1, ARK355_EINVAL, "a point array is NULL");
    const bool dev = on_device(ctx->policy.pairing_each_min, n);
    const double t0 = now_ms();
    double t1 = t0;
    std::vector<uint8_t> verdict(n);
    if (dev) {
      hipStream_t st = ctx->stream;
      s.pg1.ensure(n * sizeof(G1));
      ARK_CHECK_HIP(hipMemcpyAsync(s.pg1.p, g1, n * sizeof(G1), hipMemcpyHostToDevice, st));
      if (const unsigned long long e = on_curve_dev(s.pg1.p, n, nullptr, 0)) refuse_word(e);
      t1 = now_ms();
      const FeDev fe = fe_upload(Gt::one());
      const typename PD::Consts k = dev_consts();
      const uint32_t stride = (uint32_t)((std::min(n, PVK_PAIR_CHUNK) + PAIR_LANES - 1) / PAIR_LANES * PAIR_LANES);
      s.pkmill.ensure((size_t)PD::W12 * stride * sizeof(uint32_t));
      if (out_gt) s.pgt.ensure(n * PD::W12 * sizeof(uint32_t));
      s.pverd.ensure(n);
      for (uint64_t off = 0; off < n; off += PVK_PAIR_CHUNK) {
        const uint32_t m = (uint32_t)std::min(PVK_PAIR_CHUNK, n - off);
        const uint32_t blocks = (m + PAIR_LANES - 1) / PAIR_LANES;
        ARK_LAUNCH((pairing_accumulate_key_kernel<Curve>), dim3(blocks), dim3(PAIR_LANES), 0, st, (const G1*)s.pg1.as<G1>() + off, m,
                   pvk_lines(pvk, which), (const G1*)nullptr, 0u, (const uint32_t*)nullptr, blocks, stride, 1u, 0u, 0u, k,
                   s.pkmill.as<uint32_t>());
        ARK_CHECK_LAUNCH();
        fe_launch(fe, s.pkmill.as<uint32_t>(), stride, off, m, 1, nullptr, out_gt != nullptr);
      }
      fe_download(n, out_gt, verdict.data());
    } else {
      for (uint64_t i = 0; i < n; i++)
        if (!on_curve(load_g1(g1 + i * sizeof(G1)))) refuse(at("g1", i));
      t1 = now_ms();
      const G2 Q = pvk_point(pvk, which);
      host_each(n, [&](uint64_t i) {
        const Gt gt = PH::final_exponentiation(PH::miller_loop(load_g1(g1 + i * sizeof(G1)), Q));
        if (out_gt) memcpy(out_gt + i * sizeof(Gt), &gt, sizeof(gt));
        verdict[i] = gt == Gt::one() ? 1 : 0;
      });
    }
    if (is_one) memcpy(is_one, verdict.data(), n);
    trace("pvk_pairings", dev, n, t1 - t0, 0.0, now_ms() - t1, 0.0);
  }

  // The device route of ark355_verify_each_pvk and ark355_verify_each_bytes from the staged proofs on (s.pg1 = A_j, C_j with
  // room for 4 count points, s.pg2 = B_j): curve flags, prepared inputs, the pairs against gamma and delta, the chunked Miller
  // stage, one final exponentiation per proof.  d_pst: the per-point statuses of proof_decode_kernel (NULL: the proofs came as
  // points); a proof that failed to decode is marked bad like one off its curve, and s.pstatus receives the per-proof statuses.
  void each_pvk_staged(const PvkDev& pvk, const uint8_t* inputs, uint64_t count, const uint8_t* d_pst, uint8_t* ok) {
    hipStream_t st = ctx->stream;
    const uint32_t m = (uint32_t)(pvk.ell - 1);
    const Gt target = pvk_target(pvk);
    s.pflags.ensure(4 * count);
    G1* d_ac = s.pg1.as<G1>();
    G2* d_b = s.pg2.as<G2>();
    G1* d_nacc = d_ac + 2 * count;
    G1* d_negc = d_ac + 3 * count;
    uint8_t* d_flags = s.pflags.as<uint8_t>();
    const G1* d_abc = pvk.abc.as<G1>();
    ARK_LAUNCH((on_curve_flags_kernel<Curve>), dim3((uint32_t)((3 * count + 127) / 128)), dim3(128), 0, st, (const G1*)d_ac,
               2 * count, (const G2*)d_b, count, d_flags);
    ARK_CHECK_LAUNCH();
    if (d_pst) {
      s.pstatus.ensure(count);
      ARK_LAUNCH((proof_status_kernel<Curve>), dim3((uint32_t)((count + 127) / 128)), dim3(128), 0, st, d_pst, count, s.pstatus.as<uint8_t>(),
                 d_flags);
      ARK_CHECK_LAUNCH();
    }
    if (m) {
      s.psc.ensure(count * m * sizeof(Fr));
      s.pprod.ensure(count * m * sizeof(XYZZ<Fq>));
      ARK_CHECK_HIP(hipMemcpyAsync(s.psc.p, inputs, count * m * sizeof(Fr), hipMemcpyHostToDevice, st));
      ARK_LAUNCH((prepared_input_terms_kernel<Curve>), dim3((uint32_t)((count * m + 127) / 128)), dim3(128), 0, st, d_abc,
                 (const Fr*)s.psc.as<Fr>(), count, m, s.pprod.as<XYZZ<Fq>>());
      ARK_CHECK_LAUNCH();
    }
    ARK_LAUNCH((verify_each_key_pairs_kernel<Curve>), dim3((uint32_t)((count + 127) / 128)), dim3(128), 0, st, d_abc,
               (const XYZZ<Fq>*)s.pprod.as<XYZZ<Fq>>(), m, (const G1*)d_ac, (const uint8_t*)d_flags, count, d_nacc, d_negc,
               d_flags + 3 * count);
    ARK_CHECK_LAUNCH();
    const FeDev fe = fe_upload(target);
    const typename PD::Consts k = dev_consts();
    s.pverd.ensure(count);
    const uint32_t* lg = pvk_lines(pvk, 1);
    const uint32_t* ld = pvk_lines(pvk, 2);
    miller_chunks<true>(d_ac, d_b, count, PVK_EACH_CHUNK, [&](uint64_t off, uint32_t n, uint32_t stride) {
      // the group layout of the chunk: proof j of it at 3 j .. 3 j + 2 of a row of 3 * stride
      const uint32_t row = 3 * stride, blocks = (n + PAIR_LANES - 1) / PAIR_LANES;
      s.pkmill.ensure((size_t)PD::W12 * row * sizeof(uint32_t));
      ARK_LAUNCH((miller_spread_kernel<Curve>), dim3((n + 255) / 256), dim3(256), 0, st, (const uint32_t*)s.pmill.as<uint32_t>(),
                 stride, n, row, 3u, s.pkmill.as<uint32_t>());
      ARK_CHECK_LAUNCH();
      ARK_LAUNCH((pairing_accumulate_key_kernel<Curve>), dim3(2 * blocks), dim3(PAIR_LANES), 0, st, (const G1*)d_nacc + off, n, lg,
                 (const G1*)d_negc + off, n, ld, blocks, row, 3u, 1u, 2u, k, s.pkmill.as<uint32_t>());
      ARK_CHECK_LAUNCH();
      fe_launch(fe, s.pkmill.as<uint32_t>(), row, off, n, 3, d_flags + 3 * count, false);
    });
    fe_download(count, nullptr, ok);
  }

  // SNARK::verify_with_processed_vk for every proof on its own: verify_each without the per-key work.  Device route: pass A
  // and the per-pair pass B over the count pairs (A_j, B_j) only; the 2 count pairs (-acc_j, gamma), (-C_j, delta) go through
  // pairing_accumulate_key_kernel against the handle's lines; one final exponentiation per proof over its three Miller values.
  void verify_each_pvk(const PvkDev& pvk, const ark355_proof_raw* proofs, const uint8_t* inputs, uint64_t count, uint8_t* ok) {
    pvk_usable(pvk);
    const uint64_t ell = pvk.ell;
    if (count == 0) return;
    ARK_REQUIRE(ell == 1 || inputs, ARK355_EINVAL, "public_inputs is NULL");
    ARK_REQUIRE(count <= 0xFFFFFFFFull / 3, ARK355_EINVAL, "3 * count must stay below 2^32");
    const double t0 = now_ms();
    const bool dev = on_device(ctx->policy.pairing_each_min, count);
    if (dev) {
      // behind the staged proofs: s.pg1 the -acc_j and the -C_j
      const StagedProofs staged = stage_proofs(proofs, count, 4 * count, count);
      each_pvk_staged(pvk, inputs, count, nullptr, ok);
    } else {
      each_host(reinterpret_cast<const G1*>(pvk.abc_host.data()), (uint32_t)(ell - 1), pvk_point(pvk, 1), pvk_point(pvk, 2),
                pvk_target(pvk), proofs, inputs, count, ok);
    }
    trace("verify_each_pvk", dev, 3 * count, 0.0, 0.0, now_ms() - t0, 0.0);
  }

  // ---- proofs as wire bytes (Proof: CanonicalDeserialize, snark/src/lib.rs:32) ---------------------------------------------
  // The arguments of the three entries are checked once, in capi.hip (ARK355_EINVAL names the argument).
  static size_t proof_size(bool compressed) { return 2 * W::g1_size(compressed) + W::g2_size(compressed); }
  // upload + proof_decode_kernel: s.pg1 / s.pg2 staged as stage_proofs leaves them (room for cap1 G1 points), s.ppst the
  // per-point statuses.  Nothing is synchronised: `in` must stay alive until the caller has.
  void decode_proofs_dev(const uint8_t* in, uint64_t count, bool compressed, int validate, uint64_t cap1) {
    hipStream_t st = ctx->stream;
    s.pbytes.ensure(count * proof_size(compressed));
    s.pg1.ensure(cap1 * sizeof(G1));
    s.pg2.ensure(count * sizeof(G2));
    s.ppst.ensure(3 * count);
    ARK_CHECK_HIP(hipMemcpyAsync(s.pbytes.p, in, count * proof_size(compressed), hipMemcpyHostToDevice, st));
    const uint32_t blocks1 = (uint32_t)((2 * count + 127) / 128), blocks2 = (uint32_t)((count + 127) / 128);
    ARK_LAUNCH((proof_decode_kernel<Curve>), dim3(blocks1 + blocks2), dim3(128), 0, st, (const uint8_t*)s.pbytes.as<uint8_t>(), count,
               compressed ? 1 : 0, validate, blocks1, s.pg1.as<G1>(), s.pg2.as<G2>(), s.ppst.as<uint8_t>());
    ARK_CHECK_LAUNCH();
  }
  // one proof on the host, the same verdict as the kernels': (k << 4) | status of the first failing point, out zero then
  static uint8_t decode_proof_host(const uint8_t* in, bool compressed, int validate, ark355_proof_raw* out) {
    const size_t s1 = W::g1_size(compressed), s2 = W::g2_size(compressed);
    G1 a = G1::inf(), c = G1::inf();
    G2 b = G2::inf();
    uint8_t st = 0;                                    // the first failing point decides: nothing behind it is decoded
    if (const int sa = W::g1_decode(in, compressed, validate, &a)) st = (uint8_t)(0x10 | sa);
    else if (const int sb = W::g2_decode(in + s1, compressed, validate, &b)) st = (uint8_t)(0x20 | sb);
    else if (const int sc = W::g1_decode(in + s1 + s2, compressed, validate, &c)) st = (uint8_t)(0x30 | sc);
    memset(out, 0, sizeof(*out));
    if (st == 0) {
      memcpy(out->a, &a, sizeof(a));
      memcpy(out->b, &b, sizeof(b));
      memcpy(out->c, &c, sizeof(c));
    }
    return st;
  }

  // `count` proofs decoded on the device: the raw images and one status per proof; a bad proof is no error of the call
  void proofs_from_bytes(const uint8_t* in, uint64_t count, bool compressed, int validate, ark355_proof_raw* out, uint8_t* status) {
    if (count == 0) return;
    hipStream_t st = ctx->stream;
    decode_proofs_dev(in, count, compressed, validate, 2 * count);
    s.pstatus.ensure(count);
    ARK_LAUNCH((proof_status_kernel<Curve>), dim3((uint32_t)((count + 127) / 128)), dim3(128), 0, st, (const uint8_t*)s.ppst.as<uint8_t>(),
               count, s.pstatus.as<uint8_t>(), (uint8_t*)nullptr);
    ARK_CHECK_LAUNCH();
    std::vector<G1> ac(2 * count);
    std::vector<G2> bs(count);
    ARK_CHECK_HIP(hipMemcpyAsync(ac.data(), s.pg1.p, 2 * count * sizeof(G1), hipMemcpyDeviceToHost, st));
    ARK_CHECK_HIP(hipMemcpyAsync(bs.data(), s.pg2.p, count * sizeof(G2), hipMemcpyDeviceToHost, st));
    ARK_CHECK_HIP(hipMemcpyAsync(status, s.pstatus.p, count, hipMemcpyDeviceToHost, st));
    ARK_CHECK_HIP(hipStreamSynchronize(st));
    memset(out, 0, count * sizeof(*out));
    for (uint64_t j = 0; j < count; j++) {
      if (status[j]) continue;
      memcpy(out[j].a, &ac[j], sizeof(G1));
      memcpy(out[j].b, &bs[j], sizeof(G2));
      memcpy(out[j].c, &ac[count + j], sizeof(G1));
    }
  }

  // Proof::deserialize_with_mode + verify_with_processed_vk per proof.  Device route: the bytes are decoded where the
  // verifier reads its points (proof_decode_kernel), then the stages of ark355_verify_each_pvk; host route: decode_proof_host
  // and each_host on host threads.  Both give the same ok and status.
  void verify_each_bytes(const PvkDev& pvk, const uint8_t* in, uint64_t count, bool compressed, int validate, const uint8_t* inputs,
                         uint8_t* ok, uint8_t* status) {
    pvk_usable(pvk);
    if (count == 0) return;
    ARK_REQUIRE(pvk.ell == 1 || inputs, ARK355_EINVAL, "public_inputs is NULL");
    const double t0 = now_ms();
    double t1 = t0;
    const bool dev = on_device(ctx->policy.pairing_each_min, count);
    if (dev) {
      decode_proofs_dev(in, count, compressed, validate, 4 * count);
      if (ctx->policy.trace_host) {                       // the decode stage alone, for the trace only
        ARK_CHECK_HIP(hipStreamSynchronize(ctx->stream));
        t1 = now_ms();
      }
      each_pvk_staged(pvk, inputs, count, s.ppst.as<uint8_t>(), ok);
      if (status) {
        ARK_CHECK_HIP(hipMemcpyAsync(status, s.pstatus.p, count, hipMemcpyDeviceToHost, ctx->stream));
        ARK_CHECK_HIP(hipStreamSynchronize(ctx->stream));
      }
    } else {
      std::vector<ark355_proof_raw> proofs(count);
      std::vector<uint8_t> stv(count);
      const size_t sp = proof_size(compressed);
      host_each(count, [&](uint64_t j) { stv[j] = decode_proof_host(in + j * sp, compressed, validate, &proofs[j]); });
      t1 = now_ms();
      each_host(reinterpret_cast<const G1*>(pvk.abc_host.data()), (uint32_t)(pvk.ell - 1), pvk_point(pvk, 1), pvk_point(pvk, 2),
                pvk_target(pvk), proofs.data(), inputs, count, ok);
      for (uint64_t j = 0; j < count; j++)
        if (stv[j]) ok[j] = 0;
      if (status) memcpy(status, stv.data(), count);
    }
    trace("verify_each_bytes", dev, 3 * count, t1 - t0, 0.0, now_ms() - t1, 0.0);
  }

  // is_on_curve + is_in_correct_subgroup_assuming_on_curve of n raw images, always on the device (the two subgroup tests are
  // compared where they run)
  void points_check(int group, const uint8_t* raw, uint64_t n, int method, uint8_t* status) {
    if (n == 0) return;
    hipStream_t st = ctx->stream;
    const size_t bytes = n * (group == 1 ? sizeof(G1) : sizeof(G2));
    s.pbytes.ensure(bytes);
    s.ppst.ensure(n);
    ARK_CHECK_HIP(hipMemcpyAsync(s.pbytes.p, raw, bytes, hipMemcpyHostToDevice, st));
    const dim3 grid((uint32_t)((n + 127) / 128));
    if (group == 1)
      ARK_LAUNCH((points_check_kernel<Curve, 1>), grid, dim3(128), 0, st, (const void*)s.pbytes.p, n, method, s.ppst.as<uint8_t>());
    else
      ARK_LAUNCH((points_check_kernel<Curve, 2>), grid, dim3(128), 0, st, (const void*)s.pbytes.p, n, method, s.ppst.as<uint8_t>());
    ARK_CHECK_LAUNCH();
    ARK_CHECK_HIP(hipMemcpyAsync(status, s.ppst.p, n, hipMemcpyDeviceToHost, st));
    ARK_CHECK_HIP(hipStreamSynchronize(st));
  }

  // ark355_verify_batch over the handle's copies of the key (unchecked, as ark355_verify_batch leaves the key unchecked)
  template <class Msm>
  bool verify_batch_pvk(const PvkDev& pvk, const ark355_proof_raw* proofs, const uint8_t* inputs, const uint8_t* rho, uint64_t count,
                        Msm&& msm) {
    pvk_usable(pvk);
    ark355_vk_desc vk{};
    vk.num_instance = pvk.ell;
    vk.alpha_g1 = pvk.alpha.data();
    vk.beta_g2 = pvk.g2.data();
    vk.gamma_g2 = pvk.g2.data() + sizeof(G2);
    vk.delta_g2 = pvk.g2.data() + 2 * sizeof(G2);
    vk.gamma_abc_g1 = pvk.abc_host.data();
    return verify_batch(&vk, proofs, inputs, rho, count, msm);
  }
};

}  // namespace ark355
