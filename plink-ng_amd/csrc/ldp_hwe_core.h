// ldp_hwe_core.h -- the exact Hardy-Weinberg test of one variant's genotype counts, as ONE piece of arithmetic for the device
// (hwe_kernel, ldp_hwe.hip) and the host (ldp_hwe_ln_p_host, ldp_hwe_host.cpp).  DESIGN.md section 4.2g has the derivation of the
// accuracy bound and the tie rule.
//
// Counts (hom1, het, hom2), n = hom1 + het + hom2 < 2^31, rare = 2 * min(hom1, hom2) + het.  Conditional on n and rare the het count
// k has weight w(k) = 2^k n! / (r! k! c!), r = (rare - k) / 2 the rarer homozygote's count, c = n - k - r the other's; the p-value is
// the weight of every table no likelier than the observed one over the weight of all tables, `midp` taking half of the tables that
// tie with the observed one off the numerator.
//
// The walk starts at the observed table with relative weight 1 and goes up (k + 2: times 4 r c / ((k + 2)(k + 1))) and down (k - 2:
// times k (k - 1) / (4 (r + 1)(c + 1))), r steps up and het / 2 steps down at most: both loops count an integer, whatever the
// floating-point values do.  A value is kept as m * S^e, S = 2^256, 1 <= m < S (one exact multiplication by S or 1 / S restores that
// after a step, a step's factor lying in [2^-62, 2^61]); a direction ends early once its value is below 2^-100 (below_cutoff).
// Plain IEEE double *, /, + and one log; the build has -ffp-contract=off.
#ifndef LDP_HWE_CORE_H
#define LDP_HWE_CORE_H
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LDP_HWE_HD __host__ __device__ inline
#else
#define LDP_HWE_HD inline
#endif

namespace ldp_hwe {

constexpr double kScale = 0x1p256;  // S
constexpr double kScaleInv = 0x1p-256, kScaleInv2 = 0x1p-512, kScaleInv3 = 0x1p-768;
constexpr double kLnScale = 256.0 * 0.693147180559945309417;  // ln S
constexpr double kTwoPowM52 = 0x1p-52;
constexpr uint8_t kFlagToleranceTie = 1;  // a table other than the observed one's neighbours came within the tolerance of the observed weight

// the two sums of the walk: terms no likelier than the observed table (scale 0: the observed table's own 1 is among them), the terms
// that tie with it, and all terms as tm * S^te
struct Sums {
  double tail, ties, tm;
  int32_t te;
  uint8_t flags;
};

// S^e for -3 <= e <= 0 (the sums' scales meet within that range; a term that reaches add_term has e >= -1)
LDP_HWE_HD double scale_down(int32_t e) { return (e == 0) ? 1.0 : ((e == -1) ? kScaleInv : ((e == -2) ? kScaleInv2 : kScaleInv3)); }

// a value below 2^-100: a direction ends there.  It is below 1, so the walk is past the mode on that side and the terms behind it only fall
// (the weights are log-concave in k); fewer than 2^30 of them remain, together below 2^-70 of the observed table's own term, which both sums hold
LDP_HWE_HD bool below_cutoff(double m, int32_t e) { return (e < -1) || ((e == -1) && (m < 0x1p156)); }

// one term m * S^e (1 <= m < S), `steps` steps away from the observed table; exact_cmp: -1 / 0 / 1 = it is below / ties with / is
// above the observed weight by the integer test (the observed table's neighbours), 2 = compare the value
LDP_HWE_HD void add_term(Sums* s, double m, int32_t e, uint32_t steps, int exact_cmp) {
  // all terms, at the larger of the two scales (a term or a sum 4 powers of S below the other is below its last bit many times over)
  if (e > s->te) {
    const int32_t d = s->te - e;
    s->tm = (d >= -3) ? (s->tm * scale_down(d)) : 0.0;
    s->te = e;
  }
  if (e - s->te >= -3) {
    s->tm += m * scale_down(e - s->te);
  }
  bool le, tie;
  if (exact_cmp != 2) {
    le = exact_cmp <= 0;
    tie = exact_cmp == 0;
  } else {
    // a value within 4 * steps * 2^-52 of 1 (more than its own rounding error after that many steps) counts as a tie
    const double tol = 4.0 * static_cast<double>(steps) * kTwoPowM52;
    if (e == 0) {
      le = m <= 1.0 + tol;
      tie = le;
    } else if (e == -1) {
      le = true;
      tie = m * kScaleInv >= 1.0 - tol;
    } else {
      le = e < 0;
      tie = false;
    }
    if (tie) {
      s->flags |= kFlagToleranceTie;
    }
  }
  if (le && (e >= -3)) {
    const double v = m * scale_down(e);
    s->tail += v;
    if (tie) {
      s->ties += v;
    }
  }
}

// ln of the p-value; *flags_out (may be null): kFlagToleranceTie.  hom1 + het + hom2 < 2^31 is the caller's to check.
LDP_HWE_HD double ln_p(uint32_t hom1, uint32_t het, uint32_t hom2, int midp, uint8_t* flags_out) {
  const uint32_t r0 = (hom1 < hom2) ? hom1 : hom2;
  const uint32_t c0 = (hom1 < hom2) ? hom2 : hom1;
  Sums s;
  s.tail = 1.0;
  s.ties = 1.0;
  s.tm = 1.0;
  s.te = 0;
  s.flags = 0;
  // up: r0 steps at most
  {
    double m = 1.0;
    int32_t e = 0;
    uint32_t r = r0, c = c0, k = het;
    for (uint32_t step = 1; step <= r0; ++step) {
      const uint64_t num_i = 4ull * r * static_cast<uint64_t>(c);
      const uint64_t den_i = (static_cast<uint64_t>(k) + 2) * (static_cast<uint64_t>(k) + 1);
      m = m * (static_cast<double>(num_i) / static_cast<double>(den_i));
      if (m >= kScale) {
        m *= kScaleInv;
        ++e;
      } else if (m < 1.0) {
        m *= kScale;
        --e;
      }
      if (below_cutoff(m, e)) {
        break;
      }
      add_term(&s, m, e, step, (step == 1) ? ((num_i < den_i) ? -1 : ((num_i == den_i) ? 0 : 1)) : 2);
      --r;
      --c;
      k += 2;
    }
  }
  // down: het / 2 steps at most
  {
    double m = 1.0;
    int32_t e = 0;
    uint32_t r = r0, c = c0, k = het;
    const uint32_t down_ct = het >> 1;
    for (uint32_t step = 1; step <= down_ct; ++step) {
      const uint64_t num_i = static_cast<uint64_t>(k) * (k - 1);
      const uint64_t den_i = 4ull * (static_cast<uint64_t>(r) + 1) * (static_cast<uint64_t>(c) + 1);
      m = m * (static_cast<double>(num_i) / static_cast<double>(den_i));
      if (m >= kScale) {
        m *= kScaleInv;
        ++e;
      } else if (m < 1.0) {
        m *= kScale;
        --e;
      }
      if (below_cutoff(m, e)) {
        break;
      }
      add_term(&s, m, e, step, (step == 1) ? ((num_i < den_i) ? -1 : ((num_i == den_i) ? 0 : 1)) : 2);
      ++r;
      ++c;
      k -= 2;
    }
  }
  if (flags_out) {
    *flags_out = s.flags;
  }
  const double tail = midp ? (s.tail - 0.5 * s.ties) : s.tail;
  const double lnq = log(tail / s.tm);
  return s.te ? (lnq - static_cast<double>(s.te) * kLnScale) : lnq;
}

}  // namespace ldp_hwe
#endif
