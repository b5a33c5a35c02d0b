// ldp_phased_ld.cpp -- the floating-point tail of --r2-phased / --r-phased on the HOST: haplotype-frequency r^2, D and D' of a pair
// from the five integers the device produces (ldp_phased_stats_t, include/ldprune_hip.h).
//
// The statistic is the maximum-likelihood haplotype-frequency estimate of two biallelic loci.  With n jointly called samples, a / b
// the counted-allele sums of the two variants over them, k the haplotypes known to carry both counted alleles and u the samples
// heterozygous at both variants without phase information, everything is in units of t = 1 / (2 n):
//     f22 = k t                  both counted alleles
//     f21 = (a - k - u) t        counted allele of the first variant only
//     f12 = (b - k - u) t        ... of the second only
//     f11 = 1 - (a + b - k) t    neither
//     K   = u t                  the share of the unphased double heterozygotes: each of them is either (11 + 22) or (12 + 21)
// The likelihood of x = the part of K that is (11 + 22) has its stationary points where
//     (f11 + x)(f22 + x)(K - x) = x (f12 + K - x)(f21 + K - x),
// a cubic in x.  The work is cut the way the problem is: haplotype_freqs() makes the frequencies, candidate_splits() returns the
// stationary points that count, already confined to [0, K] (cubic_stationary_points() solves the cubic, distinct() merges
// coincident roots), likeliest_split() picks one, and phased_pair() turns it into D, r^2 and D'.
//
// What is NOT free is the arithmetic: the table prints six significant digits of doubles that went through log, acos, cos and cbrt,
// and a threshold decides on the last bit, so every double is produced by the operations, in the association, that the reference's
// PhasedLD / CubicRealRoots / EmPhaseUnscaledLnlike use (plink2_ld.cc:4573-4765, plink2_cmdline.cc:2384-2458; each expression below
// cites its line), on the host's libm.  The library is built with -ffp-contract=off, as the reference is; fma() stands exactly where
// the reference asks for a fused multiply-add by name (its prefer_fma is fma() in a build with -mfma, plink2_float.h:202) and
// nowhere else.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/ldprune_hip.h"

namespace {

constexpr double kMergeGap = 1.0 / (1LL << 30);   // roots closer than this are one root (plink2_float.h:118)
constexpr double kClipBand = 1.0 / (1LL << 32);   // a root this close to 0 or K is 0 or K (plink2_ld.cc:4665-4681)
constexpr double kLinearGap = 1.0 / (1LL << 35);  // (:4699)
constexpr double kZeroD = 1.0 / (1LL << 44);      // |D| below this is 0 (:4732)
constexpr double kMonomorphic = kZeroD * 0.125;   // an allele frequency below 2^-47 (:4644)
constexpr double kPi = 3.1415926535897932;

struct Roots {
  double x[3];
  int n;
};

// ascending, and of roots closer than kMergeGap to the last one kept only the first stays: the two- and three-root endings of
// plink2_cmdline.cc:2403, :2451-2457 are this rule (s1 against s0, then s2 against whichever of them was kept last)
Roots distinct(Roots r) {
  for (int a = 1; a < r.n; ++a) {  // (three values at most: insertion sort)
    for (int b = a; (b > 0) && (r.x[b - 1] > r.x[b]); --b) {
      std::swap(r.x[b - 1], r.x[b]);
    }
  }
  Roots out;
  out.n = 0;
  for (int a = 0; a < r.n; ++a) {
    if ((out.n == 0) || !(r.x[a] - out.x[out.n - 1] < kMergeGap)) {
      out.x[out.n++] = r.x[a];
    }
  }
  return out;
}

// Real roots of x^3 + A x^2 + B x + C.  With q = A^2 - 3 B and r = 2 A^3 - 9 A B + 27 C (9 Q and 54 R of the textbook) the sign of
// r^2 - 4 q^3 separates one real root (Cardano) from three (Viete's cosines), equality being the double root.
Roots cubic_stationary_points(double A, double B, double C) {
  const double AA = A * A;                               // plink2_cmdline.cc:2385
  const double q = AA - 3 * B;                           // :2386
  const double r = AA * (2 * A) + 27 * C - 9 * A * B;    // :2387
  const double lhs = r * r, rhs = q * q * (4 * q);       // :2388-2389
  const double centre = A * (1.0 / 3.0);                 // :2390: the roots of the depressed cubic are shifted by -A / 3
  Roots out;
  if (lhs > rhs) {
    // one real root: the cube root of |R| + sqrt(R^2 - Q^3) with the sign opposite to R, plus Q over it (:2414-2422)
    const double Q = q * (1.0 / 9.0), R = r * (1.0 / 54.0);
    const double u = ((r >= 0) ? -1 : 1) * cbrt(fma(sqrt(lhs - rhs), 1.0 / 54.0, fabs(R)));
    out.x[0] = u + Q / u - centre;
    out.n = 1;
    return out;
  }
  if (lhs == rhs) {
    // a double root and a simple one, at -2 s and s or at -s and 2 s around the centre, s = sqrt(q) / 3 (:2394-2401)
    const double s = (1.0 / 3.0) * sqrt(q);
    const bool simple_below = r > 0.0;
    out.x[0] = (simple_below ? (-2 * s) : (-s)) - centre;
    out.x[1] = (simple_below ? s : (2 * s)) - centre;
    out.n = 2;
    return distinct(out);
  }
  // three real roots: -2 sqrt(Q) cos((theta + 2 pi k) / 3) with cos(theta) = R / Q^(3/2) (:2405-2432)
  const double Q = q * (1.0 / 9.0), R = r * (1.0 / 54.0);
  const double sq = sqrt(Q);
  const double third = acos(R / (sq * Q)) * (1.0 / 3.0);
  const double amp = -2 * sq;
  const double turn[3] = {0.0, 2.0 * kPi / 3.0, -(2.0 * kPi / 3.0)};
  for (int k = 0; k < 3; ++k) {
    out.x[k] = fma(amp, cos(third + turn[k]), -centre);
  }
  out.n = 3;
  return distinct(out);
}

struct Freqs {
  double f11, f12, f21, f22, K;
  double p1, p2, q1, q2;  // allele frequencies: first variant "neither" / counted, second variant likewise
  bool defined;
};

Freqs haplotype_freqs(const ldp_phased_stats_t& s) {
  Freqs F = {};
  if (!s.valid_obs) {
    return F;  // no joint sample (plink2_ld.cc:6708)
  }
  const double a = static_cast<double>(s.sum0), b = static_cast<double>(s.sum1);
  const double k = static_cast<double>(s.known_dotprod), u = static_cast<double>(s.unknown_hethet);
  const double t = 0.5 / static_cast<double>(s.valid_obs);  // :6711
  F.f11 = fmax(fma(a + b - k, -t, 1.0), 0.0);               // :4633 (never below zero)
  F.f12 = (b - k - u) * t;                                  // :4634
  F.f21 = (a - k - u) * t;                                  // :4635
  F.f22 = k * t;                                            // :4636
  F.K = u * t;                                              // :4637
  F.p1 = F.f11 + F.f12 + F.K;                               // :4638-4641
  F.p2 = 1.0 - F.p1;
  F.q1 = F.f11 + F.f21 + F.K;
  F.q2 = 1.0 - F.q1;
  // a variant without variation over the joint samples has no LD with anything (:4644-4649)
  F.defined = !((F.p1 < kMonomorphic) || (F.p2 < kMonomorphic) || (F.q1 < kMonomorphic) || (F.q2 < kMonomorphic));
  return F;
}

// The splits x in [0, K] at which the likelihood can peak, ascending.
Roots candidate_splits(const Freqs& F) {
  Roots c;
  c.x[0] = 0.0;
  c.n = 1;
  if (F.K == 0.0) {
    return c;  // nothing to split (:4722)
  }
  const double same = F.f11 * F.f22, cross = F.f12 * F.f21;
  if ((same == 0.0) && (cross == 0.0)) {
    // One of {f11, f22} and one of {f12, f21} vanish: the cubic factors into x (K - x) (linear), so 0 and K always are stationary and
    // the linear factor adds (K + (f12 + f21) - (f11 + f22)) / 2 when that lies strictly between them (:4695-4706).
    const double diag = F.f11 + F.f22, anti = F.f12 + F.f21;
    if ((diag + kLinearGap < F.K + anti) && (anti + kLinearGap < F.K + diag)) {
      c.x[c.n++] = (F.K + anti - diag) * 0.5;
    }
    c.x[c.n++] = F.K;
    return c;
  }
  // the cubic, halved: x^3 + A x^2 + B x + C with the coefficients as :4662 forms them
  const double A = 0.5 * (F.f11 + F.f22 - F.f12 - fma(3, F.K, F.f21));
  const double B = 0.5 * fma(F.K, F.f12 + F.f21 - (F.f11 + F.f22) + F.K, same + cross);
  const double C = -0.5 * F.K * F.f11 * F.f22;
  const Roots r = cubic_stationary_points(A, B, C);
  // confine to [0, K]: roots beyond K + band and below -band are no splits -- but the last root standing is never discarded --, and
  // what lands within the band of an end IS that end (:4663-4682; a lone root is only ever raised to 0, :4678-4682)
  int lo = 0, hi = r.n;
  Roots keep = r;
  if (r.n > 1) {
    while ((hi > 1) && (keep.x[hi - 1] > F.K + kClipBand)) {
      --hi;
    }
    if (keep.x[hi - 1] > F.K - kClipBand) {
      keep.x[hi - 1] = F.K;
    }
    while ((lo + 1 < hi) && (keep.x[lo] < -kClipBand)) {
      ++lo;
    }
  }
  if (keep.x[lo] < kClipBand) {
    keep.x[lo] = 0.0;
  }
  c.n = 0;
  for (int a = lo; a < hi; ++a) {
    c.x[c.n++] = keep.x[a];
  }
  return c;
}

// log-likelihood per allele of the split x (:4573-4598): K log(g12 g21 + g11 g22) for the unphased double heterozygotes plus
// f log(g) for each known haplotype class, g = the class's frequency under the split; empty classes add nothing.
double split_lnlike(const Freqs& F, double x) {
  const double g11 = F.f11 + x, g22 = F.f22 + x;                  // :4576-4577
  const double g12 = F.f12 + F.K - x, g21 = F.f21 + F.K - x;      // :4578-4579
  const double both = fma(g12, g21, g11 * g22);                   // :4580
  double ll = (both != 0.0) ? (F.K * log(both)) : 0.0;            // :4583
  // the (1, 1) class comes first and counts the running value twice (the reference's `+=` of an fma that already carries it,
  // :4586): the choice among splits is made with exactly this number, so it is kept
  if (g11 != 0.0) {
    ll = ll + fma(F.f11, log(g11), ll);
  }
  const double known[3][2] = {{F.f12, g12}, {F.f21, g21}, {F.f22, g22}};  // :4588-4596, in this order
  for (const double (&term)[2] : known) {
    if (term[1] != 0.0) {
      ll = fma(term[0], log(term[1]), ll);
    }
  }
  return ll;
}

// the candidate with the largest likelihood, the lowest one among equals (:4710-4729)
double likeliest_split(const Freqs& F, const Roots& c) {
  int best = 0;
  if (c.n > 1) {
    double top = -DBL_MAX;
    for (int a = 0; a < c.n; ++a) {
      const double ll = split_lnlike(F, c.x[a]);
      if (ll > top) {
        top = ll;
        best = a;
      }
    }
  }
  return c.x[best];
}

struct PhasedOut {
  double r2, d, dprime;
  uint8_t neg;
};

PhasedOut phased_pair(const ldp_phased_stats_t& s) {
  const double nan = std::nan("");
  PhasedOut o = {nan, nan, nan, 0};
  const Freqs F = haplotype_freqs(s);
  if (!F.defined) {
    return o;
  }
  const double x = likeliest_split(F, candidate_splits(F));
  double D = F.f11 + x - F.p1 * F.q1;  // :4731
  if (fabs(D) < kZeroD) {
    D = 0.0;
  }
  o.d = D;
  o.neg = (D < 0.0) ? 1 : 0;
  o.r2 = D * D / (F.p1 * F.q1 * (F.p2 * F.q2));  // :4735
  // D' = D over the largest |D| the allele frequencies allow on D's side of zero (:4741-4745)
  const double room = (D >= 0.0) ? fmin(F.q1 * F.p2, F.q2 * F.p1) : fmin(F.q1 * F.p1, F.q2 * F.p2);
  o.dprime = D / room;
  return o;
}

}  // namespace

extern "C" int ldp_phased_ld(const ldp_phased_stats_t* in, uint64_t n, double* r2, double* d, double* dprime, uint8_t* is_neg) {
  if (n && (!in || !r2)) {
    return LDP_ERR_INVALID;
  }
  auto work = [&](uint64_t q0, uint64_t q1) {
    for (uint64_t q = q0; q < q1; ++q) {
      const PhasedOut o = phased_pair(in[q]);
      r2[q] = o.r2;
      if (d) {
        d[q] = o.d;
      }
      if (dprime) {
        dprime[q] = o.dprime;
      }
      if (is_neg) {
        is_neg[q] = o.neg;
      }
    }
  };
  // threads over pairs: a pair costs a few hundred nanoseconds (a log or two, sometimes acos and three cos)
  constexpr uint64_t kPairsPerThread = 8192;
  const uint64_t want = (n + kPairsPerThread - 1) / kPairsPerThread;
  const uint64_t nt = std::min<uint64_t>(std::max(1u, std::min(32u, std::thread::hardware_concurrency())), want);
  if (nt <= 1) {
    work(0, n);
    return LDP_OK;
  }
  std::vector<std::thread> pool;
  const uint64_t per = (n + nt - 1) / nt;
  for (uint64_t w = 0; w < nt; ++w) {
    const uint64_t q0 = std::min(n, w * per), q1 = std::min(n, q0 + per);
    pool.emplace_back(work, q0, q1);
  }
  for (std::thread& th : pool) {
    th.join();
  }
  return LDP_OK;
}
