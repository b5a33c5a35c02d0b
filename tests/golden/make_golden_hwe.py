"""Writes tests/golden/hwe_large.json: the exact Hardy-Weinberg ln p of triples at sample counts where an exact evaluation takes minutes
(n = 70,001 and n = 500,000), for both `midp` settings, to 25 significant digits.  Offline:  python tests/golden/make_golden_hwe.py

Every weight w(k) = 2^k n! / (r! k! c!) is an integer; from the true w(k_min) the recurrence w(k + 2) = w(k) 4 r c / ((k + 2)(k + 1))
divides exactly, so one pass finds w(het) and a second one sums the tail, the ties and the total -- integers of up to a million bits, never
more than a few alive at a time."""
import json
import os
import sys
from decimal import Decimal, getcontext
from math import comb

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import hwe_tools as H  # noqa: E402

getcontext().prec = 60


def walk(hom1, het, hom2):
    n = hom1 + het + hom2
    rare = 2 * min(hom1, hom2) + het
    k = rare & 1
    r = (rare - k) // 2
    c = n - k - r
    w = comb(n, r) * comb(n - r, k) * (1 << k)
    while True:
        yield k, w
        if r == 0:
            return
        w, rem = divmod(w * (4 * r * c), (k + 2) * (k + 1))
        assert rem == 0
        k, r, c = k + 2, r - 1, c - 1


def exact(hom1, het, hom2):
    w_obs = next(w for k, w in walk(hom1, het, hom2) if k == het)
    tail = ties = total = 0
    far_tie = False
    for k, w in walk(hom1, het, hom2):
        total += w
        if w <= w_obs:
            tail += w
            if w == w_obs:
                ties += w
                far_tie = far_tie or (abs(k - het) > 2)
    return H.ln_int(tail) - H.ln_int(total), H.ln_int(2 * tail - ties) - H.ln_int(2 * total), far_tie


def hwe_triple(n, q, shift=0.0):
    """the expected counts at allele frequency q, `shift` of the het calls moved to (negative: taken from) the homozygotes"""
    het = round(2 * q * (1 - q) * n)
    hom2 = round(q * q * n)
    mv = round(abs(shift) * het)
    if shift > 0:      # deficit
        het -= mv
        hom2 += mv // 2
    elif shift < 0:    # excess
        mv = min(mv, 2 * hom2)
        het += mv
        hom2 -= mv // 2
    return n - het - hom2, het, hom2


def triples():
    out = []
    for n in (70001, 500000):
        out += [hwe_triple(n, 0.3, 0.004), hwe_triple(n, 0.05, 0.10), hwe_triple(n, 0.2, -0.10)]
        out += [(0, n, 0), (n // 2, 0, n - n // 2)]                  # all het; half / half homozygotes
        # rare = 1, 2, 3.  (At n = 500,000 a table with rare = 2 has, with midp, p = n / (2 n - 1) or 1 / (4 n - 2): 1e-12 from a boundary between
        # two 6-digit decimals either way, and the .hardy comparison over these triples takes no line out of its P column.  A mild excess at MAF 0.1
        # stands in for it there.)
        out += [(n - 1, 1, 0), (0, 2, n - 2) if n < 100000 else hwe_triple(n, 0.1, -0.02), (n - 2, 1, 1)]
    return out


if __name__ == "__main__":
    rows = []
    for a, b, c in triples():
        lp, lpm, far_tie = exact(a, b, c)
        rows.append({"hom1": a, "het": b, "hom2": c, "ln_p": format(lp, ".25E"), "ln_p_midp": format(lpm, ".25E"), "far_tie": far_tie})
        print(rows[-1], flush=True)
    with open(H.GOLDEN_LARGE, "w") as f:
        json.dump({"triples": rows}, f, indent=1)
        f.write("\n")
