"""ldp_hwe_ln_p_host() -- the host restatement of hwe_kernel's arithmetic (csrc/ldp_hwe_core.h) -- against the exact evaluation of the
definition in integers (hwe_tools.py), within the derived bound (4 n + 64) 2^-52 + 4 |ln p| 2^-52, both `midp` settings.  No GPU."""
import math

import numpy as np
import pytest

import hwe_tools as H


def host_eval(pkg, triples, midp):
    got = [pkg.hwe_ln_p_host(a, b, c, midp) for a, b, c in triples]
    return np.array([g[0] for g in got], dtype=np.float64), np.array([g[1] for g in got], dtype=np.uint8)


@pytest.mark.parametrize("midp", [False, True])
@pytest.mark.parametrize("name", ["small", "n400", "n3000", "golden"])
def test_host_matches_the_exact_value(pkg, name, midp):
    """`small`: every triple with n <= 32 (every exact tie there is among them); `n400` / `n3000`: seeded draws with planted het excess and
    deficit, either allele the rarer; `golden`: n = 70,001 and n = 500,000, all-het and rare = 1, 2, 3 included"""
    want = H.oracle_set(name)
    ln_p, flags = host_eval(pkg, [(a, b, c) for a, b, c, _ in want], midp)
    H.check_against_oracle(name, midp, ln_p, flags)


def test_the_small_set_holds_the_adjacent_ties(pkg):
    """the exhaustive set does contain exact ties with a neighbour (4 r c == (k + 2)(k + 1)), where `midp` differs from half the observed term"""
    ties = 0
    for a, b, c, exp in H.oracle_set("small"):
        ws, obs = H.weights(a, b, c)
        ties += sum(1 for i, (_, w) in enumerate(ws) if (i != obs) and (w == ws[obs][1]))
        assert not exp[False][1]
    assert ties >= 10


def test_empty_and_invalid_triples(pkg):
    assert pkg.hwe_ln_p_host(0, 0, 0, False) == (0.0, 0)
    assert pkg.hwe_ln_p_host(0, 0, 0, True) == (math.log(0.5), 0)
    v, f = pkg.hwe_ln_p_host(2 ** 30, 2 ** 30, 0, False)
    assert math.isnan(v) and f == 0x80
    v, f = pkg.hwe_ln_p_host(2 ** 31 - 1, 0, 0, False)   # the largest n: monomorphic, one table
    assert v == 0.0 and f == 0


def test_orientation_does_not_matter(pkg):
    for a, b, c, _ in H.oracle_set("n400")[:50]:
        for midp in (False, True):
            assert pkg.hwe_ln_p_host(a, b, c, midp) == pkg.hwe_ln_p_host(c, b, a, midp)
