"""ldp_phased_ld (host code: haplotype-frequency r^2, D, D' from a pair's five integers) against the reference binary's --r2-phased /
--r-phased tables, field by field as text.  No GPU: the integers come from numpy, sample by sample (phased_tools.brute_dense)."""
import numpy as np
import pytest

import ldtools as T
import phased_tools as P

COLS = "cols=+d,+dprime,+dprimeabs"


def _positions(m):
    return np.arange(m) * 10 + 1


def _check_against_reference(pkg, cwd, file_args, raw, present=None, info=None, cols=COLS):
    """every line of both tables equals what ldp_phased_ld gives for numpy's integers; pairs the reference leaves out are exactly the
    undefined ones (NaN here)"""
    m = raw.shape[0]
    ids = ["snp%d" % i for i in range(m)]
    first, second = P.all_pairs(m)
    stats = P.brute_stats(raw, first, second, present, info)
    r2, d, dprime, neg = pkg.phased_ld(stats)
    assert np.array_equal(np.isnan(r2), np.isnan(d)) and np.array_equal(np.isnan(r2), np.isnan(dprime))
    compared = 0
    for flag, signed in (("--r2-phased", False), ("--r-phased", True)):
        ref, names = P.ref_table(cwd, file_args, flag, [cols, "--ld-window-r2", "0"], out="ref" + flag[2:4].strip("-"))
        assert names[0] == ("PHASED_R" if signed else "PHASED_R2") and names[1] == "D", names
        abs_dprime = names[2] == "ABS_DPRIME"
        assert abs_dprime or names[2] == "DPRIME", names
        defined = {(ids[i], ids[j]) for i, j, v in zip(first, second, r2) if v == v}
        assert set(ref) == defined, (sorted(set(ref) ^ defined)[:10], len(ref), len(defined))
        for k in range(len(first)):
            key = (ids[first[k]], ids[second[k]])
            if key in ref:
                got = P.table_fields(r2[k], d[k], dprime[k], neg[k], signed, abs_dprime)
                assert got == ref[key][:3], (flag, key, got, ref[key], stats[k])
                compared += 1
    return compared


def _need_ref():
    if not T.have_ref():
        pytest.skip("oracle/_ref/plink2 not built")


def test_unphased_fileset_matches_reference(pkg, tmp_path):
    _need_ref()
    m, n = 120, 90
    raw = T.synth_raw_codes(m, n, seed=5, missing_rate=0.05)
    T.write_pgen_fixed(str(tmp_path / "d"), raw, ["1"] * m, _positions(m))
    assert _check_against_reference(pkg, str(tmp_path), ["--pfile", "d"], raw) > 10000
    # ... and the signed D' column
    assert _check_against_reference(pkg, str(tmp_path), ["--pfile", "d"], raw, cols="cols=+d,+dprime") > 10000


def test_fully_phased_fileset_matches_reference(pkg, tmp_path):
    _need_ref()
    m, n = 80, 130
    raw, present, info = T.synth_phased(m, n, seed=6, missing_rate=0.03)
    T.write_pgen_phased(str(tmp_path / "d"), raw, info, ["1"] * m, _positions(m))
    assert _check_against_reference(pkg, str(tmp_path), ["--pfile", "d"], raw, present, info) > 5000


def test_partially_phased_fileset_matches_reference(pkg, tmp_path):
    _need_ref()
    m, n = 80, 130
    raw = T.synth_raw_codes(m, n, seed=7, missing_rate=0.03)
    present, info = T.synth_phase(raw, seed=8, unphased_rate=0.3)
    T.write_vcf(str(tmp_path / "d.vcf"), raw, ["1"] * m, _positions(m), present, info)
    T.ref_import_vcf(str(tmp_path / "d.vcf"), str(tmp_path / "d"))
    assert _check_against_reference(pkg, str(tmp_path), ["--pfile", "d"], raw, present, info) > 5000


# ten samples, by hand: the branches random data seldom takes (plink2_ld.cc:4644-4724)
HAND = np.array([
    [1, 1, 1, 1, 1, 1, 1, 1, 1, 1],   # 0 every sample heterozygous
    [1, 1, 1, 1, 1, 1, 1, 1, 1, 1],   # 1 the same: with 0 all four known frequencies vanish (three candidate splits 0, K/2, K)
    [0, 0, 0, 0, 0, 2, 2, 2, 2, 2],   # 2 no heterozygote: K = 0 with every partner
    [0, 0, 0, 0, 0, 2, 2, 2, 2, 2],   # 3 ... r^2 = 1 with 2
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0],   # 4 monomorphic
    [3, 3, 3, 3, 3, 3, 3, 3, 3, 3],   # 5 never called: no joint sample
    [1, 1, 1, 1, 1, 1, 0, 0, 0, 0],   # 6
    [1, 0, 0, 0, 0, 0, 0, 0, 0, 0],   # 7 with 6: f22 = f12 = 0 and the middle split out of range (two candidates 0, K)
    [3, 3, 3, 3, 3, 0, 0, 0, 0, 0],   # 8 monomorphic over the joint samples with 2, though not on its own ...
    [0, 0, 0, 0, 0, 3, 3, 2, 2, 1],   # 9 ... and no joint sample with 8's called half missing here: partly
    [0, 1, 2, 0, 1, 2, 0, 1, 1, 0],   # 10 a generic partner
    [1, 1, 0, 2, 1, 0, 0, 2, 1, 0],   # 11 ... and another
    [0, 0, 0, 0, 0, 1, 1, 1, 0, 0],   # 12 with 6: f22 = 0 only, the cubic's constant term vanishes and its root at 0 is clipped to exactly 0
    [0, 1, 1, 0, 2, 2, 0, 0, 0, 2],   # 13 with 14 (n 10, sums 8 and 9, known 1, unknown 1): the cubic has ONE real root, 0.00369 of K = 0.05
    [0, 1, 2, 2, 0, 0, 1, 2, 1, 0],   # 14
    [0, 0, 1, 0, 0, 0, 1, 0, 2, 1],   # 15 with 16 (sums 5 and 4, known 0, unknown 2): three roots -K/2, 0, K/2 -- the first is no split, the
    [0, 0, 0, 1, 0, 1, 1, 0, 0, 1],   # 16    second is clipped to 0
], dtype=np.uint8)


def test_hand_made_branches_match_reference(pkg, tmp_path):
    _need_ref()
    m = HAND.shape[0]
    T.write_pgen_fixed(str(tmp_path / "d"), HAND, ["1"] * m, _positions(m))
    assert _check_against_reference(pkg, str(tmp_path), ["--pfile", "d"], HAND) > 20
    assert _check_against_reference(pkg, str(tmp_path), ["--pfile", "d"], HAND, cols="cols=+d,+dprime") > 20


def _one(pkg, n, a, b, k, u):
    st = np.array([(n, a, b, k, u)], dtype=pkg.PHASED_STATS_DTYPE)
    r2, d, dp, neg = pkg.phased_ld(st)
    return float(r2[0]), float(d[0]), float(dp[0]), int(neg[0])


def test_branches_on_tuples(pkg):
    """the same branches straight on integers, with the values the mathematics gives"""
    # K = 0: two variants without a double heterozygote, in complete LD (f11 = f22 = 1/2)
    assert _one(pkg, 10, 10, 10, 10, 0) == (1.0, 0.25, 1.0, 0)
    # ... in complete repulsion (f12 = f21 = 1/2)
    assert _one(pkg, 10, 10, 10, 0, 0) == (1.0, -0.25, -1.0, 1)
    # K = 0, independent: D = 0 exactly, the sign stays positive
    r2, d, dp, neg = _one(pkg, 8, 8, 8, 4, 0)
    assert (r2, d, dp, neg) == (0.0, 0.0, 0.0, 0)
    # every sample heterozygous at both: f11 = f22 = f12 = f21 = 0, K = 1/2; splits 0, K/2, K tie two by two and the reference's
    # likelihood (its f11 term counted twice, plink2_ld.cc:4586) prefers x = 0: complete repulsion
    assert _one(pkg, 10, 10, 10, 0, 10) == (1.0, -0.25, -1.0, 1)
    # f22 = f12 = 0, K = 1/20, f11 = 13/20, f21 = 1/4: candidates 0 and K only; the likelihood decides
    # (x = 0: 0.05 ln 0.015, doubled, + 0.65 ln 0.65 + 0.25 ln 0.3 = -1.001; x = K: 0.05 ln 0.035, doubled, + 0.65 ln 0.7 + 0.25 ln 0.25
    # = -0.914): x = K, D = 0.7 - 0.7 * 0.95 = 0.035, r^2 = 0.035^2 / (0.7 * 0.95 * 0.3 * 0.05), D' = 0.035 / min(0.95 * 0.3, 0.05 * 0.7) = 1;
    # a handful of roundings each: 1e-14 is a hundred times their sum
    r2, d, dp, neg = _one(pkg, 10, 6, 1, 0, 1)
    assert neg == 0 and abs(d - 0.035) < 1e-14 and abs(r2 - 0.035 ** 2 / (0.7 * 0.95 * 0.3 * 0.05)) < 1e-14 and abs(dp - 1.0) < 1e-13
    # one real root of the cubic (HAND rows 13, 14, pinned against the reference's text below): inside (0, K), D of its sign
    r2, d, dp, neg = _one(pkg, 10, 8, 9, 1, 1)
    p, q = 1 - 8 / 20, 1 - 9 / 20
    f11 = 1 - 16 / 20
    assert f11 - p * q - 1e-15 <= d <= f11 + 0.05 - p * q + 1e-15 and abs(d - (f11 + 0.0036901001192129216 - p * q)) < 1e-9
    # monomorphic over the joint samples (first, then second variant), and no joint sample: undefined
    for t in ((10, 0, 5, 0, 0), (10, 5, 0, 0, 0), (10, 20, 5, 10, 0), (0, 0, 0, 0, 0)):
        assert all(x != x for x in _one(pkg, *t)[:3]) and _one(pkg, *t)[3] == 0
    # optional outputs may be left out
    import ctypes
    st = np.array([(10, 10, 10, 10, 0)], dtype=pkg.PHASED_STATS_DTYPE)
    r2 = np.zeros(1)
    assert pkg.lib().ldp_phased_ld(st.ctypes.data_as(ctypes.c_void_p), 1, r2.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None, None, None) == 0 and r2[0] == 1.0
    assert pkg.lib().ldp_phased_ld(None, 1, None, None, None, None) == pkg.LDP_ERR_INVALID


def test_many_pairs_run_on_threads_and_agree_with_one_by_one(pkg):
    rng = np.random.default_rng(3)
    n = 40000
    nm = rng.integers(1, 200, n)
    u = rng.integers(0, nm + 1)
    k = rng.integers(0, 2 * (nm - u) + 1)
    a = k + u + rng.integers(0, 2 * nm - k - u + 1)
    a = np.minimum(a, 2 * nm)
    b = np.minimum(k + u + rng.integers(0, 2 * nm + 1), 2 * nm)
    b = np.minimum(b, 2 * nm - (a - k - u))   # f11 >= 0
    b = np.maximum(b, k + u)
    st = np.zeros(n, dtype=pkg.PHASED_STATS_DTYPE)
    for f, x in zip(P.STATS_FIELDS, (nm, a, b, k, u)):
        st[f] = x
    whole = pkg.phased_ld(st)
    for lo in (0, 17000, 39990):
        part = pkg.phased_ld(st[lo:lo + 10])
        for w, p in zip(whole, part):
            assert np.array_equal(w[lo:lo + 10], p, equal_nan=True)
