"""CPU tests of the references tests/test_pair_decisions_inputs.py compares the engine with for rows that are re-laid out on their
way into the image: ldtools.hap_raw_codes (LDP_GENO_PHASED rows as 2S haplotype "samples") and ldtools.mapped_raw_codes
(LDP_GENO_MAPPED rows as the engine's gathered columns).  Both feed the ONE per-pair reference band_pair_stats / band_decisions,
which tests/test_pair_reference.py checks against the oracle; here the column order of the haplotypes, the decisions of EVERY
candidate pair of small bands and the orientation-independence that lets one reference serve every input form are checked
against the oracle's own word-by-word arithmetic (oracle/ldoracle.c)."""
import ctypes

import numpy as np
import pytest

import ldtools as T
from test_host_logic import make_positions
from test_pair_reference import oracle_all_pairs

R2S = (0.02, 0.2, 0.5, 0.95)


def band_of(pkg, n, chr_idx, bps, window=25):
    eng = pkg.LdPruneEngine(n, window, 1, False, 0.2)
    eng.set_variants(chr_idx, bps)
    lo, cand = eng.band()
    eng.close()
    return lo, cand


@pytest.mark.parametrize("s", [2, 33, 513])
def test_haplotype_columns_and_every_decision_equal_the_oracle(pkg, s):
    m = 64
    raw, pp, pi = T.synth_phased(m, s, seed=300 + s, missing_rate=0.05, ld_copy_prob=0.6, redraw=0.1)
    raw[7] = 2                                   # monomorphic rows, an all-missing one, an all-het one
    raw[13] = 0
    raw[21] = 3
    raw[34] = 1
    pi = pi & (raw == 1)
    pi[34] = np.arange(s) % 2
    codes = T.hap_raw_codes(raw, pi)
    assert codes.shape == (m, 2 * s) and set(np.unique(codes)) <= {0, 2, 3}
    hrows, mf, unphased, hap_ct = T.oracle_hapsplit(raw, (raw == 1).astype(np.uint8), pi)
    assert hap_ct == 2 * s and not unphased.any()
    # the column order: HapsplitMustPhased's bits, haplotype by haplotype.  The oracle's rows count the MINOR allele (PgrGetInv1P), so a row
    # whose major allele is ALT carries "has REF" where hap_raw_codes carries "has ALT"
    _, _, altmaj = T.oracle_prepare(raw)
    wc = (hap_ct + 63) // 64
    hap = np.stack([T.bitmap_to_bool(hrows[v, :wc].copy(), hap_ct) for v in range(m)])
    nm = np.stack([T.bitmap_to_bool(hrows[v, wc:].copy(), hap_ct) for v in range(m)])
    assert np.array_equal(nm, codes != 3)
    assert np.array_equal(hap, ((codes == 2) ^ altmaj[:, None].astype(bool)) & nm)
    assert (hap[:, 0::2] != hap[:, 1::2]).any()  # (het calls: the two haplotypes of a sample differ, so the order is really tested)
    chr_idx, bps = make_positions(m, 2, s + 3)
    lo, cand = band_of(pkg, hap_ct, chr_idx, bps)
    first, second = T.band_pairs(lo)
    assert len(first) == cand > 300
    stats = T.band_pair_stats(codes, lo)
    lib = T.oracle()
    hstats = [T.oracle_hap_pair_stats(hrows, hap_ct, int(i), int(j)) for i, j in zip(first, second)]
    # the six integers are the genotype-coded ones of the haplotype columns: cov and both variances 4 x the reference's
    h = np.array([st.astuple() for st in hstats], dtype=np.int64).reshape(-1, 4)
    cov, v1, v2 = T.band_cov_vars(stats)
    assert np.array_equal(stats[:, 0], h[:, 0])
    assert np.array_equal(cov, 4.0 * (h[:, 0] * h[:, 3] - h[:, 1] * h[:, 2]))
    assert np.array_equal(v1, 4.0 * (h[:, 1] * (h[:, 0] - h[:, 1]))) and np.array_equal(v2, 4.0 * (h[:, 2] * (h[:, 0] - h[:, 2])))
    for r2 in R2S:
        thr = lib.ldo_prune_thresh(r2)
        want = np.array([bool(lib.ldo_hap_exceeds(ctypes.byref(st), thr)) for st in hstats], dtype=bool)
        nd, msg = T.compare_decisions(T.band_decisions(stats, r2), want, lo, stats, r2)
        assert nd == 0, msg
        if s > 2 and r2 == 0.2:
            assert 0 < int(want.sum()) < cand   # (both answers occur)
    print("pairs compared: %d x %d thresholds" % (cand, len(R2S)))


@pytest.mark.parametrize("n_raw,ones,twice", [(5, 2, 2), (90, 31, 29), (700, 300, 250)])
def test_mapped_columns_and_every_decision_equal_the_oracle(pkg, n_raw, ones, twice):
    """columns = `ones` samples whose het calls become missing + `twice` samples two times each (the chrX layout)"""
    m = 64
    rng = np.random.default_rng(n_raw)
    raw = T.synth_raw_codes(m, n_raw, seed=n_raw + 1, missing_rate=0.04, ld_copy_prob=0.6, redraw=0.1)
    raw[2] = 1        # all het: every call of the first group becomes missing
    raw[3] = 3
    perm = rng.permutation(n_raw)
    part1, part2 = np.sort(perm[:ones]), np.sort(perm[ones:ones + twice])
    src = np.concatenate([part1, part2, part2]).astype(np.uint32)
    het = np.concatenate([np.ones(ones, np.uint8), np.zeros(2 * twice, np.uint8)])
    cols = T.mapped_raw_codes(raw, src, het)
    assert cols.shape == (m, len(src)) and not ((cols[:, :ones] == 1).any()) and np.array_equal(cols[:, ones:], raw[:, src[ones:]])
    rows, mf, alt_major = T.host_rows(raw, src, het)
    # the host-built rows are the same columns, inverted where ALT is the major allele of the columns BEFORE the substitution
    swap = np.array([2, 1, 0, 3], dtype=np.uint8)
    assert np.array_equal(np.where(alt_major[:, None], swap[cols], cols), rows)
    chr_idx, bps = make_positions(m, 2, n_raw + 3)
    lo, cand = band_of(pkg, len(src), chr_idx, bps)
    stats = T.band_pair_stats(cols, lo)
    # oracle_all_pairs-style decisions over the host-built rows: they are in the orientation their builder chose (loaded as
    # LDP_GENO_INVERSE), so the oracle's planes are split from them as they are
    hom, r2h, vaggs = T.oracle_split(T.pack_2bit(rows), len(src))
    lib = T.oracle()
    first, second = T.band_pairs(lo)
    sts = [T.oracle_pair_stats(hom, r2h, vaggs, len(src), int(i), int(j)) for i, j in zip(first, second)]
    want_stats = np.array([st.astuple() for st in sts], dtype=np.int64).reshape(-1, 6)
    # nm and the two ssq are the same numbers; sums and dot agree up to the rows' orientation, which the decision does not see
    assert np.array_equal(stats[:, [0, 2, 4]], want_stats[:, [0, 2, 4]])
    assert np.array_equal(np.abs(stats[:, [1, 3]]), np.abs(want_stats[:, [1, 3]]))
    for r2 in R2S:
        thr = lib.ldo_prune_thresh(r2)
        want = np.array([bool(lib.ldo_exceeds(ctypes.byref(st), thr)) for st in sts], dtype=bool)
        nd, msg = T.compare_decisions(T.band_decisions(stats, r2), want, lo, stats, r2)
        assert nd == 0, msg
    print("pairs compared: %d x %d thresholds" % (cand, len(R2S)))


def test_decisions_do_not_depend_on_the_allele_a_row_is_oriented_on(pkg):
    """One reference for every input form: flip the alleles of a third of the rows (REF-coded 0 <-> 2) and every decision stays -- against
    band_decisions and against the oracle over the flipped rows.  The six integers do change (sums and dot products change sign where
    one row of the pair flips relative to its major allele ... which re-orienting on the major allele undoes: they are equal too)."""
    m, n = 64, 257
    raw = T.synth_raw_codes(m, n, seed=77, missing_rate=0.0, ld_copy_prob=0.6, redraw=0.1)
    raw[0::3, ::17] = 3
    raw[10, :] = 1
    raw[10, : n // 2] = 0
    flipped = raw.copy()
    swap = np.array([2, 1, 0, 3], dtype=np.uint8)
    flipped[1::3] = swap[raw[1::3]]
    chr_idx, bps = make_positions(m, 2, 9)
    lo, cand = band_of(pkg, n, chr_idx, bps)
    a, b = T.band_pair_stats(raw, lo), T.band_pair_stats(flipped, lo)
    # without the major-allele orientation the integers differ, with it they are the same up to exact ties (REF wins a tie on both sides)
    assert not np.array_equal(T.band_pair_stats(raw, lo, orient=False), T.band_pair_stats(flipped, lo, orient=False))
    assert np.array_equal(a[:, [0, 2, 4]], b[:, [0, 2, 4]]) and np.array_equal(np.abs(a[:, [1, 3, 5]]), np.abs(b[:, [1, 3, 5]]))
    for r2 in R2S:
        da, db = T.band_decisions(a, r2), T.band_decisions(b, r2)
        assert np.array_equal(da, db) and (r2 != 0.2 or 0 < int(da.sum()) < cand)
        # ... and REF-oriented statistics, which really do differ between the two, decide the same
        assert np.array_equal(T.band_decisions(T.band_pair_stats(flipped, lo, orient=False), r2), da)
        _, want, _ = oracle_all_pairs(flipped, lo, r2)
        assert np.array_equal(want, da)


def test_major_oriented_planes_of_codes():
    """ldtools.major_oriented_planes (what the GPU tests compare LdPruneEngine.planes() with) against the oracle's SplitHomRef2het"""
    raw = T.synth_raw_codes(12, 77, seed=4, missing_rate=0.1)
    raw[5] = np.where(np.arange(77) % 3 == 0, 0, 2)     # ALT-major
    inv, mf, altmaj = T.oracle_prepare(raw)
    assert altmaj[5] and not altmaj.all()
    hom, r2h, _ = T.oracle_split(inv, 77)
    for v in range(12):
        h, r = T.major_oriented_planes(raw[v])
        assert np.array_equal(h, hom[v].view(np.uint32)[:3]) and np.array_equal(r, r2h[v].view(np.uint32)[:3]), v
