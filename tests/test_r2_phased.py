"""--r2-phased on the GPU: the five integers of every pair (ldp_r2_phased_stats_block / _band_stats: the six-integer pair kernels plus
the double-heterozygote product of ldp_pair_phased.hip, with and without a phase engine) exact against numpy, and the device-side
filter of ldp_r2_phased_band_hits against the host-exact statistic.  Shapes cross the kernel's boundaries -- the 64-sample k-step, the
256-sample stage, the 512-sample chunk, the 32-row block, more than one 64 x 64 workgroup -- and nothing else."""
import functools

import numpy as np
import pytest

import ldtools as T
import phased_tools as P

pytestmark = pytest.mark.gpu

SHAPES = [(70, 63, 0.0), (150, 130, 0.05), (70, 257, 0.0), (96, 513, 0.2), (45, 1100, 0.01)]


@functools.lru_cache(maxsize=None)
def dataset(m, n, miss, phased):
    """raw codes with one row all-het, one all-missing, one monomorphic, one forced ALT-major; phased: 0 none, 1 every het, 2 70 % of
    them, with one variant whose phaseinfo is mostly 1.  Returns (raw, present, info, numpy's dense integers): computed once."""
    raw = T.synth_raw_codes(m, n, seed=1, missing_rate=miss)
    raw[5] = 1
    raw[11] = 3
    raw[17] = 0
    raw[23] = np.where(np.arange(n) % 7 == 0, 1, 2)   # ALT-major with hets
    present = info = None
    if phased:
        present, info = T.synth_phase(raw, seed=2, unphased_rate=0.0 if phased == 1 else 0.3)
        info[5] = present[5] & (np.arange(n) % 5 != 0)   # mostly 1: the phase row is stored inverted
        info[23] = present[23]
    want = P.brute_dense(raw, present, info)
    for a in (raw, want) + ((present, info) if phased else ()):
        a.setflags(write=False)
    return raw, present, info, want


def engines(pkg, raw, present, info, plan):
    """the genotype engine and (with phase) the phase engine, planned by plan(engine) and loaded"""
    m, n = raw.shape
    out = []
    for codes in (raw,) + ((P.phase_rows(present, info),) if present is not None else ()):
        e = pkg.LdPruneEngine(n, 100, 1, False, 0.2, device=0)
        plan(e)
        e.load_genotypes_host(0, T.pack_2bit(codes), pkg.LDP_GENO_REF)
        out.append(e)
    return out[0], (out[1] if len(out) > 1 else None)


def assert_same(got, want, what):
    for f in P.STATS_FIELDS:
        if not np.array_equal(got[f], want[f]):
            bad = np.argwhere(got[f] != want[f])
            k = tuple(bad[0])
            raise AssertionError("%s: %s differs at %d places, first %s: got %s, want %s" % (what, f, len(bad), k, got[k], want[k]))


def block_want(want, r0, rc, c0, cc):
    sub = want[r0:r0 + rc, c0:c0 + cc].copy()
    j = np.arange(r0, r0 + rc)[:, None]
    i = np.arange(c0, c0 + cc)[None, :]
    sub[i >= j] = 0
    return sub


def blocks_of(m):
    # the whole triangle, and sub-blocks whose edges are no multiples of 32 (below, across and above the diagonal)
    return [(0, m, 0, m), (33, m - 33, 0, 29), (m - 37, 37, 13, m - 30), (3, min(41, m - 3), 7, min(50, m - 7)), (1, 1, 0, 1)]


@pytest.mark.parametrize("phased", [0, 1, 2])
@pytest.mark.parametrize("m,n,miss", SHAPES)
def test_block_integers_match_numpy(gpu_pkg, m, n, miss, phased):
    raw, present, info, want = dataset(m, n, miss, phased)
    e, ph = engines(gpu_pkg, raw, present, info, lambda eng: eng.set_variants_matrix(m))
    try:
        for r0, rc, c0, cc in blocks_of(m):
            got = e.r2_phased_stats_block(r0, rc, c0, cc, phase=ph)
            assert_same(got, block_want(want, r0, rc, c0, cc), "block (%d, %d, %d, %d)" % (r0, rc, c0, cc))
        f = e.phased_filter()
        assert f["pairs_seen"] == 0 and f["pairs_dropped"] == 0
    finally:
        e.close()
        if ph is not None:
            ph.close()


def band_case(m):
    half = m // 2
    chr_idx = (np.arange(m) >= half).astype(np.uint32)
    bps = (1000 + 10 * np.arange(m)).astype(np.uint32)
    return chr_idx, bps


def band_want(want, lo, r0, rc):
    return np.concatenate([want[j, lo[j]:j] for j in range(r0, r0 + rc)] + [want[0, :0]])


@pytest.mark.parametrize("phased", [0, 2])
@pytest.mark.parametrize("var_radius", [3, 140])
@pytest.mark.parametrize("m,n,miss", SHAPES)
def test_band_integers_match_numpy(gpu_pkg, m, n, miss, var_radius, phased):
    """a 3-variant window and one wider than 128 (the whole chromosome where it is shorter), two chromosomes"""
    raw, present, info, want = dataset(m, n, miss, phased)
    chr_idx, bps = band_case(m)
    e, ph = engines(gpu_pkg, raw, present, info, lambda eng: eng.set_variants_vcor(chr_idx, bps, 10 ** 9, var_radius))
    try:
        lo, total = e.band()
        lo = lo.astype(np.int64)
        assert total == int((np.arange(m) - lo).sum()) and total > 0
        for r0, rc in ((0, m), (m // 2 - 9, 21), (35, 2)):
            got = e.r2_phased_band_stats(r0, rc, phase=ph)
            assert_same(got, band_want(want, lo, r0, rc), "band rows (%d, %d), radius %d" % (r0, rc, var_radius))
    finally:
        e.close()
        if ph is not None:
            ph.close()


def test_band_hits_keep_every_pair_that_passes(gpu_pkg):
    """thresholds 0.2, 0.8 and 0 on the (150, 130, 0.05) shape, one chromosome, every pair in the window: the survivors hold every pair
    whose host-exact value passes; nothing is dropped at 0; at 0.2 the filter drops at least half of what it sees; a buffer smaller
    than the survivors still reports their number."""
    m, n, miss = 150, 130, 0.05
    raw = T.synth_raw_codes(m, n, seed=1, missing_rate=miss)
    want = P.brute_dense(raw)
    first, second = P.all_pairs(m)
    stats = want[second, first]
    r2, d, dprime, neg = gpu_pkg.phased_ld(stats)
    bps = (1000 + 10 * np.arange(m)).astype(np.uint32)
    e, _ = engines(gpu_pkg, raw, None, None, lambda eng: eng.set_variants_vcor(np.zeros(m, dtype=np.uint32), bps, 10 ** 9))
    try:
        pairs = m * (m - 1) // 2
        for thr, unsquared in ((0.2, False), (0.8, False), (0.0, False), (0.2, True)):
            value = np.sqrt(r2) if unsquared else r2
            exact = {(int(i), int(j)) for i, j, v in zip(first, second, value) if v >= thr}
            st, hf, hs, found = e.r2_phased_band_hits(thr, phase=None, unsquared=unsquared)
            f = e.phased_filter()
            print("threshold %g%s: %d exact hits, %d survivors, filter saw %d and dropped %d" % (thr, " on |r|" if unsquared else "", len(exact), found, f["pairs_seen"], f["pairs_dropped"]))
            assert found == len(st) and f["pairs_seen"] == pairs and f["pairs_dropped"] == pairs - found
            got = {(int(i), int(j)) for i, j in zip(hf, hs)}
            assert len(got) == found and exact <= got, sorted(exact - got)[:10]
            assert_same(st, want[hs.astype(np.int64), hf.astype(np.int64)], "survivors' integers at %g" % thr)
            if thr == 0.0:
                assert f["pairs_dropped"] == 0 and found == pairs
            if (thr == 0.2) and not unsquared:
                assert len(exact) == 124 and 2 * f["pairs_dropped"] >= f["pairs_seen"]   # (124: the CPU count for this seed)
                st2, hf2, hs2, found2 = e.r2_phased_band_hits(thr, capacity=found // 2)
                assert found2 == found and len(st2) == found // 2
                assert {(int(i), int(j)) for i, j in zip(hf2, hs2)} <= got
        # a row range: only its second variants
        st, hf, hs, found = e.r2_phased_band_hits(0.0, row_first=40, row_ct=9)
        assert found == sum(range(40, 49)) and hs.min() == 40 and hs.max() == 48
    finally:
        e.close()


def test_engines_beyond_the_matrix_pipe_are_refused(gpu_pkg):
    """the double-heterozygote counts are f32 accumulators: an engine above ldp_matrix_pipe_max_founders() gets the library's
    'unsupported' status from every phased call, before anything is allocated or loaded"""
    n = gpu_pkg.matrix_pipe_max_founders() + 1
    e = gpu_pkg.LdPruneEngine(n, 100, 1, False, 0.2, device=0)
    try:
        e.set_variants_matrix(4)
        with pytest.raises(gpu_pkg.LdpError) as ei:
            e.r2_phased_stats_block(0, 4, 0, 4)
        assert ei.value.code == gpu_pkg.LDP_ERR_UNSUPPORTED
        e.set_variants_vcor(np.zeros(4, dtype=np.uint32), np.arange(4, dtype=np.uint32) + 1, 1000)
        with pytest.raises(gpu_pkg.LdpError) as ei:
            e.r2_phased_band_hits(0.2)
        assert ei.value.code == gpu_pkg.LDP_ERR_UNSUPPORTED
    finally:
        e.close()


def test_phase_engine_must_match(gpu_pkg):
    raw, present, info, _ = dataset(70, 63, 0.0, 1)
    e, ph = engines(gpu_pkg, raw, present, info, lambda eng: eng.set_variants_matrix(70))
    other = gpu_pkg.LdPruneEngine(64, 100, 1, False, 0.2, device=0)
    try:
        other.set_variants_matrix(70)
        for bad in (e, other):
            with pytest.raises(gpu_pkg.LdpError) as ei:
                e.r2_phased_stats_block(0, 70, 0, 70, phase=bad)
            assert ei.value.code == gpu_pkg.LDP_ERR_INVALID
        with pytest.raises(gpu_pkg.LdpError) as ei:
            e.r2_phased_band_stats(0, 70, phase=ph)   # an all-pairs plan has no band
        assert ei.value.code == gpu_pkg.LDP_ERR_STATE
    finally:
        for x in (e, ph, other):
            x.close()
