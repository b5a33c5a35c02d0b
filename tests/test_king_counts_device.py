"""ldp_king_counts_block / ldp_king_block_hits: the KING-robust integers of sample pairs from the resident image (ldp_king.hip) against the
numpy definition of king_tools, exact: integers only, and a kinship double that is one correctly rounded division of them on either side, so
every comparison is equality and no pair is left out.  The shapes walk the kernels' edges: sample counts around the 32-sample MFMA block, the
64-sample tile, the 256-sample strip group and the image's 512-sample column group; variant counts around the 64-variant k-step, the 128
variants a lane loads at once and the 256-variant minimum slab; slabs of the minimum length against the launch's own choice; and one image of
70,000 variants whose all-het sample takes hethet past 16 bits over many slabs."""
import functools

import numpy as np
import pytest

import king_tools as K
import ldtools as T

pytestmark = pytest.mark.gpu

SAMPLES = (2, 31, 32, 33, 63, 64, 65, 255, 257, 511, 513)
VARIANTS = (1, 63, 64, 65, 127, 129, 255, 256, 257)
SWAP = np.array([2, 1, 0, 3], dtype=np.uint8)          # REF-based <-> ALT-based codes
TO_BED = np.array([3, 2, 0, 1], dtype=np.uint8)        # .pgen code -> .bed code
MIN_SLAB = 256
THRESHOLDS = (-1.0, 0.0442, 0.177, 0.354)


@functools.lru_cache(maxsize=None)
def codes(m, n, rate, seed=1):
    """(m, n) REF-based codes with hets, `rate` of the calls missing; where the shape allows: a variant nobody has a call at, two identical
    samples, a sample without a call and one without a het call.  Read-only, shared by the tests"""
    rng = np.random.default_rng(seed + 1000003 * m + n)
    raw = ((rng.random((m, n)) < 0.3).astype(np.uint8) + (rng.random((m, n)) < 0.3).astype(np.uint8))
    if rate:
        raw[rng.random((m, n)) < rate] = 3
    if m >= 3:
        raw[m // 2, :] = 3
    if n >= 8:
        raw[:, 3] = raw[:, 2]
        raw[:, 5] = 3
        raw[:, 6][raw[:, 6] == 1] = 2
    raw.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def want(m, n, rate, seed=1):
    return K.counts(codes(m, n, rate, seed))


def loaded(pkg, raw, encoding="ref", options=()):
    m, n = raw.shape
    eng = pkg.LdPruneEngine(n, 50, 5, False, 0.2, order=2, device=0)
    for name, value in options:
        eng.set_option(name, value)
    eng.set_variants_matrix(m)
    if encoding == "bed":
        eng.load_genotypes_host(0, T.pack_2bit(TO_BED[raw]), pkg.LDP_GENO_BED)
    elif encoding == "inverse":
        eng.load_genotypes_host(0, T.pack_2bit(raw), pkg.LDP_GENO_INVERSE)
    else:
        eng.load_genotypes_host(0, T.pack_2bit(raw), pkg.LDP_GENO_REF)
    return eng


def check(pkg, eng, c, block=None, what=None, **kw):
    """the dense form of the block (default: every sample against every sample) against the definition's matrices c"""
    n = c["hethet"].shape[0]
    rf, rc, cf, cc = block or (0, n, 0, n)
    got = eng.king_counts_block(rf, rc, cf, cc, **kw)
    exp = K.block_struct(c, rf, rc, cf, cc, pkg.KING_COUNTS_DTYPE)
    assert got.shape == exp.shape and got.dtype == exp.dtype
    for f in K.FIELDS:
        assert np.array_equal(got[f], exp[f]), (f, what, block)


def check_hits(eng, c, thr, block=None, **kw):
    n = c["hethet"].shape[0]
    rf, rc, cf, cc = block or (0, n, 0, n)
    got, found = eng.king_block_hits(thr, rf, rc, cf, cc, **kw)
    exp = K.hits(c, thr, rf, rc, cf, cc)
    assert found == len(exp), (thr, block)
    assert [tuple(int(v) for v in h) for h in got] == exp, (thr, block)


@pytest.mark.parametrize("n", SAMPLES)
def test_sample_counts_around_block_tile_and_column_group(gpu_pkg, n):
    raw = codes(300, n, 0.04)
    eng = loaded(gpu_pkg, raw)
    check(gpu_pkg, eng, want(300, n, 0.04))
    check_hits(eng, want(300, n, 0.04), 0.0442)
    eng.close()


def test_eleven_hundred_samples_run_several_tiles_and_the_diagonal(gpu_pkg):
    n = 1100
    raw = codes(300, n, 0.04)
    c = want(300, n, 0.04)
    eng = loaded(gpu_pkg, raw)
    stats = {}
    check(gpu_pkg, eng, c, stats=stats)
    assert stats["pair_variants"] == (n * (n - 1) // 2) * 300 and stats["ms_kernel"] > 0.0
    # blocks that cut through tiles, strip groups and the diagonal; one entirely above the diagonal (all zero); 1 x 1 blocks
    for block in ((515, 300, 3, 700), (33, 1, 32, 1), (40, 1, 40, 1), (0, 100, 200, 300), (257, 843, 250, 10), (1099, 1, 0, 1100), (1, 1, 0, 1), (700, 37, 690, 45)):
        check(gpu_pkg, eng, c, block)
    check_hits(eng, c, 0.0442, (515, 300, 3, 700))
    eng.close()


@pytest.mark.parametrize("m", VARIANTS)
def test_variant_counts_around_k_step_and_minimum_slab(gpu_pkg, m):
    raw = codes(m, 130, 0.04)
    eng = loaded(gpu_pkg, raw)
    check(gpu_pkg, eng, want(m, 130, 0.04))
    check(gpu_pkg, eng, want(m, 130, 0.04), slab_variants=MIN_SLAB)
    eng.close()


def test_seventy_thousand_variants_pass_sixteen_bits_over_many_slabs(gpu_pkg):
    base = codes(70000, 200, 0.04)
    raw = base.copy()
    raw[:, 3] = 1
    raw[:, 4] = 1
    raw[:, 64] = 3
    c = K.counts(raw)
    assert c["hethet"][4, 3] == 70000 and not K.nsnp(c)[64].any()
    eng = loaded(gpu_pkg, raw)
    check(gpu_pkg, eng, c)
    check(gpu_pkg, eng, c, slab_variants=4096)   # 18 slabs
    check_hits(eng, c, 0.177)
    eng.close()


def test_three_minimum_slabs_and_one_variant(gpu_pkg):
    m = 3 * MIN_SLAB + 1
    raw = codes(m, 130, 0.04)
    eng = loaded(gpu_pkg, raw)
    a = eng.king_counts_block(0, 130, 0, 130, slab_variants=MIN_SLAB)
    b = eng.king_counts_block(0, 130, 0, 130)
    assert np.array_equal(a, b)
    check(gpu_pkg, eng, want(m, 130, 0.04), slab_variants=MIN_SLAB)
    for bad in (1, 255, 257, 65536 + 256):
        with pytest.raises(gpu_pkg.LdpError) as err:
            eng.king_counts_block(0, 130, 0, 130, slab_variants=bad)
        assert err.value.code == gpu_pkg.LDP_ERR_INVALID
    eng.close()


@pytest.mark.parametrize("rate", (0.0, 0.04, 0.6))
def test_missing_rates_and_include_masks(gpu_pkg, rate):
    m, n = 700, 257
    raw = codes(m, n, rate)
    eng = loaded(gpu_pkg, raw)
    check(gpu_pkg, eng, want(m, n, rate))
    for kind in ("all", "none", "alternating", "last"):
        inc = np.zeros(m, dtype=np.uint8)
        if kind == "all":
            inc[:] = 1
        elif kind == "alternating":
            inc[::2] = 1
        elif kind == "last":
            inc[m - 1] = 7   # (any non-zero byte includes)
        c = K.counts(raw, inc)
        check(gpu_pkg, eng, c, what=kind, include=inc)
        check(gpu_pkg, eng, c, what=kind, include=inc, slab_variants=MIN_SLAB)
        check_hits(eng, c, 0.0442, include=inc)
    eng.close()


@pytest.mark.parametrize("encoding", ("ref", "bed", "inverse", "alt_major"))
def test_every_input_coding(gpu_pkg, encoding):
    """... and rows the image stores inverted (ALT is the major allele of every row of the "alt_major" set): all five integers are the same
    when a variant's 0 and 2 are swapped"""
    m, n = 300, 130
    raw = codes(m, n, 0.04)
    c = want(m, n, 0.04)
    if encoding == "alt_major":
        major_ref = ((raw == 0).sum(axis=1) >= (raw == 2).sum(axis=1))
        raw = np.where(major_ref[:, None], SWAP[raw], raw)
        for f in K.FIELDS:
            assert np.array_equal(K.counts(raw)[f], c[f])
    eng = loaded(gpu_pkg, raw, "ref" if encoding == "alt_major" else encoding)
    if encoding == "alt_major":
        recs = eng.variant_recs()
        decided = (raw == 0).sum(axis=1) != (raw == 2).sum(axis=1)
        assert ((recs["flags"][decided] & 1) == 1).all(), "the set is meant to be ALT-major"
    check(gpu_pkg, eng, c)
    eng.close()


def test_sub_ranges_of_variants(gpu_pkg):
    raw = codes(1000, 130, 0.04)
    eng = loaded(gpu_pkg, raw)
    for first, n in ((0, 1000), (1, 998), (37, 129), (255, 257), (999, 1), (500, 0), (1000, 0)):
        inc = np.zeros(n, dtype=np.uint8)
        inc[::3] = 1
        check(gpu_pkg, eng, K.counts(raw[first:first + n]), first=first, n=n, what=(first, n))
        check(gpu_pkg, eng, K.counts(raw[first:first + n], inc), first=first, n=n, include=inc, slab_variants=MIN_SLAB, what=(first, n))
    with pytest.raises(gpu_pkg.LdpError) as err:
        eng.king_counts_block(0, 130, 0, 130, first=999, n=2)
    assert err.value.code == gpu_pkg.LDP_ERR_INVALID
    # no variant: zeros, and every pair a hit (0 / 0 is NaN, which the filter keeps)
    got, found = eng.king_block_hits(0.0442, 0, 130, 0, 130, first=500, n=0)
    assert found == 130 * 129 // 2 and not got["homhom"].any()
    eng.close()


def test_before_and_after_restrict_variants_and_after_a_reload(gpu_pkg):
    raw = codes(1000, 257, 0.04).copy()
    eng = loaded(gpu_pkg, raw)
    check(gpu_pkg, eng, K.counts(raw))
    raw[77] = codes(1000, 257, 0.6, seed=5)[12]
    eng.load_genotypes_host(77, T.pack_2bit(raw[77:78]), gpu_pkg.LDP_GENO_REF)
    check(gpu_pkg, eng, K.counts(raw))
    keep = np.random.default_rng(9).random(1000) < 0.6
    keep[[0, 999]] = (False, True)
    eng.restrict_variants(keep, np.zeros(int(keep.sum()), dtype=np.uint32))
    kept = raw[keep]
    check(gpu_pkg, eng, K.counts(kept))
    check(gpu_pkg, eng, K.counts(kept[33:433]), first=33, n=400)
    # the engine is still the engine the restriction made: it runs, and the image reads the same afterwards
    eng.run()
    check(gpu_pkg, eng, K.counts(kept))
    eng.close()


def test_windowed_plan_with_several_owned_runs(gpu_pkg):
    raw = codes(300, 130, 0.04)
    eng = gpu_pkg.LdPruneEngine(130, 50, 5, False, 0.2, order=2, device=0)
    chr_idx = np.concatenate([np.zeros(100), np.ones(50), np.full(1, 2), np.full(149, 3)]).astype(np.uint32)
    eng.set_variants(chr_idx)
    eng.load_genotypes_host(0, T.pack_2bit(raw), gpu_pkg.LDP_GENO_REF)
    check(gpu_pkg, eng, K.counts(raw[:150]), first=0, n=150)       # two chromosomes
    inc = np.zeros(120, dtype=np.uint8)
    inc[::2] = 1
    check(gpu_pkg, eng, K.counts(raw[20:140], inc), first=20, n=120, include=inc)
    with pytest.raises(gpu_pkg.LdpError) as err:   # a variant alone on its chromosome has no row
        eng.king_counts_block(0, 130, 0, 130, first=0, n=300)
    assert err.value.code == gpu_pkg.LDP_ERR_STATE
    eng.close()


@pytest.mark.parametrize("thr", THRESHOLDS)
def test_hits_are_the_pairs_not_below_the_threshold(gpu_pkg, thr):
    """nan pairs (a sample without a call) stay, -inf pairs (no het call on either side, some difference) go"""
    m, n = 300, 257
    c = want(m, n, 0.04)
    k = K.kinship(c)
    low = np.tril(np.ones((n, n), dtype=bool), -1)
    assert np.isnan(k[low]).any() and np.isneginf(k[low]).any()
    eng = loaded(gpu_pkg, codes(m, n, 0.04))
    check_hits(eng, c, thr)
    check_hits(eng, c, thr, (100, 157, 37, 100))
    eng.close()


def test_hit_count_beyond_capacity_is_reported(gpu_pkg):
    m, n = 300, 130
    c = want(m, n, 0.04)
    exp = K.hits(c, -1.0, 0, n, 0, n)
    eng = loaded(gpu_pkg, codes(m, n, 0.04))
    got, found = eng.king_block_hits(-1.0, 0, n, 0, n, capacity=10)
    assert found == len(exp) > 10 and len(got) == 10
    assert set(tuple(int(v) for v in h) for h in got) <= set(exp)
    got, found = eng.king_block_hits(-1.0, 0, n, 0, n, capacity=0)
    assert found == len(exp) and len(got) == 0
    eng.close()


def test_output_stride_and_nothing_written_outside_the_block(gpu_pkg):
    import ctypes
    pkg = gpu_pkg
    m, n = 300, 130
    eng = loaded(pkg, codes(m, n, 0.04))
    ld = 50
    buf = np.full((45, ld, 5), 0xA5A5A5A5, dtype=np.uint32)
    rc = pkg.lib().ldp_king_counts_block(eng._h, 0, m, None, 60, 40, 30, 37, buf[2:].ctypes.data_as(ctypes.c_void_p), ld)
    assert rc == 0
    exp = K.block_struct(want(m, n, 0.04), 60, 40, 30, 37, pkg.KING_COUNTS_DTYPE)
    for k, f in enumerate(K.FIELDS):
        assert np.array_equal(buf[2:42, :37, k], exp[f])
    assert (buf[:2] == 0xA5A5A5A5).all() and (buf[42:] == 0xA5A5A5A5).all() and (buf[2:42, 37:] == 0xA5A5A5A5).all()
    eng.close()


def test_state_errors_and_invalid_arguments(gpu_pkg):
    import ctypes
    pkg = gpu_pkg
    eng = pkg.LdPruneEngine(130, 50, 5, False, 0.2, order=2, device=0)
    with pytest.raises(pkg.LdpError) as err:   # no plan yet
        eng.king_counts_block(0, 130, 0, 130, n=0)
    assert err.value.code == pkg.LDP_ERR_STATE
    eng.set_variants_matrix(300)
    with pytest.raises(pkg.LdpError) as err:
        eng.king_counts_block(0, 130, 0, 130)
    assert err.value.code == pkg.LDP_ERR_STATE
    raw = codes(300, 130, 0.04)
    eng.load_genotypes_host(0, T.pack_2bit(raw[:100]), pkg.LDP_GENO_REF)   # (the first 100 rows only)
    check(pkg, eng, K.counts(raw[:100]), first=0, n=100)
    for call in (lambda: eng.king_counts_block(0, 130, 0, 130, first=0, n=101), lambda: eng.king_block_hits(0.0, 0, 130, 0, 130, first=0, n=101)):
        with pytest.raises(pkg.LdpError) as err:
            call()
        assert err.value.code == pkg.LDP_ERR_STATE
    for block in ((0, 131, 0, 130), (0, 130, 1, 130), (130, 1, 0, 1)):   # samples beyond founder_ct
        with pytest.raises(pkg.LdpError) as err:
            eng.king_counts_block(*block, first=0, n=100)
        assert err.value.code == pkg.LDP_ERR_INVALID
        with pytest.raises(pkg.LdpError) as err:
            eng.king_block_hits(0.0, *block, first=0, n=100)
        assert err.value.code == pkg.LDP_ERR_INVALID
    L = pkg.lib()
    out = np.zeros((130, 130), dtype=pkg.KING_COUNTS_DTYPE)
    cnt = ctypes.c_uint64()
    assert L.ldp_king_counts_block(eng._h, 0, 100, None, 0, 130, 0, 130, None, 130) == pkg.LDP_ERR_INVALID
    assert L.ldp_king_counts_block(eng._h, 0, 100, None, 0, 130, 0, 130, out.ctypes.data_as(ctypes.c_void_p), 129) == pkg.LDP_ERR_INVALID
    assert L.ldp_king_counts_block(None, 0, 0, None, 0, 130, 0, 130, out.ctypes.data_as(ctypes.c_void_p), 130) == pkg.LDP_ERR_INVALID
    assert L.ldp_king_block_hits(eng._h, 0, 100, None, 0, 130, 0, 130, 0.0, None, 0, None) == pkg.LDP_ERR_INVALID
    assert L.ldp_king_block_hits(eng._h, 0, 100, None, 0, 130, 0, 130, 0.0, None, 5, ctypes.byref(cnt)) == pkg.LDP_ERR_INVALID
    eng.close()


def test_unsupported_on_bit_planes_and_phased_rows(gpu_pkg):
    pkg = gpu_pkg
    raw = codes(300, 130, 0.04)
    eng = loaded(pkg, raw, options=(("pair_mfma", 0),))
    for call in (lambda: eng.king_counts_block(0, 130, 0, 130), lambda: eng.king_block_hits(0.0, 0, 130, 0, 130)):
        with pytest.raises(pkg.LdpError) as err:
            call()
        assert err.value.code == pkg.LDP_ERR_UNSUPPORTED
    eng.close()
    phase = (np.random.default_rng(3).random(raw.shape) < 0.5).astype(np.uint8)
    rows = pkg.pack_phased_rows(T.pack_2bit(raw), phase, 130)
    eng = pkg.LdPruneEngine(260, 50, 5, False, 0.2, order=2, device=0)
    eng.set_variants(np.zeros(300, dtype=np.uint32))
    eng.load_genotypes_host(0, rows, pkg.LDP_GENO_REF | pkg.LDP_GENO_PHASED)
    with pytest.raises(pkg.LdpError) as err:
        eng.king_counts_block(0, 130, 0, 130)
    assert err.value.code == pkg.LDP_ERR_UNSUPPORTED
    eng.close()


def test_unsupported_through_a_het_to_missing_sample_map(gpu_pkg):
    pkg = gpu_pkg
    raw = codes(300, 130, 0.04)
    eng = pkg.LdPruneEngine(100, 50, 5, False, 0.2, order=2, device=0)
    eng.set_variants_matrix(300)
    eng.set_sample_map(130, np.arange(100, dtype=np.uint32), np.ones(100, dtype=np.uint8))
    eng.load_genotypes_host(0, T.pack_2bit(raw), pkg.LDP_GENO_REF | pkg.LDP_GENO_MAPPED)
    with pytest.raises(pkg.LdpError) as err:
        eng.king_counts_block(0, 100, 0, 100)
    assert err.value.code == pkg.LDP_ERR_UNSUPPORTED
    eng.close()


def test_unsupported_on_a_sharded_engine(gpu_pkg):
    pkg = gpu_pkg
    eng = pkg.LdPruneEngine(130, 50, 5, False, 0.2, order=2, device=0)
    eng.set_variants(np.zeros(300, dtype=np.uint32))
    eng.set_shard(0, 2)
    with pytest.raises(pkg.LdpError) as err:
        eng.king_counts_block(0, 130, 0, 130, first=0, n=1)
    assert err.value.code == pkg.LDP_ERR_UNSUPPORTED
    eng.close()
