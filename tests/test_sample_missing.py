"""ldp_sample_missing_counts: per-sample missing-call counts read from the resident 2-bit image (ldp_sample_missing.hip) against numpy's
`(raw == 3).sum(axis=0)`, exact.  Integers only, so every comparison is equality.  The shapes walk the kernel's edges: sample counts around
the 16-sample dword, the 64-sample unit and the 512-sample column group (whose padding columns are coded missing in every row and must never
be counted), row counts around the 3 / 15 rows of the bit-sliced counters' first two levels and the 32 row lanes of a block, slabs that end
inside a group of rows, and one image of 70,000 rows where a sample that misses every call fills the 8-bit fields of full slabs (255 per
lane) and passes 65,535 in all."""
import functools

import numpy as np
import pytest

import ldtools as T

pytestmark = pytest.mark.gpu

N_AT_300 = (2, 15, 16, 17, 63, 64, 65, 511, 512, 513, 1025, 5000)
M_AT_130 = (1, 2, 3, 4, 15, 16, 17, 255, 256, 257, 1000)
PATTERNS = ("none", "row", "sample", "last", "s511_512", "random")
GUARD = 0xA5A5A5A5
SWAP = np.array([2, 1, 0, 3], dtype=np.uint8)          # REF-based <-> ALT-based codes
TO_BED = np.array([3, 2, 0, 1], dtype=np.uint8)        # .pgen code -> .bed code


@functools.lru_cache(maxsize=None)
def codes(m, n, pattern, seed=1):
    """(m, n) REF-based codes, REF the common allele, with the pattern's missing calls; read-only, shared by the tests"""
    rng = np.random.default_rng(seed + 1000003 * m + n)
    raw = ((rng.random((m, n)) < 0.2).astype(np.uint8) + (rng.random((m, n)) < 0.2).astype(np.uint8))
    if pattern == "row":
        raw[m // 2, :] = 3
    elif pattern == "sample":
        raw[:, n // 3] = 3
    elif pattern == "last":
        raw[::2, n - 1] = 3
    elif pattern == "s511_512":
        for s in (511, 512):
            if s < n:
                raw[1::3, s] = 3
    elif pattern == "random":
        rate = rng.uniform(0.0, 0.6, size=(m, 1))
        raw[rng.random((m, n)) < rate] = 3
    else:
        assert pattern == "none"
    raw.setflags(write=False)
    return raw


def want_counts(raw, first=0, n=None):
    n = raw.shape[0] - first if n is None else n
    return (raw[first:first + n] == 3).sum(axis=0).astype(np.uint32)


def loaded(pkg, raw, encoding="ref", options=()):
    """an engine in the state ldp_restrict_variants() starts from: all-pairs plan, every row loaded"""
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


def guarded_counts(eng, first=0, n=None):
    """the counts, written into the middle of a guard-filled buffer that must come back untouched around them"""
    nf = eng.founder_ct
    buf = np.full(nf + 1200, GUARD, dtype=np.uint32)      # (more than a column group of padding columns behind the last sample)
    got = eng.sample_missing_counts(first, n, out=buf[100:]).copy()
    assert (buf[:100] == GUARD).all() and (buf[100 + nf:] == GUARD).all(), "written outside out[0 .. founder_ct)"
    return got


@pytest.mark.parametrize("n", N_AT_300)
def test_sample_counts_around_dword_unit_and_column_group(gpu_pkg, n):
    raw = codes(300, n, "random")
    eng = loaded(gpu_pkg, raw)
    assert np.array_equal(guarded_counts(eng), want_counts(raw))
    eng.close()


@pytest.mark.parametrize("m", M_AT_130)
def test_row_counts_around_counter_levels_and_row_lanes(gpu_pkg, m):
    raw = codes(m, 130, "random")
    eng = loaded(gpu_pkg, raw)
    assert np.array_equal(guarded_counts(eng), want_counts(raw))
    eng.close()


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("encoding", ("ref", "bed", "inverse", "alt_major"))
def test_missing_patterns_in_every_input_coding(gpu_pkg, pattern, encoding):
    """... and in rows the image stores inverted (ALT is the major allele of every row of the "alt_major" set): missing is 11 either way"""
    for m, n in ((300, 513), (257, 130)):
        raw = codes(m, n, pattern)
        if encoding == "alt_major":
            raw = SWAP[raw]
        eng = loaded(gpu_pkg, raw, "ref" if encoding == "alt_major" else encoding)
        if encoding == "alt_major":
            recs = eng.variant_recs()
            complete = (raw != 3).any(axis=1)
            assert ((recs["flags"][complete] & 1) == 1).all(), "the set is meant to be ALT-major"
        assert np.array_equal(guarded_counts(eng), want_counts(raw)), (m, n)
        eng.close()


@pytest.mark.parametrize("slab_rows", (0, 8160, 1 << 20))
def test_seventy_thousand_rows(gpu_pkg, slab_rows):
    """the one shape where a count passes 65,535 and -- with full slabs of 8,160 rows (also what a larger request is clamped to) -- a lane's
    8-bit field reaches its 255"""
    for pattern in ("sample", "random"):
        raw = codes(70000, 100, pattern)
        eng = loaded(gpu_pkg, raw, options=(("sample_missing_slab_rows", slab_rows),))
        got = guarded_counts(eng)
        want = want_counts(raw)
        assert want.max() > 65535 or pattern == "random"
        assert np.array_equal(got, want), pattern
        assert eng.sample_missing_stats()["bytes_read"] == 70000 * 128
        eng.close()


@pytest.mark.parametrize("slab_rows", (0, 128, 100))
def test_sub_ranges_off_slab_boundaries(gpu_pkg, slab_rows):
    raw = codes(1000, 130, "random")
    eng = loaded(gpu_pkg, raw, options=(("sample_missing_slab_rows", slab_rows),))
    for first, n in ((0, 1000), (1, 998), (37, 129), (128, 128), (127, 130), (255, 2), (999, 1), (500, 0), (1000, 0)):
        assert np.array_equal(guarded_counts(eng, first, n), want_counts(raw, first, n)), (first, n)
    with pytest.raises(gpu_pkg.LdpError) as err:
        eng.sample_missing_counts(999, 2)
    assert err.value.code == gpu_pkg.LDP_ERR_INVALID
    eng.close()


def test_zero_variants_give_zeros(gpu_pkg):
    raw = codes(300, 65, "sample")
    eng = loaded(gpu_pkg, raw)
    got = guarded_counts(eng, 7, 0)
    assert got.shape == (65,) and not got.any()
    eng.close()


def test_after_restrict_variants_the_kept_rows_only(gpu_pkg):
    raw = codes(1000, 513, "random")
    eng = loaded(gpu_pkg, raw)
    before = guarded_counts(eng)
    assert np.array_equal(before, want_counts(raw))
    keep = np.random.default_rng(9).random(1000) < 0.6
    keep[[0, 999]] = (False, True)
    eng.restrict_variants(keep, np.zeros(int(keep.sum()), dtype=np.uint32))
    kept = raw[keep]
    assert np.array_equal(guarded_counts(eng), want_counts(kept))
    assert np.array_equal(guarded_counts(eng, 33, 400), want_counts(kept, 33, 400))
    # the engine is still the engine the restriction made: it runs
    eng.run()
    assert np.array_equal(guarded_counts(eng), want_counts(kept))
    eng.close()


def test_windowed_plan_counts_the_owned_rows(gpu_pkg):
    """under ldp_set_variants() too (rows of subcontigs; a variant alone on its chromosome has no row: LDP_ERR_STATE)"""
    raw = codes(300, 130, "random")
    eng = gpu_pkg.LdPruneEngine(130, 50, 5, False, 0.2, order=2, device=0)
    chr_idx = np.concatenate([np.zeros(150), np.ones(1), np.full(149, 2)]).astype(np.uint32)
    eng.set_variants(chr_idx)
    eng.load_genotypes_host(0, T.pack_2bit(raw), gpu_pkg.LDP_GENO_REF)
    assert np.array_equal(guarded_counts(eng, 0, 150), want_counts(raw, 0, 150))
    assert np.array_equal(guarded_counts(eng, 151, 149), want_counts(raw, 151, 149))
    with pytest.raises(gpu_pkg.LdpError) as err:
        eng.sample_missing_counts(0, 300)
    assert err.value.code == gpu_pkg.LDP_ERR_STATE
    eng.close()


def test_state_error_before_the_load(gpu_pkg):
    eng = gpu_pkg.LdPruneEngine(130, 50, 5, False, 0.2, order=2, device=0)
    eng.set_variants_matrix(300)
    with pytest.raises(gpu_pkg.LdpError) as err:
        eng.sample_missing_counts()
    assert err.value.code == gpu_pkg.LDP_ERR_STATE
    eng.load_genotypes_host(0, T.pack_2bit(codes(300, 130, "random")[:100]), gpu_pkg.LDP_GENO_REF)   # (the first 100 rows only)
    assert np.array_equal(guarded_counts(eng, 0, 100), want_counts(codes(300, 130, "random"), 0, 100))
    with pytest.raises(gpu_pkg.LdpError) as err:
        eng.sample_missing_counts(0, 101)
    assert err.value.code == gpu_pkg.LDP_ERR_STATE
    eng.close()


def test_unsupported_on_bit_planes_and_phased_rows(gpu_pkg):
    pkg = gpu_pkg
    raw = codes(300, 130, "random")
    eng = loaded(pkg, raw, options=(("pair_mfma", 0),))
    with pytest.raises(pkg.LdpError) as err:
        eng.sample_missing_counts()
    assert err.value.code == pkg.LDP_ERR_UNSUPPORTED
    eng.close()
    phase = (np.random.default_rng(3).random(raw.shape) < 0.5).astype(np.uint8)
    rows = pkg.pack_phased_rows(T.pack_2bit(raw), phase, 130)
    eng = pkg.LdPruneEngine(260, 50, 5, False, 0.2, order=2, device=0)
    eng.set_variants(np.zeros(300, dtype=np.uint32))
    eng.load_genotypes_host(0, rows, pkg.LDP_GENO_REF | pkg.LDP_GENO_PHASED)
    with pytest.raises(pkg.LdpError) as err:
        eng.sample_missing_counts()
    assert err.value.code == pkg.LDP_ERR_UNSUPPORTED
    eng.close()
