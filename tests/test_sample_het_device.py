"""ldp_sample_het_counts: per-sample het-call counts, missing-call counts and weighted missing-call sums read from the resident 2-bit image
(ldp_sample_het.hip) against numpy, exact: integers only (the weighted sums modulo 2^64, which numpy's uint64 wraps to as the device does), so
every comparison is equality.  The shapes walk the kernel's edges: sample counts around the 16-sample dword, the 64-sample unit and the
512-sample column group (whose padding columns are coded missing in every row: they must reach neither the counts nor the weighted walk), row
counts around the 3 / 15 rows of the bit-sliced counters' first two levels, the 32 row lanes and the 480 rows a block takes per pass, slabs of
32, 64 and the launch's own choice, a full slab of 8,160 rows and one row more, and one image of 70,000 rows where an all-het and an
all-missing sample fill every 8-bit field of full slabs (255 per lane)."""
import functools

import numpy as np
import pytest

import ldtools as T

pytestmark = pytest.mark.gpu

FOUNDERS = (1, 2, 15, 17, 63, 65, 511, 513, 1025)
ROWS = (1, 2, 3, 31, 33, 479, 481, 8160, 8161)
SLABS = (32, 64, 0)
RATES = (0.0, 0.001, 0.05, 0.6)
SWAP = np.array([2, 1, 0, 3], dtype=np.uint8)          # REF-based <-> ALT-based codes
TO_BED = np.array([3, 2, 0, 1], dtype=np.uint8)        # .pgen code -> .bed code
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


@functools.lru_cache(maxsize=None)
def codes(m, n, rate, full_row=False, seed=1):
    """(m, n) REF-based codes with hets, REF the common allele, `rate` of the calls missing (full_row: the middle row misses every call);
    read-only, shared by the tests"""
    rng = np.random.default_rng(seed + 1000003 * m + n)
    raw = ((rng.random((m, n)) < 0.25).astype(np.uint8) + (rng.random((m, n)) < 0.25).astype(np.uint8))
    if rate:
        raw[rng.random((m, n)) < rate] = 3
    if full_row:
        raw[m // 2, :] = 3
    raw.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def weights(m, kind="random"):
    if kind == "ones":
        w = np.full(m, ALL_ONES, dtype=np.uint64)
    else:
        w = np.random.default_rng(77 + m).integers(0, 1 << 63, size=m, dtype=np.uint64) * np.uint64(2) + np.uint64(1)  # (all 64 bits in use)
    w.setflags(write=False)
    return w


def include_of(m, kind):
    if kind is None:
        return None
    inc = np.zeros(m, dtype=np.uint8)
    if kind == "all":
        inc[:] = 1
    elif kind == "alternating":
        inc[::2] = 1
    elif kind == "last":
        inc[m - 1] = 7   # (any non-zero byte includes)
    else:
        assert kind == "none"
    return inc


def want(raw, include=None, weight=None, first=0, n=None):
    n = raw.shape[0] - first if n is None else n
    rows = raw[first:first + n]
    inc = np.ones(n, dtype=bool) if include is None else (np.asarray(include) != 0)
    het = ((rows == 1) & inc[:, None]).sum(axis=0).astype(np.uint32)
    mis_mask = (rows == 3) & inc[:, None]
    mis = mis_mask.sum(axis=0).astype(np.uint32)
    mw = None
    if weight is not None:
        with np.errstate(over="ignore"):
            mw = (mis_mask.astype(np.uint64) * np.asarray(weight, dtype=np.uint64)[:, None]).sum(axis=0, dtype=np.uint64)
    return het, mis, mw


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


def check(eng, raw, include=None, weight=None, first=0, n=None, what=None, slab_rows=None, stats=None):
    got = eng.sample_het_counts(first, n, include=include, weight=weight, slab_rows=slab_rows, stats=stats)
    exp = want(raw, include, weight, first, n)
    for name, g, w in zip(("het_ct", "missing_ct", "missing_weight"), got, exp):
        if w is None:
            assert g is None, (name, what)
        else:
            assert g.dtype == w.dtype and np.array_equal(g, w), (name, what)


@pytest.mark.parametrize("n", FOUNDERS)
def test_founder_counts_around_dword_unit_and_column_group(gpu_pkg, n):
    """the padding columns of the last column group (11 in every row) reach no sample's result (test_outputs_end_at_founder_ct has the guard
    behind the arrays)"""
    if n == 1:
        # an engine needs two founders (ldp_create refuses one, as the reference's prune does): a single column cannot reach the kernel
        with pytest.raises(gpu_pkg.LdpError):
            gpu_pkg.LdPruneEngine(1, 50, 5, False, 0.2, order=2, device=0)
        return
    raw = codes(300, n, 0.05, True)
    eng = loaded(gpu_pkg, raw)
    check(eng, raw, None, weights(300))
    check(eng, raw, include_of(300, "alternating"), weights(300, "ones"))
    check(eng, raw)
    eng.close()


def test_outputs_end_at_founder_ct(gpu_pkg):
    """the three arrays written through the C ABI into guard-filled buffers: nothing outside [0, founder_ct)"""
    import ctypes
    pkg = gpu_pkg
    for n in (65, 513):
        raw = codes(300, n, 0.05, True)
        eng = loaded(pkg, raw)
        het = np.full(n + 1200, 0xA5A5A5A5, dtype=np.uint32)
        mis = het.copy()
        mw = np.full(n + 1200, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        w = weights(300).copy()
        p = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))
        rc = pkg.lib().ldp_sample_het_counts(eng._h, 0, 300, None, p(w, ctypes.c_uint64), p(het[100:], ctypes.c_uint32), p(mis[100:], ctypes.c_uint32),
                                             p(mw[100:], ctypes.c_uint64))
        assert rc == 0
        e_het, e_mis, e_mw = want(raw, None, w)
        assert np.array_equal(het[100:100 + n], e_het) and np.array_equal(mis[100:100 + n], e_mis) and np.array_equal(mw[100:100 + n], e_mw)
        for buf, g in ((het, 0xA5A5A5A5), (mis, 0xA5A5A5A5), (mw, 0xA5A5A5A5A5A5A5A5)):
            assert (buf[:100] == g).all() and (buf[100 + n:] == g).all(), "written outside [0, founder_ct)"
        eng.close()


@pytest.mark.parametrize("m", ROWS)
def test_row_counts_around_counter_levels_lanes_and_slabs(gpu_pkg, m):
    raw = codes(m, 130, 0.05, True)
    eng = loaded(gpu_pkg, raw)
    for slab in SLABS:
        stats = {}
        check(eng, raw, None, weights(m), what=slab, slab_rows=slab)
        check(eng, raw, include_of(m, "alternating"), weights(m), what=slab, slab_rows=slab, stats=stats)
        assert stats["bytes_read"] == m * 128 and stats["ms_kernel"] > 0.0
    eng.close()


@pytest.mark.parametrize("slab_rows", (0, 8160, 1 << 20))
def test_seventy_thousand_rows_fill_every_field(gpu_pkg, slab_rows):
    """one all-het and one all-missing sample: with full slabs of 8,160 rows (also what a larger request is clamped to) every lane's 8-bit
    fields of both counter sets reach their 255, and both counts pass 65,535"""
    base = codes(70000, 65, 0.001)
    raw = base.copy()
    raw[:, 3] = 1
    raw[:, 64] = 3
    eng = loaded(gpu_pkg, raw)
    stats = {}
    for wkind in ("random", "ones"):
        check(eng, raw, None, weights(70000, wkind), what=wkind, slab_rows=slab_rows, stats=stats)
    assert stats["bytes_read"] == 70000 * 128
    het, mis, _ = eng.sample_het_counts(slab_rows=slab_rows)
    assert het[3] == 70000 and mis[64] == 70000 and mis[3] == 0 and het[64] == 0
    eng.close()


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("full_row", (False, True))
def test_missing_rates_weights_and_includes(gpu_pkg, rate, full_row):
    m, n = 481, 513
    raw = codes(m, n, rate, full_row)
    eng = loaded(gpu_pkg, raw)
    for wkind in ("random", "ones", None):
        for ikind in ("all", "none", "alternating", "last", None):
            check(eng, raw, include_of(m, ikind), None if wkind is None else weights(m, wkind), what=(wkind, ikind))
    eng.close()


@pytest.mark.parametrize("encoding", ("ref", "bed", "inverse", "alt_major"))
def test_every_input_coding(gpu_pkg, encoding):
    """... and rows the image stores inverted (ALT is the major allele of every row of the "alt_major" set): het is 01 and missing 11 either way"""
    for m, n in ((300, 513), (257, 130)):
        raw = codes(m, n, 0.05, True)
        if encoding == "alt_major":
            raw = SWAP[raw]
        eng = loaded(gpu_pkg, raw, "ref" if encoding == "alt_major" else encoding)
        if encoding == "alt_major":
            recs = eng.variant_recs()
            complete = (raw != 3).any(axis=1)
            assert ((recs["flags"][complete] & 1) == 1).all(), "the set is meant to be ALT-major"
        check(eng, raw, include_of(m, "alternating"), weights(m), what=(m, n))
        eng.close()


@pytest.mark.parametrize("slab_rows", SLABS)
def test_sub_ranges(gpu_pkg, slab_rows):
    """first_variant > 0: include and weight are the RANGE's arrays (entry 0 belongs to first_variant)"""
    raw = codes(1000, 130, 0.05)
    eng = loaded(gpu_pkg, raw)
    for first, n in ((0, 1000), (1, 998), (37, 129), (127, 130), (999, 1), (500, 0), (1000, 0)):
        inc = include_of(n, "alternating") if n else np.zeros(0, dtype=np.uint8)
        check(eng, raw, inc, weights(1000)[first:first + n], first, n, what=(first, n), slab_rows=slab_rows)
    with pytest.raises(gpu_pkg.LdpError) as err:
        eng.sample_het_counts(999, 2)
    assert err.value.code == gpu_pkg.LDP_ERR_INVALID
    eng.close()


def test_zero_variants_give_zeros(gpu_pkg):
    raw = codes(300, 65, 0.05)
    eng = loaded(gpu_pkg, raw)
    het, mis, mw = eng.sample_het_counts(7, 0, weight=np.zeros(0, dtype=np.uint64))
    assert het.shape == mis.shape == mw.shape == (65,) and not het.any() and not mis.any() and not mw.any()
    eng.close()


def test_before_and_after_restrict_variants(gpu_pkg):
    raw = codes(1000, 513, 0.05, True)
    eng = loaded(gpu_pkg, raw)
    w = weights(1000)
    check(eng, raw, None, w)
    keep = np.random.default_rng(9).random(1000) < 0.6
    keep[[0, 999]] = (False, True)
    eng.restrict_variants(keep, np.zeros(int(keep.sum()), dtype=np.uint32))
    kept = raw[keep]
    check(eng, kept, None, w[keep])
    check(eng, kept, include_of(400, "alternating"), w[keep][33:433], 33, 400)
    # the engine is still the engine the restriction made: it runs, and the image reads the same afterwards
    eng.run()
    check(eng, kept, None, w[keep])
    eng.close()


def test_windowed_plan_with_several_owned_runs(gpu_pkg):
    """under ldp_set_variants() the rows lie in runs of subcontigs (a variant alone on its chromosome has no row: LDP_ERR_STATE); a range
    over two runs takes one launch each, and each gets its own part of include / weight"""
    raw = codes(300, 130, 0.05)
    eng = gpu_pkg.LdPruneEngine(130, 50, 5, False, 0.2, order=2, device=0)
    chr_idx = np.concatenate([np.zeros(100), np.ones(50), np.full(1, 2), np.full(149, 3)]).astype(np.uint32)
    eng.set_variants(chr_idx)
    eng.load_genotypes_host(0, T.pack_2bit(raw), gpu_pkg.LDP_GENO_REF)
    w = weights(300)
    check(eng, raw, include_of(150, "alternating"), w[:150], 0, 150)       # two chromosomes
    check(eng, raw, include_of(120, "last"), w[20:140], 20, 120)
    check(eng, raw, None, w[151:], 151, 149)
    with pytest.raises(gpu_pkg.LdpError) as err:
        eng.sample_het_counts(0, 300)
    assert err.value.code == gpu_pkg.LDP_ERR_STATE
    eng.close()


def test_reload_of_a_row(gpu_pkg):
    raw = codes(300, 130, 0.05).copy()
    eng = loaded(gpu_pkg, raw)
    check(eng, raw, None, weights(300))
    raw[77] = codes(300, 130, 0.6, seed=5)[12]
    eng.load_genotypes_host(77, T.pack_2bit(raw[77:78]), gpu_pkg.LDP_GENO_REF)
    check(eng, raw, None, weights(300))
    eng.close()


def test_state_errors_and_missing_outputs(gpu_pkg):
    import ctypes
    pkg = gpu_pkg
    eng = pkg.LdPruneEngine(130, 50, 5, False, 0.2, order=2, device=0)
    with pytest.raises(pkg.LdpError) as err:   # no plan yet
        eng.sample_het_counts(0, 0)
    assert err.value.code == pkg.LDP_ERR_STATE
    eng.set_variants_matrix(300)
    with pytest.raises(pkg.LdpError) as err:
        eng.sample_het_counts()
    assert err.value.code == pkg.LDP_ERR_STATE
    raw = codes(300, 130, 0.05)
    eng.load_genotypes_host(0, T.pack_2bit(raw[:100]), pkg.LDP_GENO_REF)   # (the first 100 rows only)
    check(eng, raw, None, weights(300)[:100], 0, 100)
    with pytest.raises(pkg.LdpError) as err:
        eng.sample_het_counts(0, 101)
    assert err.value.code == pkg.LDP_ERR_STATE
    L = pkg.lib()
    buf = np.zeros(130, dtype=np.uint32)
    p32 = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    w = weights(300).copy()
    assert L.ldp_sample_het_counts(eng._h, 0, 100, None, None, None, p32, None) == pkg.LDP_ERR_INVALID
    assert L.ldp_sample_het_counts(eng._h, 0, 100, None, None, p32, None, None) == pkg.LDP_ERR_INVALID
    assert L.ldp_sample_het_counts(eng._h, 0, 100, None, w.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), p32, p32, None) == pkg.LDP_ERR_INVALID
    assert L.ldp_sample_het_counts(None, 0, 0, None, None, p32, p32, None) == pkg.LDP_ERR_INVALID
    eng.close()


def test_unsupported_on_bit_planes_and_phased_rows(gpu_pkg):
    pkg = gpu_pkg
    raw = codes(300, 130, 0.05)
    eng = loaded(pkg, raw, options=(("pair_mfma", 0),))
    with pytest.raises(pkg.LdpError) as err:
        eng.sample_het_counts()
    assert err.value.code == pkg.LDP_ERR_UNSUPPORTED
    eng.close()
    phase = (np.random.default_rng(3).random(raw.shape) < 0.5).astype(np.uint8)
    rows = pkg.pack_phased_rows(T.pack_2bit(raw), phase, 130)
    eng = pkg.LdPruneEngine(260, 50, 5, False, 0.2, order=2, device=0)
    eng.set_variants(np.zeros(300, dtype=np.uint32))
    eng.load_genotypes_host(0, rows, pkg.LDP_GENO_REF | pkg.LDP_GENO_PHASED)
    with pytest.raises(pkg.LdpError) as err:
        eng.sample_het_counts()
    assert err.value.code == pkg.LDP_ERR_UNSUPPORTED
    eng.close()


def test_unsupported_through_a_het_to_missing_sample_map(gpu_pkg):
    pkg = gpu_pkg
    raw = codes(300, 130, 0.05)
    eng = pkg.LdPruneEngine(100, 50, 5, False, 0.2, order=2, device=0)
    eng.set_variants_matrix(300)
    eng.set_sample_map(130, np.arange(100, dtype=np.uint32), np.ones(100, dtype=np.uint8))
    eng.load_genotypes_host(0, T.pack_2bit(raw), pkg.LDP_GENO_REF | pkg.LDP_GENO_MAPPED)
    with pytest.raises(pkg.LdpError) as err:
        eng.sample_het_counts()
    assert err.value.code == pkg.LDP_ERR_UNSUPPORTED
    eng.close()


def test_unsupported_on_a_sharded_engine(gpu_pkg):
    pkg = gpu_pkg
    raw = codes(300, 130, 0.05)
    eng = pkg.LdPruneEngine(130, 50, 5, False, 0.2, order=2, device=0)
    eng.set_variants(np.zeros(300, dtype=np.uint32))
    eng.set_shard(0, 2)
    with pytest.raises(pkg.LdpError) as err:
        eng.sample_het_counts(0, 1)
    assert err.value.code == pkg.LDP_ERR_UNSUPPORTED
    eng.close()
