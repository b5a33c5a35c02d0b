"""hwe_kernel (csrc/ldp_hwe.hip) through ldp_hwe_ln_pvals_counts() and ldp_hwe_ln_pvals(): against the exact evaluation in integers
(hwe_tools.py) within the derived bound, launches around the 256-lane block edge, and on an engine bit-equal to the counts call on the records'
own counts -- before and after ldp_restrict_variants(), after a reload, over sub-ranges -- with every refusal."""
import ctypes

import numpy as np
import pytest

import hwe_tools as H
import ldtools as T

pytestmark = pytest.mark.gpu
M, N = 400, 120


def columns(triples):
    a = np.array(triples, dtype=np.uint32).reshape(-1, 3)
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()


def same_bits(a, b):
    return a.dtype == b.dtype and np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b)


@pytest.mark.parametrize("midp", [False, True])
@pytest.mark.parametrize("name", ["small", "n400", "n3000", "golden"])
def test_device_matches_the_exact_value(gpu_pkg, name, midp):
    want = H.oracle_set(name)
    ln_p, flags = gpu_pkg.hwe_ln_pvals_counts(*columns([(a, b, c) for a, b, c, _ in want]), midp=midp)
    H.check_against_oracle(name, midp, ln_p, flags)


def test_device_and_host_walk_alike(gpu_pkg):
    """the same sequence of IEEE operations up to the final log: at most a few units in the last place apart, the golden set's 250,000-step
    walks included"""
    for name in ("n3000", "golden"):
        triples = [(a, b, c) for a, b, c, _ in H.oracle_set(name)]
        for midp in (False, True):
            dev, dflags = gpu_pkg.hwe_ln_pvals_counts(*columns(triples), midp=midp)
            host = np.array([gpu_pkg.hwe_ln_p_host(a, b, c, midp)[0] for a, b, c in triples])
            assert np.all(np.abs(dev - host) <= 4 * np.spacing(np.abs(host)) + 2.0 ** -52), (name, midp, np.abs(dev - host).max())
            assert not dflags.any()


@pytest.mark.parametrize("count", [1, 255, 256, 257, 70000])
def test_block_edges(gpu_pkg, count):
    """one launch each; every lane's answer is the one the same triple gets alone in a launch of the n400 set (lanes are independent), and
    nothing is written behind the last variant"""
    pkg = gpu_pkg
    base = [(a, b, c) for a, b, c, _ in H.oracle_set("n400")]
    a0, b0, c0 = columns(base)
    ref, _ = pkg.hwe_ln_pvals_counts(a0, b0, c0)
    idx = (np.arange(count) * 7 + 3) % len(base)
    ln_p = np.full(count + 64, -777.0)
    flags = np.full(count + 64, 0xA5, dtype=np.uint8)
    p = lambda x, t: x.ctypes.data_as(ctypes.POINTER(t))
    a, b, c = a0[idx].copy(), b0[idx].copy(), c0[idx].copy()
    rc = pkg.lib().ldp_hwe_ln_pvals_counts(0, count, p(a, ctypes.c_uint32), p(b, ctypes.c_uint32), p(c, ctypes.c_uint32), 0, p(ln_p, ctypes.c_double),
                                           p(flags, ctypes.c_uint8))
    assert rc == 0
    assert same_bits(ln_p[:count], ref[idx]) and not flags[:count].any()
    assert (ln_p[count:] == -777.0).all() and (flags[count:] == 0xA5).all()


def loaded(pkg, raw, encoding=None):
    eng = pkg.LdPruneEngine(raw.shape[1], 50, 5, False, 0.2, order=2, device=0)
    eng.set_variants_matrix(raw.shape[0])
    eng.load_genotypes_host(0, T.pack_2bit(raw), pkg.LDP_GENO_REF if encoding is None else encoding)
    return eng


def check_engine(pkg, eng, raw, first=0, n=None):
    n = raw.shape[0] - first if n is None else n
    recs = eng.variant_recs(first, n)
    a, b, c = H.genotype_counts(raw[first:first + n])
    assert np.array_equal(recs["n_homref"], a) and np.array_equal(recs["n_het"], b) and np.array_equal(recs["n_homalt"], c)
    for midp in (False, True):
        want, wflags = pkg.hwe_ln_pvals_counts(recs["n_homref"], recs["n_het"], recs["n_homalt"], midp=midp)
        got, gflags = eng.hwe_ln_pvals(first, n, midp=midp)
        assert same_bits(got, want) and np.array_equal(gflags, wflags), (first, n, midp)


def test_engine_records(gpu_pkg):
    pkg = gpu_pkg
    raw = H.planted_codes(M, N, 21)
    eng = loaded(pkg, raw)
    check_engine(pkg, eng, raw)
    for first, n in ((0, 1), (1, 255), (37, 256), (143, 257), (399, 1), (400, 0)):
        check_engine(pkg, eng, raw, first, n)
    # the planted rows: all het is far out, nobody called is p = 1, as are the monomorphic row and (no het among two alleles alike) ...
    ln_p, _ = eng.hwe_ln_pvals()
    assert ln_p[H.V_ALL_HET] < -60 and ln_p[H.V_ALL_MISSING] == 0.0 and ln_p[H.V_MONO] == 0.0 and ln_p[H.V_HALF] < -60
    assert eng.hwe_ln_pvals(midp=True)[0][H.V_ALL_MISSING] == np.log(0.5)
    # a reload of some rows
    raw2 = raw.copy()
    raw2[50:60] = H.planted_codes(M, N, 22, plant=False)[100:110]
    eng.load_genotypes_host(50, T.pack_2bit(raw2[50:60]), pkg.LDP_GENO_REF)
    check_engine(pkg, eng, raw2)
    # ... and after ldp_restrict_variants(): the records follow their rows
    keep = np.random.default_rng(5).random(M) < 0.6
    keep[[H.V_ALL_HET, H.V_ALL_MISSING]] = True
    kept = np.flatnonzero(keep)
    eng.restrict_variants(keep, np.zeros(len(kept), dtype=np.uint32), (1000 + 10 * kept).astype(np.uint32))
    check_engine(pkg, eng, raw2[kept])
    check_engine(pkg, eng, raw2[kept], 5, 200)
    eng.close()


def test_engine_on_bit_planes(gpu_pkg):
    """the records, not the image, are read: an engine that keeps bit-planes answers the same"""
    pkg = gpu_pkg
    raw = H.planted_codes(M, N, 21)
    eng = pkg.LdPruneEngine(N, 50, 5, False, 0.2, order=2, device=0)
    eng.set_option("pair_mfma", 0)
    eng.set_variants_matrix(M)
    eng.load_genotypes_host(0, T.pack_2bit(raw), pkg.LDP_GENO_REF)
    check_engine(pkg, eng, raw)
    eng.close()


def test_state_errors(gpu_pkg):
    pkg = gpu_pkg
    raw = H.planted_codes(M, N, 21)
    eng = pkg.LdPruneEngine(N, 50, 5, False, 0.2, order=2, device=0)
    with pytest.raises(pkg.LdpError) as err:   # no plan yet
        eng.hwe_ln_pvals(0, 0)
    assert err.value.code == pkg.LDP_ERR_STATE
    eng.set_variants_matrix(M)
    with pytest.raises(pkg.LdpError) as err:   # nothing loaded
        eng.hwe_ln_pvals()
    assert err.value.code == pkg.LDP_ERR_STATE
    eng.load_genotypes_host(0, T.pack_2bit(raw[:100]), pkg.LDP_GENO_REF)
    check_engine(pkg, eng, raw[:100], 0, 100)
    with pytest.raises(pkg.LdpError) as err:
        eng.hwe_ln_pvals(0, 101)
    assert err.value.code == pkg.LDP_ERR_STATE
    with pytest.raises(pkg.LdpError) as err:   # beyond variant_ct
        eng.hwe_ln_pvals(390, 11)
    assert err.value.code == pkg.LDP_ERR_INVALID
    L = pkg.lib()
    buf = np.zeros(100, dtype=np.float64)
    assert L.ldp_hwe_ln_pvals(eng._h, 0, 100, 0, None, None) == pkg.LDP_ERR_INVALID
    assert L.ldp_hwe_ln_pvals(None, 0, 0, 0, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None) == pkg.LDP_ERR_INVALID
    assert L.ldp_hwe_ln_pvals(eng._h, 0, 100, 0, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None) == 0   # flags may be NULL
    assert same_bits(buf, eng.hwe_ln_pvals(0, 100)[0])
    eng.close()


def test_rows_without_raw_counts_are_refused(gpu_pkg):
    pkg = gpu_pkg
    raw = H.planted_codes(M, N, 21)
    eng = loaded(pkg, raw, pkg.LDP_GENO_INVERSE)
    with pytest.raises(pkg.LdpError) as err:
        eng.hwe_ln_pvals()
    assert err.value.code == pkg.LDP_ERR_UNSUPPORTED
    eng.close()
    # one INVERSE row among REF rows: ranges that leave it out are served
    eng = loaded(pkg, raw)
    eng.load_genotypes_host(200, T.pack_2bit(raw[200:201]), pkg.LDP_GENO_INVERSE)
    check_engine(pkg, eng, raw[:200], 0, 200)
    with pytest.raises(pkg.LdpError) as err:
        eng.hwe_ln_pvals(150, 100)
    assert err.value.code == pkg.LDP_ERR_UNSUPPORTED
    eng.close()
    phase = (np.random.default_rng(3).random(raw.shape) < 0.5).astype(np.uint8)
    rows = pkg.pack_phased_rows(T.pack_2bit(raw), phase, N)
    eng = pkg.LdPruneEngine(2 * N, 50, 5, False, 0.2, order=2, device=0)
    eng.set_variants(np.zeros(M, dtype=np.uint32))
    eng.load_genotypes_host(0, rows, pkg.LDP_GENO_REF | pkg.LDP_GENO_PHASED)
    with pytest.raises(pkg.LdpError) as err:
        eng.hwe_ln_pvals()
    assert err.value.code == pkg.LDP_ERR_UNSUPPORTED
    eng.close()
    eng = pkg.LdPruneEngine(100, 50, 5, False, 0.2, order=2, device=0)
    eng.set_variants_matrix(M)
    eng.set_sample_map(N, np.arange(100, dtype=np.uint32), np.ones(100, dtype=np.uint8))
    eng.load_genotypes_host(0, T.pack_2bit(raw), pkg.LDP_GENO_REF | pkg.LDP_GENO_MAPPED)
    with pytest.raises(pkg.LdpError) as err:
        eng.hwe_ln_pvals()
    assert err.value.code == pkg.LDP_ERR_UNSUPPORTED
    eng.close()


def test_sharded_engines_are_refused(gpu_pkg):
    pkg = gpu_pkg
    eng = pkg.LdPruneEngine(N, 50, 5, False, 0.2, order=2, device=0)
    eng.set_variants(np.zeros(M, dtype=np.uint32))
    eng.set_shard(0, 2)
    with pytest.raises(pkg.LdpError) as err:
        eng.hwe_ln_pvals(0, 1)
    assert err.value.code == pkg.LDP_ERR_UNSUPPORTED
    eng.close()


def test_counts_call_refuses_oversized_triples(gpu_pkg):
    pkg = gpu_pkg
    with pytest.raises(pkg.LdpError) as err:
        pkg.hwe_ln_pvals_counts([5, 2 ** 30], [5, 2 ** 30], [5, 0])
    assert err.value.code == pkg.LDP_ERR_INVALID
    ln_p, flags = pkg.hwe_ln_pvals_counts([], [], [])
    assert len(ln_p) == 0 and len(flags) == 0
    ln_p, _ = pkg.hwe_ln_pvals_counts([2 ** 31 - 1], [0], [0])
    assert ln_p[0] == 0.0
