"""ldp_restrict_variants: an engine that was loaded first (unplanned: ldp_set_variants_matrix) and then restricted to a subset of its variants
must be indistinguishable from a fresh engine that was planned with ldp_set_variants over the kept variants and loaded with the kept rows
alone -- image rows, records, major-allele frequencies, the prune set (also against the CPU oracle) and every candidate pair's decision,
bit for bit.  The image is compacted in place in batches of 16 rows here, so that both forms of a batch (direct copy, bounce buffer) run."""
import functools

import numpy as np
import pytest

import ldtools as T
from test_gpu_parity import WIDE_CASES
from test_host_logic import make_positions

pytestmark = pytest.mark.gpu

M = 600
BATCH = 16
WIDE = min((c for c in WIDE_CASES if c[5]), key=lambda c: c[0] * c[1])   # the smallest WIDE_CASES row with a bp window

# window, step, is_bp, r2, order, engine options set before planning
PLANS = {
    "count": (50, 5, False, 0.2, 2, {}),                                      # parallelogram work items
    "wide": (WIDE[3], WIDE[4], True, WIDE[6], WIDE[7], {"wide_min_reach": WIDE[8]}),   # 8 x 8 tiles
    "planes": (50, 5, False, 0.2, 2, {"pair_mfma": 0}),                      # bit-planes, popcount kernels
}


@functools.lru_cache(maxsize=None)
def genotype_rows(n):
    """(M, n) REF-based codes: the generator's rows, 5 % missing calls in every third row, and every fourth row with its alleles
    swapped, so that its REF allele is the rare one and the engine stores the row inverted."""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    complete = T.unpack_2bit(pkg.synth_genotypes_host(7, 0, M, n, 0.0), n)
    missing = T.unpack_2bit(pkg.synth_genotypes_host(7, 0, M, n, 0.05), n)
    raw = complete.copy()
    raw[0::3] = missing[0::3]
    swap = np.array([2, 1, 0, 3], dtype=np.uint8)
    raw[1::4] = swap[raw[1::4]]
    raw.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def positions(plan):
    if PLANS[plan][2]:
        # one run of positions without the generator's big gaps (the window reaches hundreds of variants: tiles), cut into two chromosomes
        _, bps = make_positions(M, 1, 17, big_gap_prob=0.0)
        return (np.arange(M) >= 450).astype(np.uint32), bps
    return (np.arange(M) >= 330).astype(np.uint32), None


def keep_masks():
    rng = np.random.default_rng(5)
    everything = np.ones(M, dtype=bool)
    row0 = everything.copy()
    row0[0] = False
    run40 = everything.copy()
    run40[100:140] = False
    two = np.zeros(M, dtype=bool)
    two[[211, 212]] = True
    one = np.zeros(M, dtype=bool)
    one[377] = True
    return {"everything": everything, "row0": row0, "run40": run40, "random": rng.random(M) < 0.5, "two": two, "one": one, "none": np.zeros(M, dtype=bool)}


MASKS = keep_masks()


def new_engine(pkg, n, plan):
    window, step, is_bp, r2, order, options = PLANS[plan]
    eng = pkg.LdPruneEngine(n, window, step, is_bp, r2, order=order, device=0)
    for name, value in options.items():
        eng.set_option(name, value)
    return eng


def loaded_unplanned(pkg, n, plan):
    eng = new_engine(pkg, n, plan)
    eng.set_variants_matrix(M)
    eng.load_genotypes_host(0, T.pack_2bit(genotype_rows(n)), pkg.LDP_GENO_REF)
    eng.set_option("compact_batch_rows", BATCH)
    return eng


def kept_positions(plan, keep):
    chr_idx, bps = positions(plan)
    return chr_idx[keep], (None if bps is None else bps[keep])


def fresh_engine(pkg, n, plan, keep):
    eng = new_engine(pkg, n, plan)
    chr_idx, bps = kept_positions(plan, keep)
    eng.set_variants(chr_idx, bps)
    if keep.any():
        eng.load_genotypes_host(0, T.pack_2bit(genotype_rows(n)[keep]), pkg.LDP_GENO_REF)
    return eng


def state_of(pkg, eng, kept_ct):
    """everything the issue compares: records, frequencies, planes of the owned variants, the prune bitmap, every decision, the counters"""
    owned = np.zeros(kept_ct, dtype=bool)
    for length, first in eng.subcontigs():
        owned[first:first + length] = True
    planes = [eng.planes(int(v)) for v in np.where(owned)[0]]
    recs = eng.variant_recs().copy()
    mf = eng.maj_freqs().copy()
    removed = eng.run()
    pred, outside = eng.last_pred(with_outside=True)
    return {"owned": owned, "planes": planes, "recs": recs, "mf": mf, "removed": removed, "pred": pred, "outside": outside, "ctr": eng.counters(),
            "band": eng.band()}


def assert_same_state(got, want, what):
    assert np.array_equal(got["owned"], want["owned"]), what
    assert got["recs"].tobytes() == want["recs"].tobytes(), what
    assert got["mf"].tobytes() == want["mf"].tobytes(), what
    assert len(got["planes"]) == len(want["planes"])
    for v, (a, b) in enumerate(zip(got["planes"], want["planes"])):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (what, "planes of owned variant", v)
    assert np.array_equal(got["band"][0], want["band"][0]) and got["band"][1] == want["band"][1], what
    assert np.array_equal(got["removed"], want["removed"]), (what, int(got["removed"].sum()), int(want["removed"].sum()))
    assert np.array_equal(got["pred"], want["pred"]) and got["outside"] == 0 and want["outside"] == 0, what
    for name in ("candidate_pairs", "pred_true", "wide_tiles", "mfma_block_products", "subcontig_ct", "window_max"):
        assert got["ctr"][name] == want["ctr"][name], (what, name)


def oracle_removed(n, plan, keep):
    window, step, is_bp, r2, order, _ = PLANS[plan]
    raw = genotype_rows(n)[keep]
    kept_ct = int(keep.sum())
    if kept_ct == 0:
        return np.zeros(0, dtype=bool)
    chr_idx, bps = kept_positions(plan, keep)
    inv, mf, _ = T.oracle_prepare(raw)
    want, _ = T.oracle_indep_pairwise(inv, n, chr_idx, bps if bps is not None else np.arange(kept_ct, dtype=np.uint32), mf, window, step, is_bp, r2, order)
    return want


@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("n,plan", [(67, "count"), (513, "count"), (67, "wide"), (513, "wide"), (67, "planes"), (513, "planes")])
def test_restricted_engine_equals_a_fresh_one(gpu_pkg, n, plan, mask):
    pkg = gpu_pkg
    keep = MASKS[mask]
    kept_ct = int(keep.sum())
    what = "%s, %d founders, mask %s" % (plan, n, mask)
    eng = loaded_unplanned(pkg, n, plan)
    before = eng.variant_recs()
    # both orientations of the image occur (flags bit 3: the row is stored inverted), and rows with missing calls (in every third row only) lie among complete ones
    if plan != "planes":
        assert 0 < int(((before["flags"] >> 3) & 1).sum()) < M, what
    with_missing = (genotype_rows(n) == 3).any(axis=1)
    assert np.array_equal(((before["flags"] >> 2) & 1).astype(bool), with_missing) and 0 < int(with_missing.sum()) <= M // 3, what
    chr_idx, bps = kept_positions(plan, keep)
    eng.restrict_variants(keep, chr_idx, bps)
    assert eng.variant_ct == kept_ct
    moved = eng.compact_stats()
    got = state_of(pkg, eng, kept_ct)
    eng.close()
    ref = fresh_engine(pkg, n, plan, keep)
    want = state_of(pkg, ref, kept_ct)
    ref.close()
    assert_same_state(got, want, what)
    assert np.array_equal(got["removed"], oracle_removed(n, plan, keep)), what
    owned_ct = int(got["owned"].sum())
    if kept_ct < 2:
        assert owned_ct == 0 and not got["removed"].any() and moved["rows_compacted"] == 0, what
    # rows in front of the first dropped one stay where they are and are not touched
    first_moved = int(np.argmin(keep)) if not keep.all() else M
    expect_moved = int(got["owned"][min(first_moved, kept_ct):].sum()) if kept_ct else 0
    assert moved["rows_compacted"] == expect_moved == moved["rows_direct"] + moved["rows_bounced"], (what, moved)
    if mask == "everything":
        assert moved["rows_compacted"] == 0
    if mask == "row0":
        # every row moves by one: no batch of 16 rows ends before its first source row
        assert moved["rows_bounced"] == M - 1 and moved["rows_direct"] == 0, moved
    if mask == "run40":
        # 40 rows dropped in front: every batch of 16 lies wholly below its sources
        assert moved["rows_direct"] == M - 140 and moved["rows_bounced"] == 0, moved
    if mask == "random":
        assert moved["rows_direct"] > 0 and moved["rows_bounced"] > 0, moved
    if plan == "wide" and mask in ("everything", "row0", "run40", "random"):
        assert got["ctr"]["wide_tiles"] > 0 and got["ctr"]["route_complete_launches"] + got["ctr"]["route_sparse_launches"] + got["ctr"]["route_general_launches"] > 0, what
    if plan == "planes":
        assert got["ctr"]["mfma_block_products"] == 0, what
    if plan == "count" and kept_ct > 2:
        assert got["ctr"]["candidate_pairs"] > 0 and got["ctr"]["wide_tiles"] == 0, what


@pytest.mark.parametrize("n,plan", [(67, "count"), (513, "wide"), (513, "planes")])
def test_restricting_twice_equals_once_by_the_intersection(gpu_pkg, n, plan):
    pkg = gpu_pkg
    rng = np.random.default_rng(11)
    first = rng.random(M) < 0.7
    first[:20] = True                        # a prefix that stays in place the first time ...
    second = rng.random(int(first.sum())) < 0.6
    second[5] = False                        # ... and moves the second time
    both = np.zeros(M, dtype=bool)
    both[np.where(first)[0][second]] = True
    eng = loaded_unplanned(pkg, n, plan)
    eng.restrict_variants(first, *kept_positions(plan, first))
    eng.restrict_variants(second, *kept_positions(plan, both))
    twice = state_of(pkg, eng, int(both.sum()))
    eng.close()
    eng = loaded_unplanned(pkg, n, plan)
    eng.restrict_variants(both, *kept_positions(plan, both))
    once = state_of(pkg, eng, int(both.sum()))
    eng.close()
    assert_same_state(twice, once, plan)
    assert np.array_equal(once["removed"], oracle_removed(n, plan, both))


def test_preferred_bits_and_caller_frequencies_follow_their_variants(gpu_pkg):
    pkg = gpu_pkg
    n, plan = 67, "count"
    keep = MASKS["random"]
    pref = np.zeros(M, dtype=bool)
    pref[::7] = True
    freqs = np.linspace(0.5, 0.99, M)
    eng = loaded_unplanned(pkg, n, plan)
    eng.set_preferred(pref)
    eng.set_maj_freqs(300, freqs[300:])
    eng.restrict_variants(keep, *kept_positions(plan, keep))
    got_mf, got = eng.maj_freqs().copy(), eng.run()
    eng.close()
    ref = fresh_engine(pkg, n, plan, keep)
    ref.set_preferred(pref[keep])
    first_late = int(keep[:300].sum())
    ref.set_maj_freqs(first_late, freqs[300:][keep[300:]])
    want_mf, want = ref.maj_freqs().copy(), ref.run()
    ref.close()
    assert got_mf.tobytes() == want_mf.tobytes() and np.array_equal(got, want)


def test_state_and_shard_errors(gpu_pkg):
    pkg = gpu_pkg
    n, plan = 67, "count"
    keep = MASKS["random"]
    chr_idx, bps = positions(plan)
    packed = T.pack_2bit(genotype_rows(n))
    # pair work has been queued: a windowed engine after ldp_run()
    eng = new_engine(pkg, n, plan)
    eng.set_variants(chr_idx, bps)
    eng.load_genotypes_host(0, packed, pkg.LDP_GENO_REF)
    eng.run()
    with pytest.raises(pkg.LdpError) as err:
        eng.restrict_variants(keep, *kept_positions(plan, keep))
    assert err.value.code == pkg.LDP_ERR_STATE
    assert eng.variant_ct == M and len(eng.run()) == M      # nothing was changed
    eng.close()
    # rows missing
    eng = new_engine(pkg, n, plan)
    eng.set_variants_matrix(M)
    eng.load_genotypes_host(0, packed[:M // 2], pkg.LDP_GENO_REF)
    with pytest.raises(pkg.LdpError) as err:
        eng.restrict_variants(keep, *kept_positions(plan, keep))
    assert err.value.code == pkg.LDP_ERR_STATE
    eng.close()
    # a sharded engine
    eng = new_engine(pkg, n, plan)
    eng.set_variants(chr_idx, bps)
    eng.set_shard(0, 2)
    with pytest.raises(pkg.LdpError) as err:
        eng.restrict_variants(keep, *kept_positions(plan, keep))
    assert err.value.code == pkg.LDP_ERR_UNSUPPORTED
    eng.close()
    # a bitmap that does not hold kept_ct bits
    eng = loaded_unplanned(pkg, n, plan)
    L = pkg.lib()
    import ctypes
    words = np.zeros(M // 64 + 2, dtype=np.uint64)
    words[0] = 0xff
    c = np.zeros(9, dtype=np.uint32)
    assert L.ldp_restrict_variants(eng._h, words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 9, c.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), None) == pkg.LDP_ERR_INVALID
    eng.restrict_variants(keep, *kept_positions(plan, keep))    # ... and the engine is still usable
    assert np.array_equal(eng.run(), oracle_removed(n, plan, keep))
    eng.close()
