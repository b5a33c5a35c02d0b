"""The compacted predicate rows a production run hands its replay, on the device.

pred_compact_kernel (csrc/ldp_pred_csr.hip) turns each launch group's dense predicate rows into CSR -- meta[j] = (first entry, entries) of row
j, an entry = (word index inside the row, bits) -- in pinned host memory; the replay of ldp_run() reads nothing else.
ldp_debug_get_pred_csr() (LdPruneEngine.last_pred_csr) hands out what it read.  The reference is the numpy compaction of the DENSE rows of
the same run: every row's words rebuilt from last_pred(with_outside=True) (a plain copy of d_pred that shares nothing with the kernel) and
the window starts, with no bit outside the band.  All comparisons are equalities of integers and bits.  For every engine:
  (a) the decisions rebuilt from (meta, ent) equal last_pred() for every candidate pair;
  (b) in every row the entries' word indices ascend strictly and are smaller than the row's word count;
  (c) no entry has bits == 0, none has a bit outside the band;
  (d) meta[j].y == 0 for rows with j <= lo[j];
  (e) the ranges [x, x + y) of the rows with entries are pairwise disjoint and tile [0, used) exactly -- in whatever order the blocks landed;
  (f) used == the device's counter == the number of non-zero dense words;
  (g) the overflow flag and the count of runs that fell back are 0 unless the case forces the fallback;
  (h) run()'s removed set equals that of a "pred_csr" 0 engine over the same input and debug_replay_pairs() of the last_pred() decisions."""
import ctypes
import functools

import numpy as np
import pytest

import ldtools as T
from test_host_logic import make_positions

pytestmark = pytest.mark.gpu

TOTALS = {"rows": 0, "entries": 0, "pairs": 0, "engines": 0}


# ---------------------------------------------------------------- the numpy side
def local_band(eng):
    """(lo, pair_off, word count per row, local -> global variant) in the engine's local row indices (the variants of its subcontigs, in order)"""
    _, lo = eng.debug_mfma_plan()
    lo = lo.astype(np.int64)
    j = np.arange(len(lo), dtype=np.int64)
    has = j > lo
    nw = np.where(has, ((j - 1) >> 5) - (lo >> 5) + 1, 0)
    pair_off = np.concatenate([[0], np.cumsum(np.where(has, j - lo, 0))])
    subs = eng.subcontigs()
    to_global = np.concatenate([np.arange(f0, f0 + ln, dtype=np.int64) for ln, f0 in subs]) if subs else np.zeros(0, dtype=np.int64)
    assert len(to_global) == len(lo)
    return lo, pair_off, nw, to_global


def true_pairs(pred, lo, pair_off):
    """(first, second) local indices of the set decisions of a band-order decision array"""
    idx = np.flatnonzero(pred)
    second = np.searchsorted(pair_off, idx, side="right") - 1
    return lo[second] + idx - pair_off[second], second


def compact(pred, lo, pair_off):
    """the specification: per row its non-zero words, ascending -- (row, word index, bits), sorted by row then word"""
    first, second = true_pairs(pred, lo, pair_off)
    word = (first >> 5) - (lo[second] >> 5)
    key, inverse = np.unique(second * (1 << 20) + word, return_inverse=True)
    bits = np.zeros(len(key), dtype=np.int64)
    np.add.at(bits, inverse, np.int64(1) << (first & 31))   # (distinct bits of one word: a sum is their union)
    return key >> 20, key & ((1 << 20) - 1), bits


def in_band_mask(row, word, lo):
    """the bits of word `word` of row `row` that are candidate pairs: firsts lo[row] <= i < row"""
    base = ((lo[row] >> 5) + word) << 5
    a = np.clip(lo[row] - base, 0, 32)
    b = np.clip(row - base, 0, 32)
    return ((np.int64(1) << b) - 1) & ~((np.int64(1) << a) - 1)


def check_csr(eng, label, overflow_runs=0, removed=None):
    """(a)-(g) on the engine's last run, (h) against debug_replay_pairs of its own decisions and, where given, against `removed` of another
    engine; returns (csr, pred)"""
    pred, outside = eng.last_pred(with_outside=True)
    assert outside == 0, (label, outside)
    csr = eng.last_pred_csr()
    lo, pair_off, nw, to_global = local_band(eng)
    rows = len(lo)
    meta, ent = csr["meta"].astype(np.int64), csr["ent"].astype(np.int64)
    assert meta.shape == (rows, 2) and len(pred) == pair_off[-1] == eng.counters()["candidate_pairs"], label
    want_row, want_word, want_bits = compact(pred, lo, pair_off)
    print("%s: %d rows, %d entries, %d candidate pairs (%d true); capacity %d" % (label, rows, csr["used"], len(pred), int(pred.sum()), csr["capacity"]))
    assert csr["overflow"] == 0 and csr["overflow_runs"] == overflow_runs, (label, csr["overflow"], csr["overflow_runs"])       # (g)
    assert csr["used"] == csr["device_count"] == len(want_row) == len(ent), (label, csr["used"], csr["device_count"], len(want_row))  # (f)
    assert not meta[np.arange(rows) <= lo, 1].any(), label                                                                   # (d)
    # (e): sorted by their first entry, the rows' runs follow one another from 0 to used
    owners = np.flatnonzero(meta[:, 1])
    owners = owners[np.argsort(meta[owners, 0], kind="stable")]
    start, count = meta[owners, 0], meta[owners, 1]
    assert np.array_equal(start, np.cumsum(count) - count) and int(count.sum()) == csr["used"], label
    # entry -> its row; then row by row in the order the entries lie
    row_of = np.repeat(owners, count)
    order = np.argsort(row_of, kind="stable")
    got_row, got_word, got_bits = row_of[order], ent[order, 0], ent[order, 1]
    same_row = got_row[1:] == got_row[:-1]
    assert np.all(got_word[1:][same_row] > got_word[:-1][same_row]) and np.all(got_word < nw[got_row]), label              # (b)
    assert np.all(got_bits != 0) and not np.any(got_bits & ~in_band_mask(got_row, got_word, lo)), label                      # (c)
    # (a): every candidate pair's decision from the entries
    rebuilt = np.zeros(len(pred), dtype=bool)
    for b in range(32):
        sel = ((got_bits >> b) & 1) == 1
        first = (((lo[got_row[sel]] >> 5) + got_word[sel]) << 5) + b
        rebuilt[pair_off[got_row[sel]] + first - lo[got_row[sel]]] = True
    assert np.array_equal(rebuilt, pred), (label, int(rebuilt.sum()), int(pred.sum()), int((rebuilt != pred).sum()))
    assert np.array_equal(got_row, want_row) and np.array_equal(got_word, want_word) and np.array_equal(got_bits, want_bits), label
    assert np.array_equal(np.bincount(want_row, minlength=rows), meta[:, 1]), label
    TOTALS["rows"] += rows
    TOTALS["entries"] += csr["used"]
    TOTALS["pairs"] += len(pred)
    TOTALS["engines"] += 1
    return csr, pred


def replayed_on_the_host(eng, pred):
    """debug_replay_pairs() of a run's own decisions (the dense host replay; the engine holds the run's records and frequencies)"""
    lo, pair_off, _, to_global = local_band(eng)
    first, second = true_pairs(pred, lo, pair_off)
    return eng.debug_replay_pairs(to_global[first], to_global[second])


def new_engine(pkg, data, options=None, order=2, load=True):
    eng = pkg.LdPruneEngine(data["n"], data["window"], data["step"], data["is_bp"], data["r2"], order=order, device=0)
    for name, value in (options or {}).items():
        eng.set_option(name, value)
    eng.set_variants(data["chr_idx"], data["bps"])
    if load:
        eng.load_genotypes_host(0, data["packed"], pkg.LDP_GENO_REF)
    return eng


def run_and_check(pkg, eng, label, dense_removed=None, overflow_runs=0):
    removed = eng.run()
    csr, pred = check_csr(eng, label, overflow_runs)
    assert np.array_equal(replayed_on_the_host(eng, pred), removed), (label, "host replay of the run's decisions")            # (h)
    if dense_removed is not None:
        assert np.array_equal(removed, dense_removed), (label, int(removed.sum()), int(dense_removed.sum()))
    return removed, csr, pred


@functools.lru_cache(maxsize=None)
def dense_engine_removed(pkg, key, order=2):
    """the removed set of a "pred_csr" 0 engine over a fixture (one run per fixture and order)"""
    eng = new_engine(pkg, FIXTURES[key](), {"pred_csr": 0}, order)
    removed = eng.run()
    with pytest.raises(pkg.LdpError) as ei:
        eng.last_pred_csr()                       # the dense rows were copied back: there is no CSR to hand out
    assert ei.value.code == pkg.LDP_ERR_STATE
    eng.close()
    return removed


# ---------------------------------------------------------------- fixtures
PLANTED_M, PLANTED_N, PLANTED_WINDOW = 6000, 130, 4200
PLANTED_SINGLES = ((5600, 0), (5603, 63), (5606, 64), (5609, 131))   # (row, word of the row its one set bit falls in)


def _fresh_row(rng, n):
    maf = rng.uniform(0.2, 0.5)
    return ((rng.random(n) < maf).astype(np.uint8) + (rng.random(n) < maf).astype(np.uint8)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def planted_rows(m=PLANTED_M, n=PLANTED_N):
    """Independent rows (no pair passes r^2 > 0.5 but by chance) with three plants, under a count window of 4,200 and step 1:
    family A, 140 copies of one row at rows 100 + 32 k -- a member's row holds one bit in (nearly) every word, up to 131 entries;
    family B, rows 5000-5199 identical -- full words; four rows with ONE entry each, in word 0, 63, 64 and the last word (131)."""
    rng = np.random.default_rng(5)
    raw = T.synth_raw_codes(m, n, seed=5, missing_rate=0.0, ld_copy_prob=0.0, maf_lo=0.2)
    fam_a = 100 + 32 * np.arange(140)
    raw[fam_a] = _fresh_row(rng, n)
    raw[5000:5200] = _fresh_row(rng, n)
    taken = set(fam_a.tolist()) | set(range(5000, 5200)) | {j for j, _ in PLANTED_SINGLES}
    copies = []
    for j, word in PLANTED_SINGLES:
        raw[j] = _fresh_row(rng, n)
        lo = j - (PLANTED_WINDOW - 1)
        base = ((lo >> 5) + word) << 5
        i = next(i for i in range(max(base, lo), min(base + 32, j)) if i not in taken)
        taken.add(i)
        raw[i] = raw[j]
        copies.append(i)
    return {"raw": raw, "packed": T.pack_2bit(raw), "n": n, "m": m, "window": PLANTED_WINDOW, "step": 1, "is_bp": False, "r2": 0.5,
            "chr_idx": np.zeros(m, dtype=np.uint32), "bps": None, "copies": copies}


@functools.lru_cache(maxsize=None)
def independent_rows(m=PLANTED_M, n=PLANTED_N):
    raw = T.synth_raw_codes(m, n, seed=6, missing_rate=0.0, ld_copy_prob=0.0, maf_lo=0.2)
    return dict(planted_rows(), raw=raw, packed=T.pack_2bit(raw), copies=None)


@functools.lru_cache(maxsize=None)
def ragged_groups(m=20011, n=130):
    """more than 512 work items (a second launch group) and a row count that is no multiple of 64; kb windows over three chromosomes"""
    raw = T.synth_raw_codes(m, n, seed=77, missing_rate=0.0, ld_copy_prob=0.7, redraw=0.1)
    chr_idx, bps = make_positions(m, 3, 11)
    return {"raw": raw, "packed": T.pack_2bit(raw), "n": n, "m": m, "window": 30000, "step": 1, "is_bp": True, "r2": 0.3, "chr_idx": chr_idx, "bps": bps}


@functools.lru_cache(maxsize=None)
def eager_groups(m=20000, n=130):
    """two launch groups under a count window of 80 (tests/test_pair_decisions.py: the cut lies near row 16,400); the rows from 18,000 on miss
    5 % of their calls, so that group 0 -- routed from the rows below its need_end -- stays on the complete-data route"""
    raw = T.synth_raw_codes(m, n, seed=2026, missing_rate=0.0, ld_copy_prob=0.6, redraw=0.1)
    part = raw[18000:]
    part[np.random.default_rng(50001).random(part.shape) < 0.05] = 3
    raw[18000:] = part
    return {"raw": raw, "packed": T.pack_2bit(raw), "n": n, "m": m, "window": 80, "step": 1, "is_bp": False, "r2": 0.2,
            "chr_idx": np.repeat(np.arange(2, dtype=np.uint32), m // 2), "bps": None}


FIXTURES = {"planted": planted_rows, "ragged": ragged_groups, "eager": eager_groups}


def test_the_planted_rows_are_what_they_are_meant_to_be():
    """the fixture's conditions from the numpy side alone, no engine: r^2 of every candidate pair restated in float64 (the rows are complete:
    the squared correlation of the codes), which decides r^2 > 0.5 as long as no pair comes within 1e-6 of the threshold -- asserted"""
    data = planted_rows()
    m, n = data["m"], data["n"]
    lo = np.maximum(np.arange(m, dtype=np.int64) - (PLANTED_WINDOW - 1), 0)   # count window w, step 1: variant j meets the w - 1 before it
    j = np.arange(m, dtype=np.int64)
    pair_off = np.concatenate([[0], np.cumsum(j - lo)])
    z = data["raw"].astype(np.float64)
    z -= z.mean(axis=1, keepdims=True)
    z /= np.sqrt((z * z).sum(axis=1, keepdims=True))
    dec = []
    for j0 in range(0, m, 512):
        j1 = min(m, j0 + 512)
        i0 = int(lo[j0])
        r2 = (z[j0:j1] @ z[i0:j1].T) ** 2
        i = np.arange(i0, j1)[None, :]
        band = (i >= lo[j0:j1, None]) & (i < j[j0:j1, None])
        assert not (np.abs(r2[band] - data["r2"]) < 1e-6).any()
        dec.append(r2[band] > data["r2"])       # (row-major over the block: second variant ascending, first ascending -- band order)
    dec = np.concatenate(dec)
    assert len(dec) == pair_off[-1]
    row, word, bits = compact(dec, lo, pair_off)
    per_row = np.bincount(row, minlength=m)
    nw = np.where(j > lo, ((j - 1) >> 5) - (lo >> 5) + 1, 0)
    print("planted rows: %d above 128 words, %d above 64, maximum %d of %d; %d full words; %d of %d rows non-empty"
          % ((per_row > 128).sum(), (per_row > 64).sum(), per_row.max(), nw.max(), (bits == 0xffffffff).sum(), (per_row > 0).sum(), m))
    assert (per_row > 128).sum() >= 1 and (per_row > 64).sum() >= 50
    for (jj, want_word), i in zip(PLANTED_SINGLES, data["copies"]):
        assert per_row[jj] == 1 and word[row == jj][0] == want_word and bits[row == jj][0] == 1 << (i & 31), (jj, want_word, i)
    assert nw[PLANTED_SINGLES[3][0]] == PLANTED_SINGLES[3][1] + 1      # 131 is that row's last word
    assert (bits == 0xffffffff).sum() >= 20
    assert (per_row == 0).sum() >= 0.9 * m
    PLANTED_NUMPY["dec"] = dec


PLANTED_NUMPY = {}


# ---------------------------------------------------------------- 1. rows of up to 132 words, on each plan
@functools.lru_cache(maxsize=None)
def planted_default_run(pkg):
    """(removed, used, decisions) of the default engine over planted_rows, checked"""
    eng = new_engine(pkg, planted_rows())
    removed, csr, pred = run_and_check(pkg, eng, "planted/default", dense_engine_removed(pkg, "planted"))
    c = eng.counters()
    eng.close()
    assert c["wide_tiles"] > 0, "a band of 131 row-blocks takes the 8 x 8 tile plan"
    per_row = csr["meta"][:, 1]
    assert per_row.max() > 128 and (per_row > 64).sum() >= 50 and csr["ent"][:, 0].max() >= 131   # (132 in a row whose firsts straddle 133 words)
    for j, word in PLANTED_SINGLES:
        assert per_row[j] == 1 and csr["ent"][csr["meta"][j, 0], 0] == word
    if "dec" in PLANTED_NUMPY:
        assert np.array_equal(pred, PLANTED_NUMPY["dec"]), "the run's decisions are not the numpy side's"
    return removed, csr["used"], pred


def test_planted_rows_on_the_tiles(gpu_pkg):
    planted_default_run(gpu_pkg)


@pytest.mark.parametrize("options,mfma", [({"wide_min_reach": 1e9}, True), ({"pair_mfma": 0}, False)])
def test_planted_rows_on_the_other_plans(gpu_pkg, options, mfma):
    """the parallelogram plan of the matrix-pipe kernels, and the popcount kernels: the same rows reach the compaction"""
    pkg = gpu_pkg
    removed0, used0, pred0 = planted_default_run(pkg)
    eng = new_engine(pkg, planted_rows(), options)
    removed, csr, pred = run_and_check(pkg, eng, "planted/%s" % options, dense_engine_removed(pkg, "planted"))
    c = eng.counters()
    eng.close()
    assert c["wide_tiles"] == 0 and (c["mfma_block_products"] > 0) == mfma, (c["wide_tiles"], c["mfma_block_products"])
    assert csr["used"] == used0 and np.array_equal(pred, pred0) and np.array_equal(removed, removed0)


# ---------------------------------------------------------------- 2. several launch groups, a ragged end, a second run
@pytest.mark.parametrize("order", [2, 1])
def test_several_launch_groups_with_a_ragged_end(gpu_pkg, order):
    pkg = gpu_pkg
    data = ragged_groups()
    eng = new_engine(pkg, data, order=order)
    lo, _, _, _ = local_band(eng)
    assert len(lo) % 64 != 0
    removed, csr, pred = run_and_check(pkg, eng, "ragged/order %d" % order, dense_engine_removed(pkg, "ragged", order))
    assert eng.counters()["pair_kernel_launches"] >= 2
    assert 50 < removed.sum() < data["m"] - 50 and csr["used"] > 1000
    # a second run on the same engine writes its rows again: counter, flag and entries start over
    again, csr2, pred2 = run_and_check(pkg, eng, "ragged/order %d/second run" % order, removed)
    assert csr2["used"] == csr["used"] and np.array_equal(pred2, pred) and eng.counters()["pair_kernel_launches"] >= 2
    eng.close()


# ---------------------------------------------------------------- 3. no entry at all; nothing stale after a reload
def assert_empty(eng, label):
    removed = eng.run()
    csr, pred = check_csr(eng, label)
    assert csr["used"] == 0 and csr["device_count"] == 0 and not csr["meta"][:, 1].any() and not pred.any(), label
    return removed


def test_no_entry_at_all_then_planted_rows_and_back(gpu_pkg):
    """independent rows at r^2 > 0.99: every launch's blocks count nothing (the counter is not touched).  The same engine loaded with the
    planted rows (their copies pass any threshold): the CSR is the new dense rows'.  And the other way round: every meta[j].y is 0 again."""
    pkg = gpu_pkg
    empty, planted = dict(independent_rows(), r2=0.99), dict(planted_rows(), r2=0.99)
    eng = new_engine(pkg, empty)
    assert_empty(eng, "empty")
    eng.load_genotypes_host(0, planted["packed"], pkg.LDP_GENO_REF)
    _, csr, _ = run_and_check(pkg, eng, "empty, then planted")
    assert csr["meta"][:, 1].max() > 128
    eng.close()
    eng = new_engine(pkg, planted)
    _, csr2, _ = run_and_check(pkg, eng, "planted at 0.99")
    assert csr2["used"] == csr["used"]
    eng.load_genotypes_host(0, empty["packed"], pkg.LDP_GENO_REF)
    assert_empty(eng, "planted, then empty")
    eng.close()


# ---------------------------------------------------------------- 4. the capacity at the edge
def test_capacity_exactly_the_entries(gpu_pkg):
    pkg = gpu_pkg
    removed0, used0, pred0 = planted_default_run(pkg)
    eng = new_engine(pkg, planted_rows(), {"csr_capacity": used0})
    removed, csr, pred = run_and_check(pkg, eng, "planted/capacity = used", removed0)
    eng.close()
    assert csr["capacity"] == used0 == csr["used"] and np.array_equal(pred, pred0)


@pytest.mark.parametrize("short_by", [1, None])
def test_capacity_too_small_falls_back_to_the_dense_rows(gpu_pkg, short_by):
    """one entry short, and a capacity of 1: the flag is raised, the run is counted as one that fell back, and it gives the same set from the
    same decisions"""
    pkg = gpu_pkg
    removed0, used0, pred0 = planted_default_run(pkg)
    capacity = used0 - short_by if short_by else 1
    eng = new_engine(pkg, planted_rows(), {"csr_capacity": capacity})
    removed = eng.run()
    csr = eng.last_pred_csr()
    pred, outside = eng.last_pred(with_outside=True)
    eng.close()
    assert csr["overflow"] == 1 and csr["overflow_runs"] == 1 and csr["capacity"] == capacity, csr
    assert csr["device_count"] == used0 and csr["used"] == capacity == len(csr["ent"])
    assert outside == 0 and np.array_equal(pred, pred0) and np.array_equal(removed, removed0)


# ---------------------------------------------------------------- 5. small plans
@pytest.mark.parametrize("m", [1, 2, 33, 64, 65, 129])
def test_small_plans(gpu_pkg, m):
    """no pair, one pair; one launch group of fewer than 64 rows, exactly 64, 64 and a remainder, two blocks and a remainder"""
    pkg = gpu_pkg
    raw = T.synth_raw_codes(m, 130, seed=40 + m, missing_rate=0.0, ld_copy_prob=0.8, redraw=0.05)
    if m == 2:
        raw[1] = raw[0]          # the one pair there is passes
    data = {"raw": raw, "packed": T.pack_2bit(raw), "n": 130, "m": m, "window": 50, "step": 5, "is_bp": False, "r2": 0.2,
            "chr_idx": np.zeros(m, dtype=np.uint32), "bps": None}
    dense = new_engine(pkg, data, {"pred_csr": 0})
    want = dense.run()
    dense.close()
    eng = new_engine(pkg, data)
    removed, csr, pred = run_and_check(pkg, eng, "m = %d" % m, want)
    eng.close()
    if m <= 2:
        assert len(pred) == m - 1 == csr["used"] and removed.sum() == m - 1, (len(pred), csr["used"], int(removed.sum()))
    else:
        assert csr["used"] > 0 and len(csr["meta"]) == m


# ---------------------------------------------------------------- 6. groups launched from inside a load call
def test_groups_launched_from_inside_a_load_call(gpu_pkg):
    """rows loaded in three uneven calls: group 0 is launched -- and compacted -- from inside the second one (launch_ready_groups), group 1 by
    run().  As in tests/test_pair_decisions.py, the routes show it: group 0 was routed from the complete rows below its need_end."""
    pkg = gpu_pkg
    data = eager_groups()
    eng = new_engine(pkg, data, load=False)
    for a, b in ((0, 7001), (7001, 17500), (17500, data["m"])):
        eng.load_genotypes_host(a, data["packed"][a:b], pkg.LDP_GENO_REF)
    removed, csr, pred = run_and_check(pkg, eng, "eager launches", dense_engine_removed(pkg, "eager"))
    c = eng.counters()
    eng.close()
    assert c["pair_kernel_launches"] >= 2
    assert c["route_complete_launches"] > 0 and c["route_general_launches"] > 0
    assert c["route_complete_launches"] + c["route_general_launches"] == c["pair_kernel_launches"]
    assert csr["used"] > 1000


# ---------------------------------------------------------------- 7. a new plan after ldp_restrict_variants
def test_after_restrict_variants(gpu_pkg):
    """the rows of the ragged case loaded without a plan (ldp_restrict_variants refuses an engine that has queued pair work), restricted to
    every third variant: the plan, the rows' offsets and the CSR buffers are new, and the CSR is the restricted run's dense rows'"""
    pkg = gpu_pkg
    data = ragged_groups()
    keep = np.arange(data["m"]) % 3 == 0
    kept = dict(data, raw=data["raw"][keep], packed=np.ascontiguousarray(data["packed"][keep]), m=int(keep.sum()), chr_idx=data["chr_idx"][keep], bps=data["bps"][keep])
    dense = new_engine(pkg, kept, {"pred_csr": 0})
    want = dense.run()
    dense.close()
    eng = pkg.LdPruneEngine(data["n"], data["window"], data["step"], data["is_bp"], data["r2"], order=2, device=0)
    eng.set_variants_matrix(data["m"])
    eng.load_genotypes_host(0, data["packed"], pkg.LDP_GENO_REF)
    eng.restrict_variants(keep, kept["chr_idx"], kept["bps"])
    removed, csr, pred = run_and_check(pkg, eng, "restricted", want)
    eng.close()
    assert csr["used"] > 100 and len(csr["meta"]) <= kept["m"]


# ---------------------------------------------------------------- 8. what the getter refuses
def test_refusals_of_the_getter(gpu_pkg):
    pkg = gpu_pkg
    m = 300
    raw = T.synth_raw_codes(m, 130, seed=8, missing_rate=0.0, ld_copy_prob=0.8)
    data = {"raw": raw, "packed": T.pack_2bit(raw), "n": 130, "m": m, "window": 50, "step": 5, "is_bp": False, "r2": 0.2,
            "chr_idx": np.zeros(m, dtype=np.uint32), "bps": None}

    def refused(eng, code):
        with pytest.raises(pkg.LdpError) as ei:
            eng.last_pred_csr()
        assert ei.value.code == code

    eng = new_engine(pkg, data, load=False)
    refused(eng, pkg.LDP_ERR_STATE)                   # nothing loaded, nothing run
    eng.load_genotypes_host(0, data["packed"], pkg.LDP_GENO_REF)
    refused(eng, pkg.LDP_ERR_STATE)                   # loaded, not run
    eng.run_with_stats()
    refused(eng, pkg.LDP_ERR_STATE)                   # an inspection run copies the dense rows
    eng.run()
    csr, _ = check_csr(eng, "refusals")
    assert csr["used"] > 0
    # too-small buffers
    u32p = ctypes.POINTER(ctypes.c_uint32)
    meta = np.zeros((m, 2), dtype=np.uint32)
    ent = np.zeros((csr["used"], 2), dtype=np.uint32)
    call = pkg.lib().ldp_debug_get_pred_csr
    tail = (None,) * 6
    assert call(eng._h, meta.ctypes.data_as(u32p), m - 1, ent.ctypes.data_as(u32p), csr["used"], *tail) == pkg.LDP_ERR_INVALID
    assert call(eng._h, meta.ctypes.data_as(u32p), m, ent.ctypes.data_as(u32p), csr["used"] - 1, *tail) == pkg.LDP_ERR_INVALID
    assert not meta.any() and not ent.any()
    assert call(eng._h, meta.ctypes.data_as(u32p), m, ent.ctypes.data_as(u32p), csr["used"], *tail) == pkg.LDP_OK
    assert np.array_equal(meta, csr["meta"]) and np.array_equal(ent, csr["ent"])
    eng.load_genotypes_host(0, data["packed"][:5], pkg.LDP_GENO_REF)
    refused(eng, pkg.LDP_ERR_STATE)                   # a load invalidates the rows
    eng.close()
    eng = new_engine(pkg, data, {"pred_csr": 0})
    eng.run()
    refused(eng, pkg.LDP_ERR_STATE)                   # "pred_csr" 0
    eng.close()
    eng = new_engine(pkg, data, load=False)
    eng.set_shard(0, 2)
    refused(eng, pkg.LDP_ERR_UNSUPPORTED)             # sharded engines
    eng.close()


def test_zz_what_was_compared():
    print("compacted rows compared in this file: %d rows, %d entries, %d candidate pairs over %d engines" % (TOTALS["rows"], TOTALS["entries"], TOTALS["pairs"], TOTALS["engines"]))
    assert TOTALS["engines"] > 0 and TOTALS["entries"] > 0
