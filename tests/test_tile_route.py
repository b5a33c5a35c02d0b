"""Per-tile routing (option "tile_route"): prune launches on the 8 x 8 tile plan give every tile the kernel its OWN rows call for
-- the complete-data body, the SPARSE tiles, the quarter tiles --, never above the launch group's route word.

Every case runs the production kernels through test_pair_decisions.decide(): every candidate pair's decision against the float64 reference,
pred_true == the number of set bits (a corner pair decided twice shows here), no bit outside the band, the prune set against the oracle.  On
top of that the class the device gave every tile (LdPruneEngine.tile_classes()) must equal tile_route_tools.expected_classes(), a numpy
restatement of the rule from the plan and the rows' missing counts.

Shapes: tiles are 256 x 256 rows; ~2,000 rows on one chromosome plus a second one, a count window of 600 (distance-1 and far tiles), n = 700
(no checkpoint) and once n = 6,000 (checkpoints retire whole waves next to tiles of another class)."""
import numpy as np
import pytest

import ldtools as T
import tile_route_tools as R
from test_pair_decisions import Reference, decide

pytestmark = pytest.mark.gpu

WINDOW, R2 = R.WINDOW, 0.2
_REFS = {}


def reference(pkg, key, build):
    """the rows of a layout and their float64 reference; computed once per session for the shared layouts and never changed"""
    if key in _REFS:
        return _REFS[key]
    raw, chr_idx = build()
    ref = Reference(pkg, raw, chr_idx, None, WINDOW, 1, False, R2, 2)
    ref.miss = R.missing_per_row(raw)
    if key[0] == "three":   # (the rows several tests share; a reference holds ~60 MB of pair statistics, so the others are not kept)
        _REFS[key] = ref
    return ref


def word_of(c):
    """the ONE route word of the run's launches (wide-plan engines have one launch group; asserted)"""
    by_route = [c["route_complete_launches"], c["route_sparse_launches"], c["route_general_launches"]]
    assert sum(1 for x in by_route if x) == 1, by_route
    return int(np.argmax(by_route))


def routed(pkg, ref, options, word=None, allow_sparse=True, corner=True, loads=None, label=""):
    """decide() + the classes; returns (counters, classes, tile_routes)"""
    cap = R.CapturingPkg(pkg)
    c = decide(cap, ref, options, None, loads=loads, label=label)
    rec = cap.captured[-1]
    assert rec["classes"] is not None, (label, "per-tile routing was not active", rec)
    if word is not None:
        assert word_of(c) == word, (label, c)
    want = R.expected_classes(rec["plan"], ref.miss, ref.n, word_of(c), allow_sparse=allow_sparse, corner=corner)
    got = rec["classes"]
    print("tiles %d: complete/sparse/general %s, corners %d (%s)" % (len(got), [int(((got & 3) == k).sum()) for k in range(3)], int(((got & 4) != 0).sum()), label))
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (label, [(int(i), rec["plan"][i].tolist(), int(got[i]), int(want[i])) for i in bad[:8]])
    assert rec["routes"] == R.class_counts(want), (label, rec["routes"], R.class_counts(want))
    assert c["wide_tiles"] == len(got) > 0
    return c, got, rec


# ---------------------------------------------------------------- 1. three classes in one group
def three_class_rows(n):
    # 300 rows at 5 % (high rows: 12 % of all rows -> the group word is general), 100 rows at 0.1 % far behind them
    return R.stretch_rows(2000, n, seed=4100 + n, stretches=[(300, 600, 0.05), (1400, 1500, 0.001)], second=300)


@pytest.mark.parametrize("n", [700, 6000])
def test_three_classes_in_one_group(gpu_pkg, n):
    ref = reference(gpu_pkg, ("three", n), lambda: three_class_rows(n))
    c, got, rec = routed(gpu_pkg, ref, {}, word=R.GENERAL, label="three classes n=%d" % n)
    assert c["route_general_launches"] > 0 and c["four_tile_launches"] == c["route_general_launches"]
    assert rec["routes"]["tiles_complete"] > 0 and rec["routes"]["tiles_sparse"] > 0 and rec["routes"]["tiles_general"] > 0
    assert rec["routes"]["corner_products"] > 0
    if n >= 6000:
        assert c["mfma_skipped_product_stages"] > 0


# ---------------------------------------------------------------- 2. the corner
CORNER_T = 4   # the J tile whose diagonal tile / distance-1 tile the placements are about


def corner_rows(place):
    m, n = 2000, 700
    raw, chr_idx = R.stretch_rows(m, n, seed=4207, stretches=[], second=300)
    if place == "front32":
        rng = np.random.default_rng(5)
        part = raw[R.TILE * CORNER_T - 32:R.TILE * CORNER_T]
        part[rng.random(part.shape) < 0.05] = 3
        raw[R.TILE * CORNER_T - 32:R.TILE * CORNER_T] = part
    else:
        row = {"last_in_front": R.TILE * CORNER_T - 1, "first_row": R.TILE * CORNER_T, "j_block_1": R.TILE * CORNER_T + 32 + 5,
               "far_only": R.TILE * (CORNER_T - 2) + 100}[place]
        raw[row, 123] = 3
    return raw, chr_idx


# (diagonal tile of J tile CORNER_T: class, taken; its distance-1 tile: class, given) with the corner hand-over on
CORNER_EXPECT = {
    "last_in_front": ((R.COMPLETE, False), (R.SPARSE, False)),   # a row of V block 7 of the distance-1 tile only
    "first_row": ((R.SPARSE, False), (R.SPARSE, False)),
    "j_block_1": ((R.SPARSE, False), (R.SPARSE, False)),
    "far_only": ((R.COMPLETE, True), (R.COMPLETE, True)),        # only (t, t - 2) and the tiles of J tile t - 2 read the row
    "front32": ((R.COMPLETE, False), (R.SPARSE, False)),         # 32 rows at 5 %: 6 % of the tile's rows are high rows, the word (sparse) caps the class
}


@pytest.mark.parametrize("place", list(CORNER_EXPECT))
def test_the_corner_product_changes_hands_only_between_two_complete_tiles(gpu_pkg, place):
    ref = reference(gpu_pkg, ("corner", place), lambda: corner_rows(place))
    for options, corner in (({}, True), ({"wide_diag_corner": 0}, False), ({"wide_diag_kernel": 0}, False)):
        c, got, rec = routed(gpu_pkg, ref, options, word=R.SPARSE, corner=corner, label="corner/%s %s" % (place, options))
        plan = rec["plan"]
        jv = R.TILE * CORNER_T
        diag = [i for i, t in enumerate(plan) if t[0] == jv and t[1] == jv]
        dist1 = [i for i, t in enumerate(plan) if t[0] == jv and t[1] == jv - R.TILE]
        assert len(diag) == 1 and len(dist1) == 1
        (dcls, taken), (ncls, given) = CORNER_EXPECT[place]
        assert (int(got[diag[0]]) & 3, bool(got[diag[0]] & R.TAKEN)) == (dcls, taken and corner), (place, options, int(got[diag[0]]))
        assert (int(got[dist1[0]]) & 3, bool(got[dist1[0]] & R.GIVEN)) == (ncls, given and corner), (place, options, int(got[dist1[0]]))
        assert not (got[diag[0]] & R.GIVEN) and not (got[dist1[0]] & R.TAKEN)
        if corner:
            assert rec["routes"]["corner_products"] > 0    # the other J tiles still hand theirs over
        else:
            assert rec["routes"]["corner_products"] == 0


# ---------------------------------------------------------------- 3. first rows only
@pytest.mark.parametrize("miss,route", [(0.001, "route_sparse_launches"), (0.05, "route_general_launches")])
def test_missing_calls_on_the_first_chromosome_leave_the_second_on_the_complete_body(gpu_pkg, miss, route):
    m1, m2 = 1200, 800
    ref = reference(gpu_pkg, ("first", miss), lambda: R.stretch_rows(m1, 700, seed=4300, stretches=[(0, m1, miss)], second=m2))
    c, got, rec = routed(gpu_pkg, ref, {}, label="first rows %g" % miss)
    # the group counters, as test_missing_calls_in_the_first_rows_take_every_group_off_the_complete_route expects them
    assert c["route_complete_launches"] == 0 and c[route] > 0
    later = np.array([int(t[0]) >= m1 for t in rec["plan"]])
    assert later.sum() > 4 and (~later).sum() > 4
    assert ((got[later] & 3) == R.COMPLETE).all()
    assert ((got[~later] & 3) != R.COMPLETE).all()


# ---------------------------------------------------------------- 4. the switch
# counters() of the parent commit (no per-tile routing) over three_class_rows(700), default options, recorded on an MI355X: tests/golden/tile_route_parent_counters.json
TIMES = ("ms_prepare", "ms_pair_kernel", "ms_pair_fast", "ms_pair_general", "ms_replay", "ms_run_total", "ms_pair_mfma", "ms_pair_mfma_general")


def test_the_switch(gpu_pkg):
    import json
    import os
    ref = reference(gpu_pkg, ("three", 700), lambda: three_class_rows(700))
    cap = R.CapturingPkg(gpu_pkg)
    c0 = decide(cap, ref, {"tile_route": 0}, None, label="switch off")
    rec = cap.captured[-1]
    assert rec["routes"] == {"tiles_complete": 0, "tiles_sparse": 0, "tiles_general": 0, "corner_products": 0}
    assert rec["classes"] is None and rec["classes_error"] == gpu_pkg.LDP_ERR_STATE
    assert c0["route_general_launches"] > 0 and c0["four_tile_launches"] == c0["route_general_launches"]
    parent = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tile_route_parent_counters.json")))
    for k, v in c0.items():
        if k not in TIMES:
            assert v == parent[k], ("option 0 against the parent", k, v, parent[k])
    # the quarter tiles off: the tile plan does not cover the general route -> inactive, all zero
    c = decide(cap, ref, {"pair_four_tiles": 0}, None, label="pair_four_tiles 0")
    rec = cap.captured[-1]
    assert rec["classes"] is None and not any(rec["routes"].values()) and c["four_tile_launches"] == 0
    # the sparse route off: complete and general tiles only
    c, got, rec = routed(gpu_pkg, ref, {"pair_sparse": 0}, word=R.GENERAL, allow_sparse=False, label="pair_sparse 0")
    assert rec["routes"]["tiles_sparse"] == 0 and rec["routes"]["tiles_complete"] > 0 and rec["routes"]["tiles_general"] > 0
    assert c["sparse_exact_pairs"] >= 0
    # the SPARSE tiles off while the sparse route is on: a sparse word would meet the parallelogram plan -> inactive
    c = decide(cap, ref, {"wide_sparse": 0}, None, label="wide_sparse 0")
    assert cap.captured[-1]["classes"] is None and not any(cap.captured[-1]["routes"].values())


# ---------------------------------------------------------------- 5. resident records
def test_classes_follow_the_resident_rows(gpu_pkg):
    pkg = gpu_pkg
    ref = reference(pkg, ("three", 700), lambda: three_class_rows(700))
    # loaded in three uneven calls: the group is launched from inside the last one (launch_ready_groups)
    routed(pkg, ref, {}, word=R.GENERAL, loads=[(0, 701), (701, 1750), (1750, ref.m)], label="eager launch")
    # ... then the incomplete stretches are re-loaded with complete rows, on the same engine
    raw2 = ref.raw.copy()
    fill = T.synth_raw_codes(ref.m, ref.n, seed=99, missing_rate=0.0, ld_copy_prob=0.6, redraw=0.1)
    for a, b in ((300, 600), (1400, 1500)):
        raw2[a:b] = fill[a:b]
    assert not (raw2 == 3).any()
    ref2 = reference(pkg, ("three-completed", 700), lambda: (raw2, ref.chr_idx))
    eng = pkg.LdPruneEngine(ref.n, WINDOW, 1, False, R2, order=2, device=0)
    eng.set_variants(ref.chr_idx, None)
    eng.load_genotypes_host(0, ref.packed, pkg.LDP_GENO_REF)
    removed = eng.run()
    assert np.array_equal(removed, ref.removed)
    first = eng.tile_classes()
    assert len(set((first & 3).tolist())) == 3
    for a, b in ((300, 600), (1400, 1500)):
        eng.load_genotypes_host(a, ref2.packed[a:b], pkg.LDP_GENO_REF)
    removed = eng.run()
    pred, outside = eng.last_pred(with_outside=True)
    c = eng.counters()
    nd, msg = T.compare_decisions(pred, ref2.dec, ref2.lo, ref2.stats, R2, counters=c)
    assert nd == 0, msg
    assert int(pred.sum()) == c["pred_true"] and outside == 0 and np.array_equal(removed, ref2.removed)
    assert c["route_complete_launches"] > 0 and c["route_sparse_launches"] == 0 and c["route_general_launches"] == 0
    second = eng.tile_classes()
    want = R.expected_classes(eng.debug_wide_plan(), ref2.miss, ref.n, R.COMPLETE)
    assert np.array_equal(second, want) and ((second & 3) == R.COMPLETE).all()
    tr = eng.tile_routes()
    assert tr["tiles_complete"] == len(second) and tr["tiles_sparse"] == 0 and tr["tiles_general"] == 0 and tr["corner_products"] > 0
    eng.close()


# ---------------------------------------------------------------- 6. randomised layouts
@pytest.mark.parametrize("seed", R.RANDOM_SEEDS)
def test_random_stretches(gpu_pkg, seed):
    raw, chr_idx, _ = R.random_layout(seed)
    ref = reference(gpu_pkg, ("random", seed), lambda: (raw, chr_idx))
    routed(gpu_pkg, ref, {}, label="random %d" % seed)
