"""Per-tile routing, the parts that need no GPU: the option, the accessors' refusals, the names in header and binding, and the
numpy restatement of the class rule (tile_route_tools) on the layouts the GPU tests use."""
import ctypes
import os
import re

import numpy as np
import pytest

import tile_route_tools as R


def engine(pkg, n=700):
    return pkg.LdPruneEngine(n, R.WINDOW, 1, False, 0.2, order=2, device=0)


def test_the_option_takes_0_and_1_only(pkg):
    eng = engine(pkg)
    for v in (0, 1, 0.0, 1.0):
        eng.set_option("tile_route", v)
    for v in (2, -1, 0.5, 1e9):
        with pytest.raises(pkg.LdpError) as ei:
            eng.set_option("tile_route", v)
        assert ei.value.code == pkg.LDP_ERR_INVALID
    eng.close()


def test_a_fresh_engine_reports_no_tile_routes_and_no_classes(pkg):
    eng = engine(pkg)
    assert eng.tile_routes() == {"tiles_complete": 0, "tiles_sparse": 0, "tiles_general": 0, "corner_products": 0}
    with pytest.raises(pkg.LdpError) as ei:
        eng.tile_classes()
    assert ei.value.code == pkg.LDP_ERR_STATE
    eng.set_variants(np.zeros(2000, dtype=np.uint32), None)
    assert len(eng.debug_wide_plan()) > 0
    assert not any(eng.tile_routes().values())
    with pytest.raises(pkg.LdpError) as ei:
        eng.tile_classes()                     # planned, nothing run
    assert ei.value.code == pkg.LDP_ERR_STATE
    L = pkg.lib()
    assert L.ldp_get_tile_routes(eng._h, None) == pkg.LDP_ERR_INVALID and L.ldp_get_tile_routes(None, None) == pkg.LDP_ERR_INVALID
    eng.close()


def test_header_binding_and_library_carry_the_new_names(pkg):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    boundary = re.sub(r"/\*.*?\*/", "", open(os.path.join(repo, "include", "ldprune_hip.h")).read(), flags=re.S)
    debug = re.sub(r"/\*.*?\*/", "", open(os.path.join(repo, "include", "ldprune_hip_debug.h")).read(), flags=re.S)
    assert re.search(r"\bldp_get_tile_routes\s*\(", boundary) and re.search(r"\bldp_debug_tile_classes\s*\(", debug)
    assert "ldp_get_tile_routes" in pkg.CABI_SYMBOLS and "ldp_debug_tile_classes" in pkg.CABI_SYMBOLS
    L = ctypes.CDLL(pkg.LIB_PATH)
    assert hasattr(L, "ldp_get_tile_routes") and hasattr(L, "ldp_debug_tile_classes")
    assert ctypes.sizeof(pkg.ldp_tile_routes) == 32
    assert ctypes.sizeof(pkg.ldp_counters) == 200     # (the counters of the boundary did not grow)
    text = open(os.path.join(repo, "include", "ldprune_hip_debug.h")).read()
    assert '"tile_route"' in text


def plan_of(pkg, chr_idx, n=700):
    eng = engine(pkg, n)
    eng.set_variants(np.asarray(chr_idx, dtype=np.uint32), None)
    plan = eng.debug_wide_plan()
    eng.close()
    return plan


def test_the_restatement_on_hand_made_tiles():
    """two J tiles of a 600-row band: (256, 0), (256, 256); one missing call in row 255 (V block 7 of the distance-1 tile) / row 300 / nowhere"""
    full = (1 << 32) - 1
    plan = np.array([[0, 0, 512, full, full], [256, 0, 512, full, full], [256, 256, 512, full, full]], dtype=np.uint32)
    miss = np.zeros(512, dtype=np.int64)
    assert R.expected_classes(plan, miss, 700, R.COMPLETE).tolist() == [0, R.GIVEN, R.TAKEN]
    assert R.expected_classes(plan, miss, 700, R.COMPLETE, corner=False).tolist() == [0, 0, 0]
    miss[255] = 1
    assert R.expected_classes(plan, miss, 700, R.SPARSE).tolist() == [1, 1, 0]          # the diagonal tile is complete, nothing is handed over
    miss[:] = 0
    miss[300] = 40
    assert R.expected_classes(plan, miss, 700, R.GENERAL).tolist() == [0, 1, 1]         # one high row in 512 / 256: 2 % of the rows allow 10 / 5
    miss[300:320] = 40
    assert R.expected_classes(plan, miss, 700, R.GENERAL).tolist() == [0, 2, 2]
    assert R.expected_classes(plan, miss, 700, R.SPARSE).tolist() == [0, 1, 1]          # capped by the group word
    assert R.expected_classes(plan, miss, 700, R.GENERAL, allow_sparse=False).tolist() == [0, 2, 2]
    # live rows: only the blocks of non-zero mask rows / columns, clipped at jend
    t = np.array([256, 0, 300, 1 << (8 * 1 + 7), 0], dtype=np.uint32)    # (J block 1, V block 7)
    assert R.live_rows(t, 10000).tolist() == list(range(224, 256)) + list(range(288, 300))


def test_the_corner_placements_mean_what_the_gpu_test_expects(pkg):
    from test_tile_route import CORNER_EXPECT, CORNER_T, corner_rows
    for place, ((dcls, taken), (ncls, given)) in CORNER_EXPECT.items():
        raw, chr_idx = corner_rows(place)
        miss = R.missing_per_row(raw)
        assert R.group_word(miss, raw.shape[1]) == R.SPARSE
        plan = plan_of(pkg, chr_idx)
        want = R.expected_classes(plan, miss, raw.shape[1], R.SPARSE)
        jv = R.TILE * CORNER_T
        d = [i for i, t in enumerate(plan) if t[0] == jv and t[1] == jv][0]
        n1 = [i for i, t in enumerate(plan) if t[0] == jv and t[1] == jv - R.TILE][0]
        assert (int(want[d]) & 3, bool(want[d] & R.TAKEN)) == (dcls, taken), place
        assert (int(want[n1]) & 3, bool(want[n1] & R.GIVEN)) == (ncls, given), place


def test_the_shared_layouts_hold_all_three_classes(pkg):
    from test_tile_route import three_class_rows
    raw, chr_idx = three_class_rows(700)
    miss = R.missing_per_row(raw)
    assert R.group_word(miss, 700) == R.GENERAL
    c = R.class_counts(R.expected_classes(plan_of(pkg, chr_idx), miss, 700, R.GENERAL))
    assert c["tiles_complete"] > 0 and c["tiles_sparse"] > 0 and c["tiles_general"] > 0 and c["corner_products"] > 0


def test_at_most_four_of_the_random_layouts_lack_a_class(pkg):
    lacking = 0
    for seed in R.RANDOM_SEEDS:
        raw, chr_idx, stretches = R.random_layout(seed)
        miss = R.missing_per_row(raw)
        c = R.class_counts(R.expected_classes(plan_of(pkg, chr_idx), miss, raw.shape[1], R.group_word(miss, raw.shape[1])))
        lacking += 0 if (c["tiles_complete"] and c["tiles_sparse"] and c["tiles_general"]) else 1
    assert len(R.RANDOM_SEEDS) == 20 and lacking <= 4, lacking
