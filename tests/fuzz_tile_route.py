#!/usr/bin/env python3
"""Randomised differential test of per-tile routing on the GPU box: filesets whose missingness differs along the genome
-- stretches of complete rows, rows at 0.1 % and rows at 5 % missing, edges on and off the tile and row-block edges, random sample
counts around the 512-sample stage boundaries, count windows wide enough for the 8 x 8 tile plan, thresholds from 0.1 to 0.8.
Compared per case: the prune set with the CPU oracle's, the decision of EVERY candidate pair with the float64 reference of ldtools,
pred_true with the number of set bits, and the class the device gave every tile with the numpy restatement of the rule
(tile_route_tools.expected_classes).  Prints the first mismatching case (seed) and exits non-zero.
    python tests/fuzz_tile_route.py --stretches [--cases 40] [--seed 1]"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import ldtools as T  # noqa: E402
import tile_route_tools as R  # noqa: E402
import __graft_entry__ as ge  # noqa: E402


def one_case(pkg, rng, idx):
    n = int(rng.choice([300, 511, 512, 513, 700, 1025, 2049, 4000]))
    m = int(rng.integers(900, 2200 if n <= 1025 else 1400))
    second = int(rng.choice([0, 0, 150, 500]))
    window = int(rng.choice([400, 600, 777]))
    r2 = float(rng.choice([0.1, 0.2, 0.5, 0.8]))
    order = int(rng.choice([1, 2]))
    stretches, a = [], 0
    while a < m:
        unit = int(rng.choice([256, 32, 1]))
        b = min(m, max(a + 1, unit * ((a + int(rng.integers(20, 700))) // unit)))
        rate = float(rng.choice([0.0, 0.0, 0.001, 0.05]))
        if rate:
            stretches.append((a, b, rate))
        a = b
    raw, chr_idx = R.stretch_rows(m, n, seed=int(rng.integers(1, 1 << 30)), stretches=stretches, second=second)
    options = {}
    if rng.random() < 0.2:
        options["wide_diag_corner"] = 0
    if rng.random() < 0.15:
        options["pair_sparse"] = 0
    eng = pkg.LdPruneEngine(n, window, 1, False, r2, order=order, device=0)
    for k, v in options.items():
        eng.set_option(k, v)
    eng.set_variants(chr_idx, None)
    lo, cand = eng.band()
    eng.load_genotypes_host(0, T.pack_2bit(raw), pkg.LDP_GENO_REF)
    removed = eng.run()
    pred, outside = eng.last_pred(with_outside=True)
    c = eng.counters()
    plan = eng.debug_wide_plan()
    routes = eng.tile_routes()
    what = "case %d: n=%d m=%d+%d window=%d r2=%g order=%d %s stretches=%s" % (idx, n, m, second, window, r2, order, options, stretches)
    stats = T.band_pair_stats(raw, lo)
    nd, msg = T.compare_decisions(pred, T.band_decisions(stats, r2), lo, stats, r2, counters=c)
    ok = (nd == 0) and (int(pred.sum()) == c["pred_true"]) and (outside == 0)
    inv, mf, _ = T.oracle_prepare(raw)
    want_removed, _ = T.oracle_indep_pairwise(inv, n, chr_idx, np.arange(m + second, dtype=np.uint32), mf, window, 1, False, r2, order)
    ok = ok and np.array_equal(removed, want_removed)
    classes_checked = 0
    if len(plan):
        by_route = [c["route_complete_launches"], c["route_sparse_launches"], c["route_general_launches"]]
        if sum(1 for x in by_route if x) == 1:   # (one word for every launch: the restatement needs the word of each tile's group)
            got = eng.tile_classes()
            want = R.expected_classes(plan, R.missing_per_row(raw), n, int(np.argmax(by_route)), allow_sparse=("pair_sparse" not in options),
                                      corner=("wide_diag_corner" not in options))
            ok = ok and np.array_equal(got, want) and (routes == R.class_counts(want))
            classes_checked = len(got)
            if not np.array_equal(got, want):
                msg += "\nclasses: got %s\n         want %s" % (got.tolist(), want.tolist())
    eng.close()
    if not ok:
        print("MISMATCH " + what + "\n" + msg)
    return ok, cand, classes_checked, routes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stretches", action="store_true", help="(the one mode: missingness in stretches along the genome)")
    ap.add_argument("--cases", type=int, default=40)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    pkg = ge.load_package()
    if pkg.device_count() < 1:
        raise SystemExit("no HIP device")
    rng = np.random.default_rng(args.seed)
    t0 = time.time()
    pairs = tiles = 0
    seen = {"tiles_complete": 0, "tiles_sparse": 0, "tiles_general": 0, "corner_products": 0}
    for idx in range(args.cases):
        ok, cand, checked, routes = one_case(pkg, rng, idx)
        if not ok:
            raise SystemExit(1)
        pairs += cand
        tiles += checked
        for k in seen:
            seen[k] += routes[k]
    print("fuzz_tile_route: %d cases, %d candidate pairs and %d tile classes compared, tiles by class %s, seed %d, %.1f s"
          % (args.cases, pairs, tiles, seen, args.seed, time.time() - t0))


if __name__ == "__main__":
    main()
