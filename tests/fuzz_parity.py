#!/usr/bin/env python3
"""Randomised differential test on the GPU box: the HIP path (early termination on, through the C ABI) against the
CPU oracle over random shapes -- sample counts around the 512-sample chunk boundaries, count/kb windows with steps,
both scan orders, thresholds from 0.02 to 0.95, missing rates from 0 to 20 %, LD blocks, monomorphic and all-missing
rows, several chromosomes.  Compared per case: the prune set with the oracle's, and the decision of EVERY candidate pair (the predicate
rows of the production run, LdPruneEngine.last_pred) with the float64 reference of ldtools (band_pair_stats / band_decisions).  Prints
the first mismatching case (seed) and exits non-zero.
    python tests/fuzz_parity.py [--cases 150] [--seed 1] [--mixed | --wide-missing | --wide-sparse | --r2]
--r2: the r^2 outputs of complete-data launches instead (rows, a column block and the hit filter of random all-pairs requests, every value
bit for bit against ldtools.band_r2; the counters must show the complete route)."""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import ldtools as T  # noqa: E402
import __graft_entry__ as ge  # noqa: E402


def one_case(pkg, rng, idx, wide_missing=False, wide_sparse=False, mixed=False):
    n = int(rng.choice([33, 64, 100, 511, 512, 513, 1000, 1536, 2047, 2049, 3000, 5000, 9000]))
    if wide_sparse:
        n = int(rng.choice([1536, 2049, 5000, 9000, 20000, 40000]))   # --wide-sparse: enough 512-sample stages for the checkpoints to fire
    m = int(rng.integers(40, 700 if n <= 3000 else 350))
    miss = float(rng.choice([0.0, 0.0, 0.0, 0.001, 0.003, 0.01, 0.05, 0.2]))
    if wide_sparse:
        miss = float(rng.choice([0.0001, 0.0003, 0.001, 0.002, 0.004, 0.005]))   # ... a FEW missing calls in every row: the tile kernel's SPARSE instantiation
    if wide_missing:
        miss = float(rng.choice([0.01, 0.05, 0.2]))   # --wide-missing: every case on the missing-call kernels ...
    raw = T.synth_raw_codes(m, n, seed=int(rng.integers(1, 1 << 30)), missing_rate=0.0 if mixed else miss)
    if mixed:
        # --mixed: the rows' missing rate is drawn per block of rows from {0, 0.1 %, 5 %} (a generator of its own, so that the sequence of the
        # other modes' cases stays what it was): complete stretches next to incomplete ones, the route following whatever is resident
        mrng = np.random.default_rng(int(rng.integers(1, 1 << 30)))
        a = 0
        while a < m:
            b = min(m, a + int(mrng.integers(8, max(9, m // 2))))
            rate = float(mrng.choice([0.0, 0.001, 0.05]))
            if rate:
                raw[a:b] = np.where(mrng.random((b - a, n)) < rate, 3, raw[a:b])
            a = b
        miss = float((raw == 3).mean())
    # sprinkle structure: copies with noise (LD), monomorphic rows, an all-missing row, rare variants
    for _ in range(m // 6):
        a = int(rng.integers(1, m))
        src = max(0, a - int(rng.integers(1, 12)))
        keep = rng.random(n) < rng.choice([0.5, 0.8, 0.95, 1.0])
        raw[a] = np.where(keep, raw[src], raw[a])
    if m > 20:
        raw[int(rng.integers(0, m))] = int(rng.integers(0, 3))
        raw[int(rng.integers(0, m))] = 3
        v = int(rng.integers(0, m))
        raw[v] = 0
        raw[v, rng.choice(n, size=max(1, n // 200), replace=False)] = 1
    n_chr = int(rng.integers(1, 5))
    chr_idx = np.sort(rng.integers(0, n_chr, size=m)).astype(np.uint32)
    bps = np.zeros(m, dtype=np.uint32)
    for c in range(n_chr):
        sel = np.where(chr_idx == c)[0]
        bps[sel] = np.sort(rng.integers(1, 60000, size=len(sel)))
    is_bp = bool(rng.random() < 0.5)
    if is_bp:
        window, step = int(rng.integers(200, 30000)), 1
    else:
        window = int(rng.integers(2, 260))
        step = int(rng.integers(1, max(2, window)))
    r2 = float(rng.choice([0.02, 0.1, 0.2, 0.35, 0.5, 0.7, 0.9, 0.95]))
    order = int(rng.integers(1, 3))
    inv, mf, _ = T.oracle_prepare(raw)
    want, _ = T.oracle_indep_pairwise(inv, n, chr_idx, bps, mf, window, step, is_bp, r2, order)
    eng = pkg.LdPruneEngine(n, window, step, is_bp, r2, order=order, device=0)
    wide = int(rng.choice([-1, -1, 0, 1, 3]))  # (drawn for every case, so that the sequence of cases stays the same)
    if wide_missing or wide_sparse:
        wide = int(idx % 3)                        # ... over the tile plan (quarter tiles of the four-product form unless switched off below)
    if wide >= 0:
        eng.set_option("wide_min_reach", wide)  # send narrower bands through the 8 x 8 tile plan of the wide-band kernel too
    if idx % 3 == 2:
        eng.set_option("pair_four", 0)   # the six-product form of the missing-call kernel (prune launches default to four)
    if idx % 4 == 3:
        eng.set_option("pair_four_tiles", 0)  # ... on the parallelogram plan in wide bands too (default: quarter tiles of the tile plan)
    if (idx % 5 == 4) and not wide_sparse:
        eng.set_option("pair_sparse", 0)  # rows with a few missing calls through the missing-call kernel too
    if wide_sparse and (idx % 7 == 6):
        eng.set_option("early_exit", 0)   # ... exhaustively now and then
    eng.set_variants(chr_idx, bps)
    packed = T.pack_2bit(raw)
    if rng.random() < 0.5:
        eng.load_genotypes_host(0, packed, pkg.LDP_GENO_REF)
    else:  # several calls, uneven pieces
        cut = sorted(set([0, m] + [int(x) for x in rng.integers(1, m, size=3)]))
        for a, b in zip(cut[:-1], cut[1:]):
            eng.load_genotypes_host(a, packed[a:b], pkg.LDP_GENO_REF)
    got = eng.run()
    ctr = eng.counters()
    pred, outside = eng.last_pred(with_outside=True)
    lo, _ = eng.band()
    eng.close()
    # every candidate pair's decision of this (production) run against the float64 reference
    stats = T.band_pair_stats(raw, lo)
    pairs_wrong, pair_msg = T.compare_decisions(pred, T.band_decisions(stats, r2), lo, stats, r2, counters=ctr, limit=3)
    ok = np.array_equal(got, want) and (pairs_wrong == 0) and (outside == 0) and (int(pred.sum()) == ctr["pred_true"])
    desc = "case %d: n=%d m=%d miss=%g %s window=%d step=%d r2=%g order=%d chr=%d wide_min_reach=%d tiles=%d four_tile_launches=%d sparse_tile_launches=%d recounted=%d removed=%d skipped=%.2f pairs=%d pairs_wrong=%d outside_band=%d" % (
        idx, n, m, miss, "bp" if is_bp else "count", window, step, r2, order, n_chr, wide, ctr["wide_tiles"], ctr["four_tile_launches"], ctr["sparse_tile_launches"],
        ctr["sparse_exact_pairs"], int(want.sum()),
        (ctr["mfma_skipped_product_stages"] / ctr["mfma_product_stages"]) if ctr["mfma_product_stages"] else 0.0, len(pred), pairs_wrong, outside)
    if pairs_wrong:
        desc += "\n" + pair_msg
    return ok, desc


def r2_case(pkg, rng, idx):
    """--r2: complete data, m from 385 (where tiles begin) to 1,500, n from 2 to 3,000, wide_min_reach in {0, 12, 1e9}: a random row chunk
    (doubles or floats), a random column block and the hits of a random chunk at a random threshold, r^2 or signed r"""
    m = int(rng.integers(385, 1501))
    n = int(rng.choice([2, 3, 31, 64, 90, 511, 512, 513, 1024, 1025, int(rng.integers(2, 3001)), int(rng.integers(2, 3001))]))
    raw = T.synth_raw_codes(m, n, seed=int(rng.integers(1, 1 << 30)), missing_rate=0.0, ld_copy_prob=0.6, redraw=0.1)
    for _ in range(m // 6):
        a = int(rng.integers(1, m))
        src = int(rng.integers(0, a))
        row = np.where(rng.random(n) < rng.choice([0.5, 0.8, 0.95, 1.0]), raw[src], raw[a])
        raw[a] = 2 - row if rng.random() < 0.3 else row
    for v in rng.integers(0, m, size=3):
        raw[int(v)] = int(rng.integers(0, 3))
    reach = float(rng.choice([0, 12, 1e9]))
    mode = int(rng.choice([0, 0, 1, 2]))
    lo = np.zeros(m, dtype=np.int64)
    first, second = T.band_pairs(lo)
    band = T.band_r2(T.band_pair_stats(raw, lo, orient=(mode != 2)), signed=1 if mode else 0)
    full = T.band_to_dense(band, lo, 0, m, 0, m, diag=T.self_r2(raw))
    eng = pkg.LdPruneEngine(n, 2, 1, False, 0.5, device=0)
    eng.set_option("wide_min_reach", reach)
    if idx % 4 == 3:
        eng.set_option("orient_rows", 0)
    eng.set_variants_matrix(m)
    eng.load_genotypes_host(0, T.pack_2bit(raw), pkg.LDP_GENO_REF)
    eng.set_r_signed(mode)
    wrong, tiles = [], 0

    def route(what, has_pairs):
        c = eng.counters()
        if has_pairs and (c["route_complete_launches"], c["route_general_launches"]) != (1, 0):   # (a request without a pair may plan nothing)
            wrong.append("%s: not on the complete route %s" % (what, c))
        return c["wide_tiles"]

    r0 = int(rng.integers(0, m))
    rc = int(rng.integers(1, m - r0 + 1))
    as_float = bool(rng.random() < 0.5)
    got = eng.r2_unphased_rows(r0, rc, as_float=as_float)
    tiles += route("rows", r0 + rc > 1)
    want = full[r0:r0 + rc, :r0 + rc]
    want = T.r2_to_float32(want) if as_float else want
    bad = np.argwhere(T.bits_of(got) != T.bits_of(want))
    if len(bad):
        wrong.append("rows(%d, %d, float=%s): %d differ, first (i=%d, j=%d) got %r want %r" % (r0, rc, as_float, len(bad), bad[0][1], r0 + bad[0][0], got[tuple(bad[0])], want[tuple(bad[0])]))
    b0 = int(rng.integers(0, m))
    bc = int(rng.integers(1, m - b0 + 1))
    c0 = int(rng.integers(0, m))
    cc = int(rng.integers(1, m - c0 + 1))
    got = eng.r2_unphased_block(b0, bc, c0, cc, as_float=not as_float)
    tiles += route("block", c0 < b0 + bc - 1)
    want = full[b0:b0 + bc, c0:c0 + cc]
    want = want if as_float else T.r2_to_float32(want)
    bad = np.argwhere(T.bits_of(got) != T.bits_of(want))
    if len(bad):
        wrong.append("block(%d, %d, %d, %d): %d differ, first (i=%d, j=%d) got %r want %r" % (b0, bc, c0, cc, len(bad), c0 + bad[0][1], b0 + bad[0][0], got[tuple(bad[0])], want[tuple(bad[0])]))
    thr = float(rng.choice([0.0, 1e-9, 0.05, 0.2, 0.5]))
    hits, found = eng.r2_unphased_block_hits(thr, b0, bc, c0, cc, capacity=m * m // 2 + 1)
    tiles += route("hits", c0 < b0 + bc - 1)
    with np.errstate(invalid="ignore"):
        sel = (second >= b0) & (second < b0 + bc) & (first >= c0) & (first < c0 + cc) & (np.abs(band) >= thr)
    order = np.lexsort((second[sel], first[sel]))
    f, s, v = first[sel][order], second[sel][order], band[sel][order]
    if not (found == len(f) == len(hits) and np.array_equal(hits["first"].astype(np.int64), f) and np.array_equal(hits["second"].astype(np.int64), s)
            and np.array_equal(T.bits_of(hits["r2"]), T.bits_of(v))):
        wrong.append("block_hits(%g, %d, %d, %d, %d): found %d, returned %d, reference %d (or values differ)" % (thr, b0, bc, c0, cc, found, len(hits), len(f)))
    eng.close()
    desc = "case %d: n=%d m=%d wide_min_reach=%g signed=%d rows=(%d, %d) block=(%d, %d, %d, %d) thr=%g tiles=%d hits=%d" % (idx, n, m, reach, mode, r0, rc, b0, bc, c0, cc, thr, tiles, len(f))
    if wrong:
        desc += "\n" + "\n".join(wrong)
    return not wrong, desc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=150)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--wide-missing", action="store_true", help="every case has missing calls and takes the wide-band tile plan (pair_mfma_tile4_kernel)")
    ap.add_argument("--wide-sparse", action="store_true", help="every case has a FEW missing calls (0.01-0.5 %%) and takes the tile plan: pair_mfma_wide_kernel's SPARSE instantiation")
    ap.add_argument("--mixed", action="store_true", help="the rows' missing rate is drawn per block of rows from {0, 0.1 %%, 5 %%}: mixed-missingness filesets")
    ap.add_argument("--r2", action="store_true", help="the r^2 outputs of complete-data launches (rows, blocks, hits) against ldtools.band_r2")
    args = ap.parse_args()
    pkg = ge.load_package()
    rng = np.random.default_rng(args.seed)
    t0 = time.time()
    if args.r2:
        for k in range(args.cases):
            ok, desc = r2_case(pkg, rng, k)
            if not ok:
                print("MISMATCH", desc, "(--r2 --seed %d)" % args.seed)
                sys.exit(1)
            if k % 25 == 0:
                print(desc, flush=True)
        print("%d r^2 cases bit-identical to the reference, %.1f s" % (args.cases, time.time() - t0))
        return
    skipped_any = sparse_tiles = 0
    for k in range(args.cases):
        ok, desc = one_case(pkg, rng, k, args.wide_missing, args.wide_sparse, args.mixed)
        if "skipped=0.00" not in desc:
            skipped_any += 1
        if "sparse_tile_launches=0" not in desc:
            sparse_tiles += 1
        if not ok:
            print("MISMATCH", desc, "(--seed %d)" % args.seed)
            sys.exit(1)
        if k % 25 == 0:
            print(desc, flush=True)
    print("%d cases identical to the oracle (%d with early termination firing, %d on the tile kernel's SPARSE instantiation), %.1f s" % (args.cases, skipped_any, sparse_tiles,
                                                                                                                                     time.time() - t0))


if __name__ == "__main__":
    main()
