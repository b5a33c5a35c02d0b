"""Measures the exact Hardy-Weinberg test for profiles/hwe.md: hwe_kernel through ldp_hwe_ln_pvals_counts (HIP events, median of 10 after 2
warm-ups) and the same triples through ldp_hwe_ln_p_host on 1 and on 16 threads (ctypes releases the GIL; blocks of triples per thread).
  python tools/bench_hwe.py [--variants 1250000] [--samples 500000] [--host-variants 100000]
Triples: Hardy-Weinberg draws over MAF 0.01-0.5, a tenth of them with 10 % of the het calls moved to or taken from the homozygotes; a second
set has 1 % all-het rows on top, the walk's worst case.  One JSON line per measurement."""
import argparse
import ctypes
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402


def triples(m, n, seed, all_het_share=0.0):
    rng = np.random.default_rng(seed)
    q = rng.uniform(0.01, 0.5, size=m)
    het = rng.binomial(n, 2 * q * (1 - q)).astype(np.int64)
    hom2 = rng.binomial(n - het, (q * q) / np.maximum(1 - 2 * q * (1 - q), 1e-300)).astype(np.int64)
    hom1 = n - het - hom2
    # a tenth of the rows: 10 % of the het calls become homozygous, two at a time into one homozygote of each kind (deficit), or as many
    # come out of the homozygotes the same way (excess): the allele counts stay
    kind = rng.random(m)
    t = het // 20
    deficit, excess = kind < 0.05, (kind >= 0.05) & (kind < 0.10)
    t = np.where(deficit, t, np.where(excess, -np.minimum(t, np.minimum(hom1, hom2)), 0))
    het, hom1, hom2 = het - 2 * t, hom1 + t, hom2 + t
    if all_het_share:
        rows = rng.random(m) < all_het_share
        hom1, het, hom2 = np.where(rows, 0, hom1), np.where(rows, n, het), np.where(rows, 0, hom2)
    assert (hom1 >= 0).all() and (het >= 0).all() and (hom2 >= 0).all() and ((hom1 + het + hom2) == n).all()
    return hom1.astype(np.uint32), het.astype(np.uint32), hom2.astype(np.uint32)


def host_seconds(pkg, cts, threads):
    L = pkg.lib()
    a, b, c = (x.tolist() for x in cts)
    m = len(a)

    def block(lo, hi):
        f = ctypes.c_uint8()
        fn = L.ldp_hwe_ln_p_host
        for v in range(lo, hi):
            fn(a[v], b[v], c[v], 0, ctypes.byref(f))

    step = max(1, m // (threads * 8))
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=threads) as pool:
        list(pool.map(lambda lo: block(lo, min(m, lo + step)), range(0, m, step)))
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", type=int, default=1250000)
    ap.add_argument("--samples", type=int, default=500000)
    ap.add_argument("--host-variants", type=int, default=100000, help="triples of the set the host runs go over (their time is scaled up)")
    ap.add_argument("--no-gpu", action="store_true")
    args = ap.parse_args()
    pkg = ge.load_package()
    for name, share in (("hwe_draws", 0.0), ("one_percent_all_het", 0.01)):
        cts = triples(args.variants, args.samples, 7, share)
        if not args.no_gpu:
            ms = []
            for it in range(12):
                st = {}
                pkg.hwe_ln_pvals_counts(*cts, stats=st)
                if it >= 2:
                    ms.append(st["ms_kernel"])
            print(json.dumps({"set": name, "variants": args.variants, "samples": args.samples, "kernel_ms_median": float(np.median(ms)), "kernel_ms_min": min(ms),
                              "kernel_ms_max": max(ms)}), flush=True)
        sub = tuple(x[:args.host_variants] for x in cts)
        for threads in (1, 16):
            s = host_seconds(pkg, sub, threads)
            print(json.dumps({"set": name, "host_threads": threads, "host_variants": len(sub[0]), "seconds": s,
                              "seconds_scaled_to_all": s * args.variants / len(sub[0]), "us_per_variant": 1e6 * s / len(sub[0])}), flush=True)


if __name__ == "__main__":
    main()
