#!/usr/bin/env python3
"""Measure --make-king-table: plink2-hip's device path beside the reference binary on the same files, and the king kernels on their own.

    python tools/bench_king.py [--samples 10000] [--variants 50000] [--missing 0.01] [--filter 0.0884] [--dir DIR] [--limit SECONDS]

Writes a fixed-width fileset of unrelated samples (plus a few planted duplicates and half-copies, so that the filter reports something),
then
  1. plink2-hip --make-king-table --king-table-filter <x> --timing, end to end (wall of the process),
  2. oracle/_ref/plink2 with the same flags and its default threads (wall), where the binary is there; the two .kin0 files must be identical,
  3. the kernels: the same rows in an engine, one 4,096 x 4,096 block below the diagonal through ldp_debug_king_counts_block -- warm-up first,
     then the median of five HIP-event times -- as pair-variants per second and as a fraction of the FP4 peak (five products per pair-variant,
     two flops per product term, 10 PF dense).
One GPU process at a time, every step under the tool's own time limit; prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
FP4_PEAK_FLOPS = 10.0e15
PRODUCTS = 5


def write_fileset(prefix, n, m, missing, seed=1):
    """fixed-width .pgen + .pvar + .psam, written in chunks of variants; returns nothing"""
    rng = np.random.default_rng(seed)
    rec = (n + 3) // 4
    dup = [(1, 0), (3, 2)]            # identical samples
    half = [(5, 4), (7, 6), (9, 8)]   # every other variant copied: related pairs
    with open(prefix + ".pgen", "wb") as f:
        f.write(bytes([0x6C, 0x1B, 0x02]))
        f.write(np.uint32(m).tobytes())
        f.write(np.uint32(n).tobytes())
        f.write(bytes([0x40]))
        for v0 in range(0, m, 2000):
            k = min(2000, m - v0)
            maf = rng.uniform(0.05, 0.5, size=(k, 1))
            raw = (rng.random((k, n)) < maf).astype(np.uint8) + (rng.random((k, n)) < maf).astype(np.uint8)
            for a, b in dup:
                raw[:, a] = raw[:, b]
            for a, b in half:
                raw[::2, a] = raw[::2, b]
            if missing:
                raw[rng.random((k, n)) < missing] = 3
            padded = np.zeros((k, rec * 4), dtype=np.uint8)
            padded[:, :n] = raw
            q = padded.reshape(k, rec, 4)
            f.write((q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)).astype(np.uint8).tobytes())
    with open(prefix + ".pvar", "w") as f:
        f.write("#CHROM\tPOS\tID\tREF\tALT\n")
        per = (m + 21) // 22
        for i in range(m):
            f.write("%d\t%d\tsnp%d\tA\tC\n" % (1 + i // per, 1000 + 100 * (i % per), i))
    with open(prefix + ".psam", "w") as f:
        f.write("#IID\tSEX\n")
        for s in range(n):
            f.write("s%d\t2\n" % s)


def timed(cmd, cwd, limit):
    t0 = time.time()
    cp = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=limit)
    return time.time() - t0, cp


def kernel_times(prefix, n, m, limit_s):
    import __graft_entry__ as ge
    pkg = ge.load_package()
    if pkg.device_count() < 1:
        raise RuntimeError("no HIP device visible")
    rec = (n + 3) // 4
    eng = pkg.LdPruneEngine(n, 50, 5, False, 0.2, order=2, device=0)
    eng.set_variants_matrix(m)
    fd = os.open(prefix + ".pgen", os.O_RDONLY)
    try:
        eng.load_genotypes_fd(0, m, fd, 12, rec, pkg.LDP_GENO_REF)
    finally:
        os.close(fd)
    side = min(4096, n // 2)
    block = (n - side, side, 0, side)   # rows = the last `side` samples, columns = the first: every pair of the block counts
    ms = []
    t0 = time.time()
    pv = 0
    for it in range(6):
        st = {}
        eng.king_counts_block(*block, stats=st)
        pv = st["pair_variants"]
        if it:
            ms.append(st["ms_kernel"])
        if time.time() - t0 > limit_s:
            break
    eng.close()
    med = float(np.median(ms)) if ms else float("nan")
    rate = pv / (med * 1e-3) if ms else float("nan")
    return {"block": list(block), "ms_kernel_runs": ms, "ms_kernel_median": med, "pair_variants": pv, "pair_variants_per_s": rate,
            "fp4_peak_fraction": rate * PRODUCTS * 2 / FP4_PEAK_FLOPS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--variants", type=int, default=50000)
    ap.add_argument("--missing", type=float, default=0.01)
    ap.add_argument("--filter", default="0.0884")
    ap.add_argument("--dir", default=None)
    ap.add_argument("--limit", type=float, default=420.0, help="time limit of each step, seconds")
    ap.add_argument("--no-reference", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.load_package()
    d = a.dir or tempfile.mkdtemp(prefix="bench_king_")
    os.makedirs(d, exist_ok=True)
    prefix = os.path.join(d, "k")
    t0 = time.time()
    write_fileset(prefix, a.samples, a.variants, a.missing)
    out = {"samples": a.samples, "variants": a.variants, "missing": a.missing, "filter": a.filter, "write_fileset_s": time.time() - t0}
    print("fileset written: %.1f s" % out["write_fileset_s"], file=sys.stderr, flush=True)
    flags = ["--pfile", "k", "--make-king-table", "--king-table-filter", a.filter]
    wall, cp = timed([pkg.CLI_PATH] + flags + ["--timing", "--out", "hip"], d, a.limit)
    if cp.returncode != 0:
        print(cp.stdout[-2000:])
        raise SystemExit("plink2-hip failed (%d)" % cp.returncode)
    timing = [l for l in cp.stdout.split("\n") if l.startswith("[timing] --make-king-table") or l.startswith("--king-table-filter")]
    out.update(hip_wall_s=wall, hip_timing=timing, hip_path="device" if any("from the resident image" in l for l in timing) else "host")
    print("plink2-hip: %.2f s" % wall, file=sys.stderr, flush=True)
    ref_bin = os.path.join(REPO, "oracle", "_ref", "plink2")
    if os.path.exists(ref_bin) and not a.no_reference:
        wall, cp = timed([ref_bin] + flags + ["--out", "ref"], d, a.limit)
        if cp.returncode != 0:
            print(cp.stdout[-2000:])
            raise SystemExit("the reference failed (%d)" % cp.returncode)
        same = open(os.path.join(d, "ref.kin0"), "rb").read() == open(os.path.join(d, "hip.kin0"), "rb").read()
        threads = [l for l in cp.stdout.split("\n") if l.startswith("Using ")]
        out.update(ref_wall_s=wall, ref_threads=threads[0] if threads else "", identical_files=same)
        print("reference: %.2f s, identical files: %s" % (wall, same), file=sys.stderr, flush=True)
        if not same:
            print(json.dumps(out))
            raise SystemExit("the two .kin0 files differ")
    out["kernels"] = kernel_times(prefix, a.samples, a.variants, a.limit)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
