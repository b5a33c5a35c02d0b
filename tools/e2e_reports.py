#!/usr/bin/env python3
"""tools/e2e_reports.py -- `--missing --freq --geno-counts` end to end on the chr22-sized fileset of bench.py (176,765 variants x 500,000 samples of
the bench generator with missing calls, the fileset tools/e2e_chr22_missing.py and tools/e2e_filters.py use): plink2-hip writing the reports
from the device's count pass, plink2-hip --debug-host-filter (the host's pass), and -- --reference -- the reference binary, every report file
compared byte for byte with the first leg's; then the prune itself (`--indep-pairwise 500kb 0.2`) with and without the report flags.  Walls are
whole processes, page cache warm, the fastest of --runs.  One JSON record, also written to --record.

  --variants 0 (= the chr22-sized share)   --missing-rate 0.015   --runs 2   --reference   --ref-timeout 1500
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
import __graft_entry__ as ge  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "tools"))
import bench_support as support  # noqa: E402

REPORTS = ["--missing", "--freq", "--geno-counts"]
EXTS = (".afreq", ".gcount", ".smiss", ".vmiss")


def run(binary, cwd, args, out, runs, timeout_s):
    walls, txt, rc = [], "", None
    for _ in range(runs):
        t0 = time.perf_counter()
        cp = subprocess.run([binary] + args + ["--out", out], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout_s)
        wall = time.perf_counter() - t0
        rc = cp.returncode
        if rc != 0:
            txt = cp.stdout
            break
        if not walls or wall < min(walls):
            txt = cp.stdout
        walls.append(wall)
    lines = txt.splitlines()
    return {"rc": rc, "wall_s": min(walls) if walls else None, "wall_s_runs": walls, "reports_line": [ln for ln in lines if "[timing] reports:" in ln],
            "timing_lines": [ln for ln in lines if ln.startswith("[timing]")][:12], "tail": txt[-400:] if rc else ""}


def same_files(cwd, a, b, exts):
    try:
        return all(open(os.path.join(cwd, a + e), "rb").read() == open(os.path.join(cwd, b + e), "rb").read() for e in exts)
    except OSError:
        return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", type=int, default=0)
    ap.add_argument("--missing-rate", type=float, default=0.015)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--reference", action="store_true", help="also run the reference binary (minutes at the full size)")
    ap.add_argument("--ref-timeout", type=int, default=1500)
    ap.add_argument("--record", default=os.path.join(REPO, "profiles", "reports_e2e.json"))
    args = ap.parse_args()
    import torch
    pkg = ge.load_package()
    cfg = dict(bench.CONFIGS["config3"])
    n = cfg["samples"]
    m = args.variants or int(round(cfg["variants"] * bench.CHR22_FRACTION))
    kb = "%gkb" % cfg["window_kb"]
    stride = (n + 3) // 4
    where = support._scratch_dir(m * stride * 1.15 + 2e9)
    if where is None:
        print(json.dumps({"skipped": "no scratch space for the fileset"}))
        return
    have_ref = os.path.exists(support.REF_BIN) and os.access(support.REF_BIN, os.X_OK)
    tmp = tempfile.mkdtemp(prefix="ldbench_reports_", dir=where)
    try:
        chr_idx, bps = bench.genome_layout(m, 1, cfg["spacing"])
        t0 = time.perf_counter()
        file_bytes = support.write_fixed_width_fileset(pkg, torch, tmp, n, m, bench.SEED, chr_idx, bps, missing_rate=args.missing_rate)
        torch.cuda.synchronize()
        res = {"variants": m, "samples": n, "missing_rate": args.missing_rate, "fileset_gb": file_bytes / 1e9, "fileset_written_s": time.perf_counter() - t0, "runs_per_leg": args.runs,
               "what": "whole-process walls (fastest of the runs, page cache warm) on the same fixed-width files, same box, one after the other with the GPU otherwise idle"}
        base = ["--pfile", "g"]
        prune = ["--indep-pairwise", kb, repr(cfg["r2"])]
        alone = {}
        alone["device_records"] = run(support.CLI_BIN, tmp, base + REPORTS + ["--timing"], "ra_dev", args.runs, args.ref_timeout)
        alone["host_pass"] = run(support.CLI_BIN, tmp, base + REPORTS + ["--timing", "--debug-host-filter"], "ra_host", args.runs, args.ref_timeout)
        alone["host_pass"]["files_identical_to_device_records"] = same_files(tmp, "ra_dev", "ra_host", EXTS)
        if args.reference and have_ref:
            # (threads for the reference: what the job was given, where a scheduler sets OMP_NUM_THREADS, else every CPU)
            given = os.environ.get("OMP_NUM_THREADS", "")
            threads = str(int(given) if given.isdigit() and int(given) > 0 else (os.cpu_count() or 1))
            alone["reference"] = run(support.REF_BIN, tmp, base + REPORTS + ["--threads", threads], "ra_ref", 1, args.ref_timeout)
            alone["reference"]["threads"] = int(threads)
            alone["reference"]["files_identical_to_device_records"] = same_files(tmp, "ra_dev", "ra_ref", EXTS)
        res["reports_alone"] = alone
        beside = {}
        beside["prune_only"] = run(support.CLI_BIN, tmp, base + prune + ["--timing"], "p_plain", args.runs, args.ref_timeout)
        beside["prune_with_reports"] = run(support.CLI_BIN, tmp, base + REPORTS + prune + ["--timing"], "p_rep", args.runs, args.ref_timeout)
        beside["prune_with_reports"]["lists_identical_to_prune_only"] = same_files(tmp, "p_plain", "p_rep", (".prune.in", ".prune.out"))
        beside["prune_with_reports"]["files_identical_to_reports_alone"] = same_files(tmp, "ra_dev", "p_rep", EXTS)
        res["beside_the_prune"] = beside
        print(json.dumps(res))
        if args.record:
            with open(args.record, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
    finally:
        subprocess.call(["rm", "-rf", tmp])


if __name__ == "__main__":
    main()
