#!/usr/bin/env python3
"""tools/e2e_filters.py -- the command people run, `--maf 0.01 --geno 0.02 --indep-pairwise 500kb 0.2`, end to end on the chr22-sized fileset of
bench.py (176,765 variants x 500,000 samples of the bench generator, here with missing calls), in both file formats: plink2-hip deciding the
count filters from the device's own count pass (load first, ldp_restrict_variants), plink2-hip --debug-host-filter (the host's counting pass in
front of the load), optionally another build of plink2-hip (--other-bin: the parent commit's), and -- --reference -- the reference binary.  Every
run's lists are compared byte for byte with the first one's.  Walls are whole processes, page cache warm, the fastest of --runs.  One JSON
record, also written to --record (default profiles/filter_on_device.json).

  --filters "--maf 0.01 --geno 0.02"   --variants 0 (= the chr22-sized share)   --missing-rate 0.015   --reference   --ref-timeout 1500
"""
import argparse
import json
import os
import re
import shlex
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


def run(binary, cwd, pfile, filters, kb, r2, out, extra=(), runs=2, timeout_s=1500):
    """one binary end to end, `runs` times: the fastest wall, its [timing] lines, the filters' log lines"""
    walls, txt, rc = [], "", None
    for _ in range(runs):
        t0 = time.perf_counter()
        cp = subprocess.run([binary, "--pfile", pfile] + filters + ["--indep-pairwise", kb, repr(r2), "--out", out] + list(extra), cwd=cwd, stdout=subprocess.PIPE,
                            stderr=subprocess.STDOUT, text=True, timeout=timeout_s)
        wall = time.perf_counter() - t0
        rc = cp.returncode
        if rc != 0:
            txt = cp.stdout
            break
        if not walls or wall < min(walls):
            txt = cp.stdout
        walls.append(wall)
    lines = txt.splitlines()
    return {"rc": rc, "wall_s": min(walls) if walls else None, "wall_s_runs": walls,
            "variant_filters_line": [ln for ln in lines if ("variant filters:" in ln) or ("[timing] compaction:" in ln) or ("sample filter (--mind):" in ln) or ("[timing] --het:" in ln)],
            "filter_log_lines": [ln.strip() for ln in lines if "removed due to" in ln],
            "removed_line": [ln.strip() for ln in lines if re.search(r"\d+/\d+ variants removed", ln)][-1:],
            "timing_lines": [ln for ln in lines if ln.startswith("[timing]")][:12], "tail": txt[-400:] if rc else ""}


def host_threads():
    """threads for the reference: what the job was given (OMP_NUM_THREADS where a scheduler sets it), else every CPU"""
    try:
        return max(1, int(os.environ.get("OMP_NUM_THREADS", "0"))) if os.environ.get("OMP_NUM_THREADS") else (os.cpu_count() or 1)
    except ValueError:
        return os.cpu_count() or 1


def same_lists(cwd, a, b):
    try:
        return all(open(os.path.join(cwd, a + e), "rb").read() == open(os.path.join(cwd, b + e), "rb").read() for e in (".prune.in", ".prune.out"))
    except OSError:
        return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filters", default="--maf 0.01 --geno 0.02")
    ap.add_argument("--variants", type=int, default=0)
    ap.add_argument("--missing-rate", type=float, default=0.015)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--reference", action="store_true", help="also run the reference binary (minutes at the full size)")
    ap.add_argument("--ref-timeout", type=int, default=1500)
    ap.add_argument("--no-variable-width", action="store_true")
    ap.add_argument("--other-bin", default="", help="another build of plink2-hip to time on the same files (the parent commit's)")
    ap.add_argument("--record", default=os.path.join(REPO, "profiles", "filter_on_device.json"))
    args = ap.parse_args()
    import torch
    pkg = ge.load_package()
    cfg = dict(bench.CONFIGS["config3"])
    n = cfg["samples"]
    m = args.variants or int(round(cfg["variants"] * bench.CHR22_FRACTION))
    filters = shlex.split(args.filters)
    kb = "%gkb" % cfg["window_kb"]
    stride = (n + 3) // 4
    where = support._scratch_dir(m * stride * (1.15 if args.no_variable_width else 2.1) + 2e9)
    if where is None:
        print(json.dumps({"skipped": "no scratch space for the fileset"}))
        return
    have_ref = os.path.exists(support.REF_BIN) and os.access(support.REF_BIN, os.X_OK)
    tmp = tempfile.mkdtemp(prefix="ldbench_filters_", dir=where)
    try:
        chr_idx, bps = bench.genome_layout(m, 1, cfg["spacing"])
        t0 = time.perf_counter()
        file_bytes = support.write_fixed_width_fileset(pkg, torch, tmp, n, m, bench.SEED, chr_idx, bps, missing_rate=args.missing_rate)
        torch.cuda.synchronize()
        res = {"command": "%s --indep-pairwise %s %g" % (args.filters, kb, cfg["r2"]), "variants": m, "samples": n, "missing_rate": args.missing_rate,
               "fileset_gb": file_bytes / 1e9, "fileset_written_s": time.perf_counter() - t0, "runs_per_leg": args.runs,
               "what": "whole-process walls (fastest of the runs, page cache warm) of the same command on the same files, same box, one after the other with the GPU otherwise idle"}
        formats = [("fixed_width", "g")]
        if (not args.no_variable_width) and have_ref:
            t1 = time.perf_counter()
            mk = subprocess.run([support.REF_BIN, "--pfile", "g", "--make-pgen", "--threads", str(min(host_threads(), 64)), "--out", "v"], cwd=tmp, stdout=subprocess.PIPE,
                                stderr=subprocess.STDOUT, text=True, timeout=args.ref_timeout)
            if mk.returncode == 0:
                formats.append(("variable_width", "v"))
                res["make_pgen_s"] = time.perf_counter() - t1
                res["variable_width_gb"] = os.path.getsize(os.path.join(tmp, "v.pgen")) / 1e9
            else:
                res["variable_width_skipped"] = mk.stdout[-300:]
        for name, pfile in formats:
            leg = {}
            leg["device_records"] = run(support.CLI_BIN, tmp, pfile, filters, kb, cfg["r2"], pfile + "_dev", extra=["--timing"], runs=args.runs)
            leg["host_pass"] = run(support.CLI_BIN, tmp, pfile, filters, kb, cfg["r2"], pfile + "_host", extra=["--timing", "--debug-host-filter"], runs=args.runs)
            leg["host_pass"]["lists_identical_to_device_records"] = same_lists(tmp, pfile + "_dev", pfile + "_host")
            if "--het" in filters:
                try:
                    leg["host_pass"]["het_identical_to_device_records"] = open(os.path.join(tmp, pfile + "_dev.het"), "rb").read() == open(os.path.join(tmp, pfile + "_host.het"), "rb").read()
                except OSError:
                    leg["host_pass"]["het_identical_to_device_records"] = False
            if args.other_bin:
                leg["other_build"] = run(os.path.abspath(args.other_bin), tmp, pfile, filters, kb, cfg["r2"], pfile + "_other", extra=["--timing"], runs=args.runs)
                leg["other_build"]["lists_identical_to_device_records"] = same_lists(tmp, pfile + "_dev", pfile + "_other")
            if args.reference and have_ref:
                t1 = time.perf_counter()
                rp = subprocess.run([support.REF_BIN, "--pfile", pfile] + filters + ["--indep-pairwise", kb, repr(cfg["r2"]), "--threads", str(host_threads()), "--out", pfile + "_ref"],
                                    cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.ref_timeout)
                leg["reference"] = {"rc": rp.returncode, "wall_s": time.perf_counter() - t1, "filter_log_lines": [ln.strip() for ln in rp.stdout.splitlines() if "removed due to" in ln],
                                    "lists_identical_to_device_records": rp.returncode == 0 and same_lists(tmp, pfile + "_dev", pfile + "_ref")}
            d, h = leg["device_records"]["wall_s"], leg["host_pass"]["wall_s"]
            if d and h:
                leg["host_pass_over_device_records"] = h / d
            res[name] = leg
        print(json.dumps(res))
        if args.record:
            with open(args.record, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
    finally:
        subprocess.call(["rm", "-rf", tmp])


if __name__ == "__main__":
    main()
