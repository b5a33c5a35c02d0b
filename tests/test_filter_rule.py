"""Where plink2-hip decides --geno / --maf / --mac from: the records of the device's count pass (load first, then ldp_restrict_variants)
when the job allows it, its own host pass over the rows otherwise.  The decision is host logic: --dry-run prints it (and plans on the
list the host pass leaves), no device needed."""
import os
import shutil

import numpy as np
import pytest

from test_cli import cli, run_cli, small_fileset  # noqa: F401  (fixture)

PRUNE = ["--indep-pairwise", "50", "5", "0.2", "--bad-ld"]
DEVICE = "dry-run: variant filters: from the device's count pass"
HOST = "dry-run: variant filters: host pass: "


def filter_line(cp):
    lines = [ln for ln in cp.stdout.splitlines() if ln.startswith("dry-run: variant filters:")]
    assert len(lines) == 1, cp.stdout[-1200:]
    return lines[0]


@pytest.mark.parametrize("fmt", ["--bfile", "--pfile"])
@pytest.mark.parametrize("filters", [["--maf", "0.05"], ["--geno", "0.05"], ["--mac", "5", "--max-mac", "100"], ["--geno", "0.04", "--max-maf", "0.45"]])
def test_eligible_jobs_take_the_device_records(cli, tmp_path, fmt, filters):
    small_fileset(tmp_path)
    cp = run_cli(cli, [fmt, "d"] + filters + PRUNE + ["--dry-run", "--out", "o"], str(tmp_path))
    assert cp.returncode == 0 and filter_line(cp) == DEVICE, cp.stdout[-800:]
    # the plan --dry-run reports is over the variants the filters leave, whoever would apply them
    host = run_cli(cli, [fmt, "d"] + filters + PRUNE + ["--debug-host-filter", "--dry-run", "--out", "o"], str(tmp_path))
    assert host.returncode == 0 and filter_line(host) == HOST + "--debug-host-filter"
    plan = [ln for ln in cp.stdout.splitlines() if ln.startswith("dry-run: founders=")]
    assert plan and plan == [ln for ln in host.stdout.splitlines() if ln.startswith("dry-run: founders=")]
    assert "variants=120 " not in plan[0]


def test_no_count_filter_no_line(cli, tmp_path):
    small_fileset(tmp_path)
    cp = run_cli(cli, ["--bfile", "d", "--chr", "1-2"] + PRUNE + ["--dry-run", "--out", "o"], str(tmp_path))
    assert cp.returncode == 0 and "variant filters" not in cp.stdout


@pytest.mark.parametrize("extra,fileset_args,reason", [
    (["--gpus", "2"], {}, "more than one GPU"),
    (["--debug-host-filter"], {}, "--debug-host-filter"),
    ([], {"nonfounders": 5}, "non-founders among the kept samples"),
])
def test_ineligible_prune_jobs_keep_the_host_pass(cli, tmp_path, extra, fileset_args, reason):
    small_fileset(tmp_path, **fileset_args)
    for fmt in ("--bfile", "--pfile"):
        cp = run_cli(cli, [fmt, "d", "--maf", "0.05", "--geno", "0.05"] + extra + PRUNE + ["--dry-run", "--out", "o"], str(tmp_path))
        assert cp.returncode == 0, cp.stdout[-800:]
        line = filter_line(cp)
        assert line.startswith(HOST) and reason in line, line
        assert "--geno: " in cp.stdout and "removed due to allele frequency" in cp.stdout   # ... and the pass ran


def test_chromosome_zero_variants_do_not_matter(cli, tmp_path):
    small_fileset(tmp_path, chr0=3)
    cp = run_cli(cli, ["--bfile", "d", "--maf", "0.05"] + PRUNE + ["--dry-run", "--out", "o"], str(tmp_path))
    assert cp.returncode == 0 and filter_line(cp) == DEVICE


def test_pairphase_and_the_r2_outputs_keep_the_host_pass(cli, tmp_path):
    small_fileset(tmp_path)
    cp = run_cli(cli, ["--bfile", "d", "--maf", "0.05", "--indep-pairphase", "50", "5", "0.2", "--bad-ld", "--dry-run", "--out", "o"], str(tmp_path))
    assert "--indep-pairphase plans its engines before the load" in filter_line(cp)
    # (the r^2 outputs have no --dry-run of their own: the line is printed before the command looks for a device)
    cp = run_cli(cli, ["--bfile", "d", "--maf", "0.05", "--r2-unphased", "--ld-window-kb", "1", "--dry-run", "--out", "o"], str(tmp_path))
    assert "the r^2 outputs and --clump plan their engines before the load" in filter_line(cp)


def test_a_file_with_dosage_tracks_keeps_the_host_pass(cli, tmp_path):
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pgen")
    g = np.load(os.path.join(gold, "dosage_small.npz"))
    n, m = int(g["n"]), int(g["m"])
    shutil.copy(os.path.join(gold, "dosage_small.pgen"), str(tmp_path / "q.pgen"))
    with open(str(tmp_path / "q.pvar"), "w") as f:
        f.write("#CHROM\tPOS\tID\tREF\tALT\n" + "".join("1\t%d\tsnp%d\tA\tC\n" % (1000 + 100 * v, v) for v in range(m)))
    with open(str(tmp_path / "q.psam"), "w") as f:
        f.write("#IID\tSEX\n" + "".join("s%d\t2\n" % s for s in range(n)))
    cp = run_cli(cli, ["--pfile", "q", "--maf", "0.05"] + PRUNE + ["--dry-run", "--out", "o"], str(tmp_path))
    assert cp.returncode == 0, cp.stdout[-800:]
    assert "the file has dosage tracks" in filter_line(cp)
