"""plink2-hip --geno / --maf / --max-maf / --mac / --max-mac in front of --indep-pairwise, decided from the records of the device's own count
pass (the variants are loaded first, ldp_restrict_variants() then drops what the filters remove and plans): the lists and the filters' log
lines against the reference binary's and against plink2-hip's host pass (--debug-host-filter), for the three file formats; and the jobs that
must keep the host pass."""
import filecmp
import os

import pytest

import ldtools as T
from test_cli import cli, run_cli  # noqa: F401  (fixture)
from test_filters import fileset

pytestmark = pytest.mark.gpu

PRUNE = ["--indep-pairwise", "60kb", "0.3"]
FORMATS = {"bed": ["--bfile", "d"], "pgen-fixed": ["--pfile", "d"], "pgen-varwidth": ["--pfile", "v"]}
FILTERS = {
    "geno": ["--geno", "0.02"],
    "maf": ["--maf", "0.05", "--max-maf", "0.4"],
    "mac": ["--mac", "20", "--max-mac", "200"],
    "all": ["--geno", "0.02", "--maf", "0.05", "--max-maf", "0.4", "--mac", "20", "--max-mac", "200"],
    "everything-goes": ["--mac", "100000"],      # more copies of the rarer allele than 150 samples hold
    "nothing-goes": ["--geno", "0.9", "--maf", "0.0001"],
}
DEVICE_LINE = "variant filters: from the device's count pass"
HOST_LINE = "variant filters: host pass"


def write_variable_width(cwd):
    mk = T.run_ref(["--pfile", "d", "--make-pgen", "--out", "v"], cwd)
    assert mk.returncode == 0, mk.stdout[-800:]


@pytest.fixture(scope="module")
def founders_dir(tmp_path_factory):
    """test_filters.fileset(with_x=False) -- 1,200 variants x 150 samples, chromosomes 0, 1, 2, 3, 7, 9 -- with every sample a founder, as
    .bed, fixed-width .pgen and the reference's variable-width .pgen"""
    assert T.have_ref()
    d = tmp_path_factory.mktemp("filter_on_device")
    fileset(d, with_x=False)
    n = 150
    fam = open(str(d / "d.fam")).read().splitlines()
    open(str(d / "d.fam"), "w").write("\n".join(" ".join(f.split()[:2] + ["0", "0"] + f.split()[4:]) for f in fam) + "\n")
    psam = open(str(d / "d.psam")).read().splitlines()
    open(str(d / "d.psam"), "w").write("\n".join([psam[0]] + ["\t".join([l.split("\t")[0], "0", "0", l.split("\t")[3]]) for l in psam[1:]]) + "\n")
    assert len(fam) == n
    write_variable_width(str(d))
    return d


def filter_lines(stdout):
    return [l.strip() for l in stdout.split("\n") if "removed due to" in l]


def three_runs(cli, cwd, args, tag):
    ref = T.run_ref(args + ["--threads", "4", "--out", tag + "_ref"], cwd)
    dev = run_cli(cli, args + ["--timing", "--out", tag + "_dev"], cwd)
    host = run_cli(cli, args + ["--timing", "--debug-host-filter", "--out", tag + "_host"], cwd)
    return ref, dev, host


@pytest.mark.parametrize("filters", list(FILTERS))
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_lists_and_log_lines_match_the_reference_and_the_host_pass(gpu_pkg, cli, founders_dir, fmt, filters):
    cwd = str(founders_dir)
    tag = "%s_%s" % (fmt, filters)
    args = FORMATS[fmt] + FILTERS[filters] + PRUNE
    ref, dev, host = three_runs(cli, cwd, args, tag)
    assert DEVICE_LINE in dev.stdout and HOST_LINE not in dev.stdout, dev.stdout[-1500:]
    assert HOST_LINE in host.stdout and DEVICE_LINE not in host.stdout, host.stdout[-1500:]
    want = filter_lines(ref.stdout)
    assert want and filter_lines(dev.stdout) == want and filter_lines(host.stdout) == want, (want, filter_lines(dev.stdout), filter_lines(host.stdout))
    if filters == "everything-goes":
        assert ref.returncode == dev.returncode == host.returncode == 13, (ref.returncode, dev.returncode, host.returncode, dev.stdout[-600:])
        assert "No variants remaining after main filters" in dev.stdout and "No variants remaining after main filters" in host.stdout
        return
    assert ref.returncode == 0 and dev.returncode == 0 and host.returncode == 0, (ref.stdout[-600:], dev.stdout[-1200:], host.stdout[-600:])
    for ext in (".prune.in", ".prune.out"):
        a = os.path.join(cwd, tag + "_ref" + ext)
        assert filecmp.cmp(a, os.path.join(cwd, tag + "_dev" + ext), shallow=False), (ext, "device records")
        assert filecmp.cmp(a, os.path.join(cwd, tag + "_host" + ext), shallow=False), (ext, "host pass")
    ignoring = [l.strip() for l in ref.stdout.split("\n") if "chromosome 0 variant" in l]
    assert [l.strip() for l in dev.stdout.split("\n") if "chromosome 0 variant" in l] == ignoring
    n_listed = sum(len(open(os.path.join(cwd, tag + "_ref" + e)).read().split()) for e in (".prune.in", ".prune.out"))
    if filters == "nothing-goes":
        assert n_listed == 1195 and all(l.startswith("0 variants") or l.startswith("--geno: 0 variants") for l in want), want
    else:
        assert 50 < n_listed < 1195   # the filters removed something and left something


def test_jobs_that_keep_the_host_pass(gpu_pkg, cli, tmp_path):
    """non-founders among the samples (--geno counts them; the image holds founders), and more than one engine"""
    assert T.have_ref()
    fileset(tmp_path, with_x=False)          # (every 13th sample has its parents in the file)
    cwd = str(tmp_path)
    args = ["--bfile", "d", "--geno", "0.02", "--maf", "0.05"] + PRUNE
    ref = T.run_ref(args + ["--threads", "4", "--out", "ref"], cwd)
    got = run_cli(cli, args + ["--timing", "--out", "hip"], cwd)
    assert ref.returncode == 0 and got.returncode == 0, (ref.stdout[-600:], got.stdout[-1200:])
    assert HOST_LINE in got.stdout and "non-founders" in got.stdout and DEVICE_LINE not in got.stdout
    assert filter_lines(got.stdout) == filter_lines(ref.stdout)
    for ext in (".prune.in", ".prune.out"):
        assert filecmp.cmp(os.path.join(cwd, "ref" + ext), os.path.join(cwd, "hip" + ext), shallow=False), ext


def test_two_engines_keep_the_host_pass(gpu_pkg, cli, founders_dir):
    cwd = str(founders_dir)
    args = ["--pfile", "d", "--geno", "0.02", "--maf", "0.05"] + PRUNE
    ref = T.run_ref(args + ["--threads", "4", "--out", "two_ref"], cwd)
    got = run_cli(cli, args + ["--gpus", "2", "--debug-alias-devices", "--timing", "--out", "two_hip"], cwd)
    assert ref.returncode == 0 and got.returncode == 0, (ref.stdout[-600:], got.stdout[-1200:])
    assert HOST_LINE in got.stdout and "more than one GPU" in got.stdout and DEVICE_LINE not in got.stdout
    assert filter_lines(got.stdout) == filter_lines(ref.stdout)
    for ext in (".prune.in", ".prune.out"):
        assert filecmp.cmp(os.path.join(cwd, "two_ref" + ext), os.path.join(cwd, "two_hip" + ext), shallow=False), ext
