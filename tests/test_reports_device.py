"""plink2-hip --missing / --freq / --geno-counts from the load's own counts: the records of the device's count pass, the per-sample read of the
resident image and, for variants with several ALT alleles, the allele counts the decode kernel kept -- against the reference binary file for file
as bytes and against the host's pass.  With --indep-pairwise in the same run (the prune lists must not move), alone, after a --mind that starts
the run over, and with two engines, which take the host's pass."""
import filecmp
import os

import numpy as np
import pytest

import ldtools as T
import reports_tools as RT
from test_cli import cli, run_cli  # noqa: F401  (fixture)
from test_pgen_reader import make_multiallelic_vcf

pytestmark = pytest.mark.gpu

DEVICE_LINE = "reports: from the device's count pass"
HOST_LINE = "reports: host pass"


@pytest.fixture(scope="module")
def fileset(tmp_path_factory):
    assert T.have_ref()
    d = tmp_path_factory.mktemp("reports_device")
    raw = RT.codes()
    RT.check_fixture(raw)
    RT.write_fileset(d, raw)
    return d, raw


def log_lines(d, sub, tag):
    return RT.report_lines(str(d / sub / (tag + ".log")))


@pytest.mark.parametrize("fmt", list(RT.FORMATS))
def test_reports_beside_the_prune(gpu_pkg, cli, fileset, fmt):
    d, _ = fileset
    tag = RT.TAG[fmt]
    args = RT.FORMATS[fmt] + RT.REPORTS + ["--geno", "0.05", "--maf", "0.1"] + RT.PRUNE
    ref = T.run_ref(args + ["--threads", "4", "--out", tag], str(d / "ref"))
    dev = run_cli(cli, args + ["--timing", "--out", tag], str(d / "dev"))
    plain = run_cli(cli, RT.FORMATS[fmt] + ["--geno", "0.05", "--maf", "0.1"] + RT.PRUNE + ["--out", tag + "_plain"], str(d / "dev"))
    assert ref.returncode == 0 and dev.returncode == 0 and plain.returncode == 0, (ref.stdout[-600:], dev.stdout[-1500:], plain.stdout[-800:])
    assert DEVICE_LINE in dev.stdout and HOST_LINE not in dev.stdout, dev.stdout[-1500:]
    RT.same_bytes(d, "dev", tag, RT.EXTS + (".prune.in", ".prune.out"))
    want = log_lines(d, "ref", tag)
    assert len(want) == 6 and want[4].startswith("--geno: ") and not want[4].startswith("--geno: 0 "), want
    assert log_lines(d, "dev", tag) == want
    # the prune's lists are what they are without the report flags
    for ext in (".prune.in", ".prune.out"):
        assert filecmp.cmp(str(d / "dev" / (tag + ext)), str(d / "dev" / (tag + "_plain" + ext)), shallow=False), ext
    assert os.path.getsize(str(d / "dev" / (tag + ".prune.in"))) > 20


@pytest.mark.parametrize("fmt", list(RT.FORMATS))
def test_reports_alone(gpu_pkg, cli, fileset, fmt):
    d, _ = fileset
    tag = RT.TAG[fmt] + "a"
    args = RT.FORMATS[fmt] + ["--freq", "counts", "--geno-counts", "--missing"]
    ref = T.run_ref(args + ["--threads", "4", "--out", tag], str(d / "ref"))
    dev = run_cli(cli, args + ["--timing", "--out", tag], str(d / "dev"))
    assert ref.returncode == 0 and dev.returncode == 0, (ref.stdout[-600:], dev.stdout[-1500:])
    assert DEVICE_LINE in dev.stdout and HOST_LINE not in dev.stdout, dev.stdout[-1500:]
    assert " GPU): " not in dev.stdout and "Variant lists written" not in dev.stdout, dev.stdout     # no plan, no pair kernel
    RT.same_bytes(d, "dev", tag, (".acount", ".gcount", ".smiss", ".vmiss"))
    assert log_lines(d, "dev", tag) == log_lines(d, "ref", tag) and len(log_lines(d, "ref", tag)) == 4
    assert not os.path.exists(str(d / "dev" / (tag + ".prune.in")))


@pytest.mark.parametrize("fmt", ["bed", "pgen-varwidth"])
def test_mind_restarts_and_the_reports_come_from_the_second_load(gpu_pkg, cli, fileset, fmt):
    d, _ = fileset
    tag = RT.TAG[fmt] + "m"
    args = RT.FORMATS[fmt] + ["--mind", "0.1"] + RT.REPORTS + RT.PRUNE
    ref = T.run_ref(args + ["--threads", "4", "--out", tag], str(d / "ref"))
    dev = run_cli(cli, args + ["--timing", "--out", tag], str(d / "dev"))
    assert ref.returncode == 0 and dev.returncode == 0, (ref.stdout[-600:], dev.stdout[-1500:])
    assert "2 samples removed, reloading)" in dev.stdout and DEVICE_LINE in dev.stdout and HOST_LINE not in dev.stdout, dev.stdout[-1500:]
    assert dev.stdout.count(DEVICE_LINE) == 1 and dev.stdout.count("--freq: Allele") == 1
    RT.same_bytes(d, "dev", tag, RT.EXTS + (".mindrem.id", ".prune.in", ".prune.out"))
    assert log_lines(d, "dev", tag) == log_lines(d, "ref", tag) and len(log_lines(d, "ref", tag)) == 5
    smiss = open(str(d / "dev" / (tag + ".smiss"))).read().split("\n")
    assert len(smiss) == RT.N - len(RT.S_30PCT) + 2


def test_two_engines_take_the_host_pass(gpu_pkg, cli, fileset):
    d, _ = fileset
    args = RT.FORMATS["pgen-fixed"] + RT.REPORTS + RT.PRUNE
    ref = T.run_ref(args + ["--threads", "4", "--out", "g2"], str(d / "ref"))
    dev = run_cli(cli, args + ["--gpus", "2", "--debug-alias-devices", "--timing", "--out", "g2"], str(d / "dev"))
    assert ref.returncode == 0 and dev.returncode == 0, (ref.stdout[-600:], dev.stdout[-1500:])
    assert HOST_LINE in dev.stdout and "more than one GPU" in dev.stdout and DEVICE_LINE not in dev.stdout, dev.stdout[-1500:]
    RT.same_bytes(d, "dev", "g2", RT.EXTS + (".prune.in", ".prune.out"))
    assert log_lines(d, "dev", "g2") == log_lines(d, "ref", "g2")


@pytest.mark.parametrize("decode", ["device", "host"])
def test_multiallelic_variants_from_the_kernels_allele_counts(gpu_pkg, cli, tmp_path, decode):
    """a VCF-imported file with 1-5 ALT alleles: .afreq / .acount from the allele counts the decode kernel kept (the [timing] line says how many rows
    had them), or -- --debug-host-decode: the host builds those rows -- from the reader's allele pairs; the same bytes either way"""
    m, n = 400, 90
    alt_ct, lo, hi = make_multiallelic_vcf(str(tmp_path / "d.vcf"), m, n, seed=31, max_alt=5, missing=0.03)
    T.ref_import_vcf(str(tmp_path / "d.vcf"), str(tmp_path / "d"))
    for sub in ("ref", "dev"):
        os.makedirs(str(tmp_path / sub))
    n_multi = int((alt_ct > 1).sum())
    extra = ["--debug-host-decode"] if decode == "host" else []
    for tag, freq in (("f", ["--freq"]), ("c", ["--freq", "counts"])):
        args = ["--pfile", "../d"] + freq + ["--missing", "--indep-pairwise", "50", "5", "0.3"]
        ref = T.run_ref(args + ["--threads", "4", "--out", tag], str(tmp_path / "ref"))
        dev = run_cli(cli, args + extra + ["--timing", "--out", tag], str(tmp_path / "dev"))
        plain = run_cli(cli, ["--pfile", "../d", "--indep-pairwise", "50", "5", "0.3"] + extra + ["--out", tag + "p"], str(tmp_path / "dev"))
        assert ref.returncode == 0 and dev.returncode == 0 and plain.returncode == 0, (ref.stdout[-600:], dev.stdout[-1500:], plain.stdout[-600:])
        assert DEVICE_LINE in dev.stdout, dev.stdout[-1500:]
        want = ("allele counts of %d multiallelic rows from the device, 0 from the reader" % n_multi) if decode == "device" else \
               ("allele counts of 0 multiallelic rows from the device, %d from the reader" % n_multi)
        assert want in dev.stdout, dev.stdout[-1500:]
        RT.same_bytes(tmp_path, "dev", tag, ((".afreq",) if tag == "f" else (".acount",)) + (".smiss", ".vmiss", ".prune.in", ".prune.out"))
        for ext in (".prune.in", ".prune.out"):
            assert filecmp.cmp(str(tmp_path / "dev" / (tag + ext)), str(tmp_path / "dev" / (tag + "p" + ext)), shallow=False), ext
