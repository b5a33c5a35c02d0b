"""plink2-hip --het on the GPU: three runs per case, as in test_mind.py -- the reference, plink2-hip reading the resident image
(ldp_sample_het_counts; the [timing] line says so) and plink2-hip --debug-host-filter (the host's pass over the rows) -- with <out>.het the
same bytes everywhere and the same --het log lines.  The filesets follow het_tools' fixture rule: the reference's --threads 1 and --threads 4
outputs are compared first.  Where the job cannot be served from the image (a multiallelic variant, a non-founder, chrX among the kept
variants) the [timing] line names the reason and the output is still the reference's."""
import filecmp
import os

import numpy as np
import pytest

import ldtools as T
import het_tools as H
from test_cli import cli  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

DEVICE_LINE = "[timing] --het: from the resident image"
HOST_LINE = "[timing] --het: host pass"


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    """1 % missing, autosomes only, every sample a founder; a sample missing everything (which --mind removes), two monomorphic variants and one
    nobody has a call at"""
    assert T.have_ref()
    d = tmp_path_factory.mktemp("het_dev")
    H.write_fileset(d, H.codes(0.01))
    return d


def three_runs(cli, d, args, tag, zs=False, device=True):
    ref, qualifies = H.reference_runs(d, args, tag, zs)
    assert ref.returncode == 0, ref.stdout[-800:]
    assert qualifies, "the reference's --threads 1 and --threads 4 outputs differ: this fileset is no fixture (pick another seed)"
    dev = H.run_cli(cli, args + ["--timing", "--out", tag], d / "dev")
    host = H.run_cli(cli, args + ["--timing", "--debug-host-filter", "--out", tag], d / "host")
    assert dev.returncode == 0 and host.returncode == 0, (dev.stdout[-1500:], host.stdout[-800:])
    assert HOST_LINE in host.stdout and DEVICE_LINE not in host.stdout and "--debug-host-filter)" in host.stdout, host.stdout[-1500:]
    if device:
        assert DEVICE_LINE in dev.stdout and HOST_LINE not in dev.stdout, dev.stdout[-1500:]
    else:
        assert HOST_LINE in dev.stdout and DEVICE_LINE not in dev.stdout, dev.stdout[-1500:]
    for sub in ("dev", "host"):
        H.assert_same_as_reference(d, sub, tag, zs)
    return ref, dev, host


@pytest.mark.parametrize("fmt", list(H.FORMATS))
@pytest.mark.parametrize("mods", ([], ["small-sample"]), ids=("default", "small-sample"))
def test_alone(gpu_pkg, cli, plain, fmt, mods):
    """no band plan, no pair kernel: the run stops behind the report"""
    tag = "a" + fmt[:1] + fmt[-1] + ("s" if mods else "")
    ref, dev, host = three_runs(cli, plain, H.FORMATS[fmt] + ["--het"] + mods, tag)
    assert "pair kernel" not in dev.stdout and "variants removed" not in dev.stdout, dev.stdout[-1500:]
    assert not os.path.exists(str(plain / "dev" / (tag + ".prune.in")))


def test_beside_the_prune(gpu_pkg, cli, plain):
    ref, dev, host = three_runs(cli, plain, ["--pfile", "../d", "--het"] + H.PRUNE, "p")
    without = H.run_cli(cli, ["--pfile", "../d"] + H.PRUNE + ["--out", "p0"], plain / "dev")
    assert without.returncode == 0, without.stdout[-800:]
    for ext in (".prune.in", ".prune.out"):
        a = str(plain / "ref" / ("p" + ext))
        assert os.path.getsize(str(plain / "ref" / "p.prune.out")) > 20
        for b in (str(plain / "dev" / ("p" + ext)), str(plain / "host" / ("p" + ext)), str(plain / "dev" / ("p0" + ext))):
            assert filecmp.cmp(a, b, shallow=False), b


@pytest.mark.parametrize("fmt", ("bed", "pgen-fixed"))
def test_with_geno_and_maf(gpu_pkg, cli, plain, fmt):
    """after filter_on_device(): the restricted engine's rows are the variants --het counts over"""
    tag = "g" + fmt[:1]
    ref, dev, host = three_runs(cli, plain, H.FORMATS[fmt] + ["--geno", "0.02", "--maf", "0.1", "--het"], tag)
    assert "variant filters: from the device's count pass" in dev.stdout, dev.stdout[-1500:]
    assert "removed due to" in "\n".join(H.het_lines(str(plain / "dev" / (tag + ".log"))))
    ref, dev, host = three_runs(cli, plain, H.FORMATS[fmt] + ["--geno", "0.02", "--maf", "0.1", "--het"] + H.PRUNE, tag + "p")
    for ext in (".prune.in", ".prune.out"):
        assert filecmp.cmp(str(plain / "ref" / (tag + "p" + ext)), str(plain / "dev" / (tag + "p" + ext)), shallow=False), ext


def test_after_a_mind_restart(gpu_pkg, cli, plain):
    """--mind removes the sample that misses everything: the rows are loaded again without it, and --het runs on that image"""
    ref, dev, host = three_runs(cli, plain, ["--pfile", "../d", "--mind", "0.5", "--het"], "m")
    assert "1 sample removed, reloading)" in dev.stdout, dev.stdout[-1500:]
    rows = open(str(plain / "dev" / "m.het")).read().split("\n")
    assert len(rows) == H.N + 1 and not any(r.startswith("s%d\t" % H.S_ALL_MISSING) for r in rows)
    three_runs(cli, plain, ["--pfile", "../d", "--mind", "0.5", "--geno", "0.02", "--het"] + H.PRUNE, "mp")


def test_zs(gpu_pkg, cli, plain):
    three_runs(cli, plain, ["--pfile", "../d", "--het", "zs"], "z", zs=True)


def test_chrx_falls_back_to_the_host(gpu_pkg, cli, tmp_path):
    assert T.have_ref()
    H.write_fileset(tmp_path, H.codes(0.01), names=H.chrom_names(H.M, x=30, mt=10), sexes=[1 + (s % 2) for s in range(H.N)], varwidth=False)
    ref, dev, host = three_runs(cli, tmp_path, ["--pfile", "../d", "--het"], "x", device=False)
    assert "chrX / chrY / MT variants" in dev.stdout, dev.stdout[-1500:]
    # with them filtered out the image serves
    three_runs(cli, tmp_path, ["--pfile", "../d", "--autosome", "--het"], "xa")


def test_nonfounders_fall_back_to_the_host(gpu_pkg, cli, tmp_path):
    assert T.have_ref()
    H.write_fileset(tmp_path, H.codes(0.01), nonfounders=(7, 8, 30), varwidth=False)
    ref, dev, host = three_runs(cli, tmp_path, ["--pfile", "../d", "--het"], "n", device=False)
    assert "non-founders among the kept samples" in dev.stdout, dev.stdout[-1500:]
    three_runs(cli, tmp_path, ["--pfile", "../d", "--het"] + H.PRUNE, "np", device=False)


def test_multiallelic_falls_back_to_the_host(gpu_pkg, cli, tmp_path):
    assert T.have_ref()
    H.write_multiallelic_fileset(tmp_path)
    ref, dev, host = three_runs(cli, tmp_path, ["--pfile", "../v", "--het"], "u", device=False)
    assert "multiallelic variants" in dev.stdout, dev.stdout[-1500:]
    three_runs(cli, tmp_path, ["--pfile", "../v", "--max-alleles", "2", "--het"], "u2")
