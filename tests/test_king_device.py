"""plink2-hip --make-king-table on the GPU: three runs per case -- the reference, plink2-hip reading the resident image (ldp_king_counts_block /
ldp_king_block_hits; the [timing] line says so) and plink2-hip --debug-host-filter (the host's popcount pass) -- with <out>.kin0 the same
bytes everywhere and the same log lines, on a fileset of 300 samples x 2,000 variants.  Where the job cannot be served from the image (a
non-founder, chrX among the kept variants, a multiallelic variant) the [timing] line names the reason and the output is still the
reference's."""
import filecmp
import os

import numpy as np
import pytest

import het_tools as H
import king_tools as K
import ldtools as T
from test_cli import cli  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

DEVICE_LINE = "[timing] --make-king-table: from the resident image"
HOST_LINE = "[timing] --make-king-table: host pass"
M, N = 2000, 300


def codes():
    raw = H.codes(0.02, m=M, n=N).copy()      # sample 5 misses every call (--mind removes it), variant 11 is missed by everybody
    raw[:, 9] = np.where(raw[:, 9] == 1, 2, raw[:, 9])   # never het
    raw[:, 31] = raw[:, 30]                   # identical samples
    return raw


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    assert T.have_ref()
    d = tmp_path_factory.mktemp("king_dev")
    H.write_fileset(d, codes(), names=H.chrom_names(M))
    return d


def three_runs(cli, d, args, tag, zs=False, id_file=False, device=True):
    ref = T.run_ref(args + ["--out", tag], str(d / "ref"))
    assert ref.returncode == 0, ref.stdout[-800:]
    dev = H.run_cli(cli, args + ["--timing", "--out", tag], d / "dev")
    host = H.run_cli(cli, args + ["--timing", "--debug-host-filter", "--out", tag], d / "host")
    assert dev.returncode == 0 and host.returncode == 0, (dev.stdout[-1500:], host.stdout[-800:])
    assert HOST_LINE in host.stdout and DEVICE_LINE not in host.stdout and "--debug-host-filter)" in host.stdout, host.stdout[-1500:]
    if device:
        assert DEVICE_LINE in dev.stdout and HOST_LINE not in dev.stdout, dev.stdout[-1500:]
    else:
        assert HOST_LINE in dev.stdout and DEVICE_LINE not in dev.stdout, dev.stdout[-1500:]
    for sub in ("dev", "host"):
        K.assert_same_as_reference(d, sub, tag, zs, id_file)
    return ref, dev, host


@pytest.mark.parametrize("fmt", list(H.FORMATS))
def test_alone(gpu_pkg, cli, plain, fmt):
    """no band plan, no prune: the run stops behind the table; nan lines (a sample without a call) and -inf lines (one without a het call)"""
    tag = "a" + fmt[:1] + fmt[-1]
    ref, dev, host = three_runs(cli, plain, H.FORMATS[fmt] + ["--make-king-table"], tag)
    assert "dense form" in dev.stdout and "variants removed" not in dev.stdout, dev.stdout[-1500:]
    text = open(str(plain / "dev" / (tag + ".kin0"))).read()
    assert text.count("\n") == 1 + N * (N - 1) // 2 and "\tnan\n" in text and "\t-inf\n" in text
    assert not os.path.exists(str(plain / "dev" / (tag + ".prune.in")))


@pytest.mark.parametrize("thr", ("0.0884", "0.3", "-0.5"))
def test_with_king_table_filter(gpu_pkg, cli, plain, thr):
    """the hit form: the device drops the pairs below the threshold, nan pairs stay, -inf pairs go"""
    tag = "f" + thr.replace(".", "").replace("-", "m")
    ref, dev, host = three_runs(cli, plain, ["--pfile", "../d", "--make-king-table", "--king-table-filter", thr], tag)
    assert "hit form" in dev.stdout and "--king-table-filter: " in dev.stdout, dev.stdout[-1500:]
    text = open(str(plain / "dev" / (tag + ".kin0"))).read()
    assert "\tnan\n" in text and "-inf" not in text


@pytest.mark.parametrize("mods,tag,id_file", (
    (["counts"], "c", False),
    (["cols=id,nsnp,hethet,ibs0,ibs1,ibs,kinship"], "i", False),
    (["counts", "cols=nsnp,ibs1,ibs"], "n", True),
    (["zs", "counts", "cols=fid,id,sid,ibs0,kinship", "--king-table-filter", "0.1"], "z", False),
), ids=("counts", "ibs1-ibs", "no-id", "zs-fid-sid-filter"))
def test_counts_and_cols(gpu_pkg, cli, plain, mods, tag, id_file):
    three_runs(cli, plain, ["--bfile", "../d", "--make-king-table"] + mods, "k" + tag, zs=("zs" in mods), id_file=id_file)


def test_beside_the_prune(gpu_pkg, cli, plain):
    ref, dev, host = three_runs(cli, plain, ["--pfile", "../d", "--make-king-table", "counts"] + H.PRUNE, "p")
    without = H.run_cli(cli, ["--pfile", "../d"] + H.PRUNE + ["--out", "p0"], plain / "dev")
    assert without.returncode == 0, without.stdout[-800:]
    assert os.path.getsize(str(plain / "ref" / "p.prune.out")) > 20
    for ext in (".prune.in", ".prune.out"):
        a = str(plain / "ref" / ("p" + ext))
        for b in (str(plain / "dev" / ("p" + ext)), str(plain / "host" / ("p" + ext)), str(plain / "dev" / ("p0" + ext))):
            assert filecmp.cmp(a, b, shallow=False), b


def test_behind_geno_and_maf_and_beside_het(gpu_pkg, cli, plain):
    """after filter_on_device(): the restricted engine's rows are the variants the table counts over"""
    ref, dev, host = three_runs(cli, plain, ["--pfile", "../d", "--geno", "0.03", "--maf", "0.1", "--make-king-table"], "g")
    assert "variant filters: from the device's count pass" in dev.stdout, dev.stdout[-1500:]
    assert "removed due to" in "\n".join(K.king_lines(str(plain / "dev" / "g.log")))
    assert not filecmp.cmp(str(plain / "dev" / "g.kin0"), str(plain / "dev" / "apd.kin0"), shallow=False) if os.path.exists(str(plain / "dev" / "apd.kin0")) else True
    ref, dev, host = three_runs(cli, plain, ["--bfile", "../d", "--geno", "0.03", "--maf", "0.1", "--het", "--make-king-table", "--king-table-filter", "0.05"] + H.PRUNE, "gp")
    assert "[timing] --het: from the resident image" in dev.stdout
    for ext in (".prune.in", ".prune.out", ".het"):
        assert filecmp.cmp(str(plain / "ref" / ("gp" + ext)), str(plain / "dev" / ("gp" + ext)), shallow=False), ext


def test_after_a_mind_restart(gpu_pkg, cli, plain):
    """--mind removes the sample that misses everything: the rows are loaded again without it, and the table is made from that image"""
    ref, dev, host = three_runs(cli, plain, ["--pfile", "../d", "--mind", "0.5", "--make-king-table"], "m")
    assert "1 sample removed, reloading)" in dev.stdout, dev.stdout[-1500:]
    text = open(str(plain / "dev" / "m.kin0")).read()
    assert text.count("\n") == 1 + (N - 1) * (N - 2) // 2 and "\tnan\n" not in text and "s5\t" not in text


def test_nonfounders_fall_back_to_the_host(gpu_pkg, cli, tmp_path):
    assert T.have_ref()
    H.write_fileset(tmp_path, codes()[:600], nonfounders=(7, 8, 30), varwidth=False)
    ref, dev, host = three_runs(cli, tmp_path, ["--pfile", "../d", "--make-king-table"], "n", device=False)
    assert "non-founders among the kept samples" in dev.stdout, dev.stdout[-1500:]
    three_runs(cli, tmp_path, ["--pfile", "../d", "--make-king-table", "--king-table-filter", "0.1"] + H.PRUNE, "np", device=False)


def test_chrx_falls_back_to_the_host(gpu_pkg, cli, tmp_path):
    assert T.have_ref()
    H.write_fileset(tmp_path, codes()[:600], names=H.chrom_names(600, x=30, mt=10), sexes=[1 + (s % 2) for s in range(N)], varwidth=False)
    ref, dev, host = three_runs(cli, tmp_path, ["--pfile", "../d", "--make-king-table"], "x", device=False)
    assert "chrX / chrY / MT variants" in dev.stdout and "Excluding 40 variants on non-autosomes from KING-robust calculation." in dev.stdout, dev.stdout[-1500:]
    # with them filtered out the image serves
    three_runs(cli, tmp_path, ["--pfile", "../d", "--autosome", "--make-king-table"], "xa")


def test_multiallelic_falls_back_to_the_host(gpu_pkg, cli, tmp_path):
    assert T.have_ref()
    H.write_multiallelic_fileset(tmp_path)
    ref, dev, host = three_runs(cli, tmp_path, ["--pfile", "../v", "--make-king-table"], "u", device=False)
    assert "multiallelic variants" in dev.stdout, dev.stdout[-1500:]
    three_runs(cli, tmp_path, ["--pfile", "../v", "--max-alleles", "2", "--make-king-table"], "u2")
