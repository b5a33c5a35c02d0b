"""plink2-hip --mind against the reference binary and against its own host pass, three runs per case as in test_filter_on_device.py: the
reference, plink2-hip deciding from the resident image (ldp_sample_missing_counts; the [timing] line says so, and says whether the run started
over without the removed samples), and plink2-hip --debug-host-filter (the host's pass over the rows).  Log lines, <out>.mindrem.id and the
prune lists must be the same bytes everywhere.  The tools run in sub-directories of the fileset's directory with the same --out name, so that
the log line naming the file is the same text."""
import filecmp
import os

import numpy as np
import pytest

import ldtools as T
import mind_tools as MT
from test_cli import cli, run_cli  # noqa: F401  (fixture)
from test_clump import write_report

pytestmark = pytest.mark.gpu

DEVICE_LINE = "sample filter (--mind): from the resident image"
HOST_LINE = "sample filter (--mind): host pass"


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    assert T.have_ref()
    d = tmp_path_factory.mktemp("mind_planted")
    raw = MT.planted_codes()
    MT.write_fileset(d, raw)
    return d, raw


@pytest.fixture(scope="module")
def planted_block(tmp_path_factory):
    assert T.have_ref()
    d = tmp_path_factory.mktemp("mind_block")
    raw = MT.planted_codes(block=True)
    MT.write_fileset(d, raw, with_varwidth=False)
    return d, raw


def three_runs(cli, d, args, tag):
    ref = T.run_ref(args + ["--threads", "4", "--out", tag], str(d / "ref"))
    dev = run_cli(cli, args + ["--timing", "--out", tag], str(d / "dev"))
    host = run_cli(cli, args + ["--timing", "--debug-host-filter", "--out", tag], str(d / "host"))
    return ref, dev, host


def same_file(d, tag, ext):
    a = str(d / "ref" / (tag + ext))
    return filecmp.cmp(a, str(d / "dev" / (tag + ext)), shallow=False) and filecmp.cmp(a, str(d / "host" / (tag + ext)), shallow=False)


def test_nothing_removed_keeps_the_image(gpu_pkg, cli, planted):
    """--mind 0.5: nobody misses half the calls -- one read of the image, no reload, no .mindrem.id from either tool"""
    d, _ = planted
    args = MT.FORMATS["pgen-fixed"] + ["--mind", "0.5"] + MT.PRUNE
    ref, dev, host = three_runs(cli, d, args, "none")
    assert ref.returncode == 0 and dev.returncode == 0 and host.returncode == 0, (ref.stdout[-600:], dev.stdout[-1500:], host.stdout[-600:])
    assert DEVICE_LINE in dev.stdout and HOST_LINE not in dev.stdout and "reloading" not in dev.stdout, dev.stdout[-1500:]
    assert "0 samples removed)" in dev.stdout
    assert HOST_LINE in host.stdout and DEVICE_LINE not in host.stdout, host.stdout[-1500:]
    want = MT.mind_lines(ref.stdout)
    assert want == ["0 samples removed due to missing genotype data (--mind)."]
    assert MT.mind_lines(dev.stdout) == want and MT.mind_lines(host.stdout) == want
    for sub in ("ref", "dev", "host"):
        assert not os.path.exists(str(d / sub / "none.mindrem.id")), sub
    for ext in (".prune.in", ".prune.out"):
        assert same_file(d, "none", ext), ext
    assert os.path.getsize(str(d / "ref" / "none.prune.in")) > 20


@pytest.mark.parametrize("fmt", list(MT.FORMATS))
def test_some_removed_reloads_without_them(gpu_pkg, cli, planted, fmt):
    d, raw = planted
    args = MT.FORMATS[fmt] + ["--mind", "0.1"] + MT.PRUNE
    ref, dev, host = three_runs(cli, d, args, fmt)
    assert ref.returncode == 0 and dev.returncode == 0 and host.returncode == 0, (ref.stdout[-600:], dev.stdout[-1500:], host.stdout[-600:])
    assert DEVICE_LINE in dev.stdout and HOST_LINE not in dev.stdout, dev.stdout[-1500:]
    assert "4 samples removed, reloading)" in dev.stdout, dev.stdout[-1500:]
    assert HOST_LINE in host.stdout and DEVICE_LINE not in host.stdout, host.stdout[-1500:]
    assert MT.read_mindrem(str(d / "ref" / (fmt + ".mindrem.id"))) == ["s%d" % s for s in MT.expected_removed(raw)]
    want = MT.mind_lines(ref.stdout)
    assert want == ["4 samples removed due to missing genotype data (--mind).", "IDs written to %s.mindrem.id ." % fmt]
    assert MT.mind_lines(dev.stdout) == want, dev.stdout      # (printed once, although the inputs were read twice)
    assert MT.mind_lines(host.stdout) == want, host.stdout
    for ext in (".mindrem.id", ".prune.in", ".prune.out"):
        assert same_file(d, fmt, ext), ext
    assert os.path.getsize(str(d / "ref" / (fmt + ".prune.in"))) > 20


@pytest.mark.parametrize("fmt", ["bed", "pgen-fixed"])
def test_mind_comes_before_geno_and_maf(gpu_pkg, cli, planted_block, fmt):
    """the planted samples' missing calls sit in one block of variants: with those samples gone --geno keeps variants it would have removed"""
    d, _ = planted_block
    filters = ["--geno", "0.02", "--maf", "0.05"]
    without = T.run_ref(MT.FORMATS[fmt] + filters + MT.PRUNE + ["--threads", "4", "--out", fmt + "_nomind"], str(d / "ref"))
    ref, dev, host = three_runs(cli, d, MT.FORMATS[fmt] + ["--mind", "0.1"] + filters + MT.PRUNE, fmt)
    assert without.returncode == 0 and ref.returncode == 0, (without.stdout[-600:], ref.stdout[-600:])
    geno = lambda out: [l for l in MT.removed_due_to_lines(out) if l.startswith("--geno")]   # noqa: E731
    assert geno(without.stdout) and geno(ref.stdout) and geno(without.stdout) != geno(ref.stdout), "the fileset does not tell the orders apart"
    assert dev.returncode == 0 and host.returncode == 0, (dev.stdout[-1500:], host.stdout[-800:])
    assert DEVICE_LINE in dev.stdout and "reloading" in dev.stdout and "variant filters: from the device's count pass" in dev.stdout, dev.stdout[-1500:]
    assert HOST_LINE in host.stdout and "variant filters: host pass" in host.stdout, host.stdout[-1500:]
    want = MT.removed_due_to_lines(ref.stdout)
    assert len(want) == 3 and MT.removed_due_to_lines(dev.stdout) == want and MT.removed_due_to_lines(host.stdout) == want, (want, dev.stdout[-1500:])
    for ext in (".mindrem.id", ".prune.in", ".prune.out"):
        assert same_file(d, fmt, ext), ext


def test_everybody_removed(gpu_pkg, cli, planted):
    d, raw = planted
    assert ((raw == 3).sum(axis=0) > 0).all()
    ref, dev, host = three_runs(cli, d, MT.FORMATS["pgen-fixed"] + ["--mind", "0"] + MT.PRUNE, "all")
    assert ref.returncode == dev.returncode == host.returncode == 13, (ref.returncode, dev.returncode, host.returncode, dev.stdout[-800:])
    message = "Error: No samples remaining after main filters."
    assert message in ref.stdout and message in dev.stdout and message in host.stdout
    want = MT.mind_lines(ref.stdout)
    assert want and want[0].startswith("150 samples removed") and MT.mind_lines(dev.stdout) == want and MT.mind_lines(host.stdout) == want
    assert same_file(d, "all", ".mindrem.id")


def test_fewer_than_fifty_founders_after_mind(gpu_pkg, cli, tmp_path):
    assert T.have_ref()
    m, n = MT.M, 60
    raw = T.synth_raw_codes(m, n, 8, missing_rate=0.01).copy()
    raw[:, :15][np.random.default_rng(8).random((m, 15)) < 0.3] = 3     # fifteen samples miss about 30 %: 45 are left
    names, pos = MT.positions()
    T.write_pgen_fixed(str(tmp_path / "d"), raw, names, pos)
    for sub in ("ref", "dev", "host"):
        os.makedirs(str(tmp_path / sub))
    ref, dev, host = three_runs(cli, tmp_path, ["--pfile", "../d", "--mind", "0.1"] + MT.PRUNE, "few")
    assert ref.returncode != 0 and ref.returncode == dev.returncode == host.returncode, (ref.returncode, dev.returncode, host.returncode, dev.stdout[-800:])
    assert "less than 50" in ref.stdout and "less than 50" in dev.stdout and "less than 50" in host.stdout
    assert MT.mind_lines(dev.stdout) == MT.mind_lines(ref.stdout) == MT.mind_lines(host.stdout)
    assert "15 samples removed" in MT.mind_lines(ref.stdout)[0]


def test_r2_table_and_clump_take_the_host_pass(gpu_pkg, cli, planted):
    d, _ = planted
    write_report(str(d / "assoc.txt"), MT.M, 4)
    for tag, cmd, ext in (("vcor", ["--r2-unphased", "--ld-window-r2", "0.2"], ".vcor"),
                          ("clump", ["--clump", "../assoc.txt", "--clump-unphased"], ".clumps")):
        args = MT.FORMATS["pgen-fixed"] + ["--mind", "0.1"] + cmd
        ref = T.run_ref(args + ["--threads", "4", "--out", tag], str(d / "ref"))
        got = run_cli(cli, args + ["--timing", "--out", tag], str(d / "dev"))
        assert ref.returncode == 0 and got.returncode == 0, (ref.stdout[-800:], got.stdout[-1500:])
        assert HOST_LINE in got.stdout and DEVICE_LINE not in got.stdout, got.stdout[-1500:]
        assert MT.mind_lines(got.stdout) == MT.mind_lines(ref.stdout)
        a, b = str(d / "ref" / (tag + ext)), str(d / "dev" / (tag + ext))
        assert os.path.getsize(a) > 200, tag
        assert filecmp.cmp(a, b, shallow=False), tag
        assert filecmp.cmp(str(d / "ref" / (tag + ".mindrem.id")), str(d / "dev" / (tag + ".mindrem.id")), shallow=False)
