"""--hwe and --hardy on the host's pass (plink2-hip --debug-host-filter: the reader's counts, ldp_hwe_ln_p_host) side by side with the reference
binary: .hardy byte for byte under the conditions hwe_tools.qualify_hardy() fixes, the prune lists and the log lines for eight settings, the
order of the filters, a --mind restart, the strictness error and the observation-count warning.  No GPU: --hardy and --hwe beside --hardy need
none on this path; the runs beside --indep-pairwise are in test_hwe_cli_device.py."""
import os

import pytest

import hwe_tools as H
import ldtools as T

pytestmark = pytest.mark.skipif(not T.have_ref(), reason="reference binary not built (oracle/_ref/plink2)")
HOST = ["--debug-host-filter", "--timing"]


@pytest.fixture(scope="module")
def cli(pkg):
    path = pkg.build_cli()
    assert path and os.path.exists(path)
    return path


@pytest.fixture(scope="module")
def fileset_a(tmp_path_factory):
    """600 variants x 400 samples: a quarter of the variants with a het deficit, a quarter with an excess, 2 % missing calls, the four planted rows"""
    d = tmp_path_factory.mktemp("hwe_a")
    raw = H.planted_codes(600, 400, 31)
    H.write_fileset(d, raw)
    return d, raw


@pytest.fixture(scope="module")
def fileset_b(tmp_path_factory):
    """40 variants x 3,000 samples with an all-het variant: p far below DBL_MIN, and the threshold branch below ln = -708.396"""
    d = tmp_path_factory.mktemp("hwe_b")
    raw = H.planted_codes(40, 3000, 32)
    H.write_fileset(d, raw, varwidth=False)
    return d, raw


def both(cli, d, args, tag, fmt="bed"):
    ref = T.run_ref(H.FORMATS[fmt] + args + ["--out", tag], os.path.join(str(d), "ref"))
    got = H.run_cli(cli, H.FORMATS[fmt] + args + HOST + ["--out", tag], os.path.join(str(d), "host"))
    assert got.returncode == ref.returncode, (tag, ref.returncode, got.returncode, got.stdout[-1500:], ref.stdout[-800:])
    if "--hwe" in args or "--hardy" in args:
        assert ("[timing] --hwe / --hardy: host pass" in got.stdout) or got.returncode, got.stdout[-1500:]
    return ref, got


@pytest.mark.parametrize("fmt", ["bed", "pgen-fixed", "pgen-varwidth"])
def test_hardy_report(cli, fileset_a, fmt):
    d, _ = fileset_a
    both(cli, d, ["--hardy"], "h_" + fmt, fmt)
    H.assert_same_hardy(d, "host", "h_" + fmt)


def test_hardy_midp_and_zs(cli, fileset_a, fileset_b):
    d, _ = fileset_a
    both(cli, d, ["--hardy", "midp"], "hm")
    H.assert_same_hardy(d, "host", "hm", midp=True)
    both(cli, d, ["--hardy", "zs"], "hz")
    H.assert_same_hardy(d, "host", "hz", zs=True)
    d, _ = fileset_b
    both(cli, d, ["--hardy"], "hb")
    H.assert_same_hardy(d, "host", "hb")
    both(cli, d, ["--hardy", "midp", "zs"], "hbm")
    H.assert_same_hardy(d, "host", "hbm", midp=True, zs=True)


def test_hardy_behind_geno(cli, fileset_a):
    """--hardy lists what --geno leaves (the count reports list everything: they are written before it)"""
    d, raw = fileset_a
    both(cli, d, ["--geno", "0.03", "--hardy", "--geno-counts"], "hg")
    H.assert_same_hardy(d, "host", "hg")
    hardy = H.read_text(os.path.join(str(d), "host", "hg.hardy")).split(b"\n")
    gcount = open(os.path.join(str(d), "host", "hg.gcount"), "rb").read().split(b"\n")
    assert len(gcount) - 2 == raw.shape[0] and 3 < len(hardy) - 2 < raw.shape[0]


@pytest.mark.parametrize("setting", H.SETTINGS, ids=["_".join(s) for s in H.SETTINGS])
def test_hwe_decisions(cli, fileset_a, setting):
    """--hwe in front of --het (a run of --hardy alone applies no filter behind --geno, in the reference as here): the log line's removal count
    against the reference's and against the rule in exact arithmetic, and the per-sample integer sums of .het, which are sums over exactly the
    variants that stay"""
    d, raw = fileset_a
    tag = "w_" + "_".join(setting).replace("-", "m")
    both(cli, d, ["--hwe"] + setting + ["--het", "--hardy"], tag)
    H.assert_same_log(d, "host", tag)
    H.assert_same_het_counts(d, "host", tag)
    want = H.expected_removals(raw, setting)
    line = [l for l in H.log_lines(os.path.join(str(d), "host", tag + ".log")) if l.startswith("--hwe")][0]
    assert ("%d variant" % int(want.sum())) in line.replace("\n", " "), (line, int(want.sum()))


def test_low_threshold_branch(cli, fileset_b):
    """fileset B's all-het variant (ln p about -2,000) against thresholds below exp(-708.396), where the reference compares logarithms only"""
    d, raw = fileset_b
    for setting in (["1e-300", "0"], ["1e-400", "0"]):
        tag = "b_" + setting[0].replace("-", "m")
        both(cli, d, ["--hwe"] + setting + ["--het", "--hardy"], tag)
        H.assert_same_log(d, "host", tag)
        H.assert_same_het_counts(d, "host", tag)
        want = H.expected_removals(raw, setting)
        assert want[H.V_ALL_HET]
        line = [l for l in H.log_lines(os.path.join(str(d), "host", tag + ".log")) if l.startswith("--hwe")][0]
        assert ("%d variant" % int(want.sum())) in line, (line, int(want.sum()))


def test_hardy_alone_applies_no_filter_behind_geno(cli, fileset_a):
    d, _ = fileset_a
    both(cli, d, ["--geno", "0.03", "--hwe", "0.9", "--maf", "0.05", "--hardy"], "alone")
    H.assert_same_hardy(d, "host", "alone")
    assert [l.split(":")[0] for l in H.log_lines(os.path.join(str(d), "host", "alone.log"))] == ["--geno", "--hardy"]


def test_filter_order(cli, fileset_a):
    """--geno first, --hwe on what it leaves, --maf on what --hwe leaves: the three removal counts"""
    d, raw = fileset_a
    both(cli, d, ["--geno", "0.03", "--hwe", "1e-3", "0", "--maf", "0.05", "--hardy", "--het"], "order")
    H.assert_same_hardy(d, "host", "order")
    H.assert_same_het_counts(d, "host", "order")
    lines = H.log_lines(os.path.join(str(d), "host", "order.log"))
    assert [l.split(":")[0].split(" ")[0] for l in lines[:3]] == ["--geno", "--hardy", "--hwe"] and "allele frequency" in lines[3], lines


def test_strictness_error_and_observation_warning(cli, fileset_a):
    d, _ = fileset_a
    ref, got = both(cli, d, ["--hwe", "0.9", "--het"], "strict")
    assert ref.returncode == 7
    H.assert_same_log(d, "host", "strict")
    assert any(l.startswith("Error: --hwe filter is suspiciously strict") for l in H.log_lines(os.path.join(str(d), "host", "strict.log")))
    # (the planted rows' call counts -- none missing on the all-het row, 2 % elsewhere, few on a thinned row -- differ by more than 10 %)
    ref, got = both(cli, d, ["--hwe", "1e-3", "0", "--het"], "warn")
    H.assert_same_log(d, "host", "warn")
    assert any(l.startswith("Warning: --hwe observation counts vary") for l in H.log_lines(os.path.join(str(d), "host", "warn.log")))


def test_mind_restart(cli, fileset_a):
    d, _ = fileset_a
    both(cli, d, ["--mind", "0.021", "--hwe", "1e-3", "0", "--hardy", "--het"], "mind")
    H.assert_same_hardy(d, "host", "mind")
    H.assert_same_het_counts(d, "host", "mind")
    assert "removed due to missing genotype data (--mind)" in open(os.path.join(str(d), "host", "mind.log")).read()
