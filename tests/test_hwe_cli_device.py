"""--hwe and --hardy through plink2-hip on the GPU, three runs side by side: the reference binary, plink2-hip --debug-host-filter (the reader's
counts, ldp_hwe_ln_p_host) and the device path (the count pass's records, hwe_kernel through ldp_hwe_ln_pvals, one ldp_restrict_variants for all
count filters).  The --timing line proves which path ran.  Compared byte for byte under the conditions fixed in hwe_tools (qualify_hardy,
expected_removals): .hardy, .prune.in / .prune.out and the log lines."""
import os

import numpy as np
import pytest

import hwe_tools as H
import ldtools as T

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not T.have_ref(), reason="reference binary not built (oracle/_ref/plink2)")]
DEVICE_LINE = "[timing] --hwe / --hardy: from the device's records"
HOST_LINE = "[timing] --hwe / --hardy: host pass"


@pytest.fixture(scope="module")
def cli(gpu_pkg):
    path = gpu_pkg.build_cli()
    assert path and os.path.exists(path)
    return path


@pytest.fixture(scope="module")
def fileset_a(tmp_path_factory):
    d = tmp_path_factory.mktemp("hwe_a")
    raw = H.planted_codes(600, 400, 31)
    H.write_fileset(d, raw)
    return d, raw


@pytest.fixture(scope="module")
def fileset_b(tmp_path_factory):
    d = tmp_path_factory.mktemp("hwe_b")
    raw = H.planted_codes(40, 3000, 32)
    H.write_fileset(d, raw, varwidth=False)
    return d, raw


@pytest.fixture(scope="module")
def fileset_c(tmp_path_factory):
    """8 variants x 500,000 samples as .bed (1 MB): the golden file's triples at that sample count, whose exact ln p an evaluation at test time
    could not afford"""
    d = tmp_path_factory.mktemp("hwe_c")
    rows = [g for g in H.golden_large() if g[0] + g[1] + g[2] == 500000]
    assert len(rows) == 8
    raw = np.zeros((8, 500000), dtype=np.uint8)
    rng = np.random.default_rng(33)
    for v, (a, b, c, _, _, _) in enumerate(rows):
        raw[v, a:a + b] = 1
        raw[v, a + b:] = 2
        raw[v] = raw[v, rng.permutation(500000)]
    H.write_fileset(d, raw, names=["1"] * 8, bed_only=True)
    return d, raw, {(a, b, c): (lp, lpm) for a, b, c, lp, lpm, _ in rows}


def three(cli, d, args, tag, fmt="bed", want_rc=0):
    ref = T.run_ref(H.FORMATS[fmt] + args + ["--out", tag], os.path.join(str(d), "ref"))
    host = H.run_cli(cli, H.FORMATS[fmt] + args + ["--debug-host-filter", "--timing", "--out", tag], os.path.join(str(d), "host"))
    dev = H.run_cli(cli, H.FORMATS[fmt] + args + ["--timing", "--out", tag], os.path.join(str(d), "dev"))
    assert ref.returncode == want_rc, ref.stdout[-1500:]
    assert host.returncode == want_rc and dev.returncode == want_rc, (tag, host.returncode, dev.returncode, host.stdout[-1500:], dev.stdout[-1500:])
    assert HOST_LINE in host.stdout and DEVICE_LINE not in host.stdout, host.stdout[-2000:]
    assert DEVICE_LINE in dev.stdout and HOST_LINE not in dev.stdout, dev.stdout[-2000:]
    return ref, host, dev


def same_lists(d, tag):
    for sub in ("host", "dev"):
        for ext in (".prune.in", ".prune.out"):
            want = open(os.path.join(str(d), "ref", tag + ext), "rb").read()
            got = open(os.path.join(str(d), sub, tag + ext), "rb").read()
            assert got == want, (sub, tag, ext, len(want), len(got))
        H.assert_same_log(d, sub, tag)


@pytest.mark.parametrize("fmt", ["bed", "pgen-fixed", "pgen-varwidth"])
def test_hardy_alone_and_beside_the_prune(cli, fileset_a, fmt):
    d, _ = fileset_a
    three(cli, d, ["--hardy"], "h_" + fmt, fmt)
    three(cli, d, ["--hardy"] + H.PRUNE, "hp_" + fmt, fmt)
    for sub in ("host", "dev"):
        H.assert_same_hardy(d, sub, "h_" + fmt)
        H.assert_same_hardy(d, sub, "hp_" + fmt)
    same_lists(d, "hp_" + fmt)


def test_hardy_midp_and_zs(cli, fileset_a, fileset_b):
    d, _ = fileset_a
    three(cli, d, ["--hardy", "midp"], "hm")
    three(cli, d, ["--hardy", "zs"], "hz")
    db, _ = fileset_b
    three(cli, db, ["--hardy"], "hb")
    three(cli, db, ["--hardy", "midp", "zs"] + H.PRUNE, "hbm")
    for sub in ("host", "dev"):
        H.assert_same_hardy(d, sub, "hm", midp=True)
        H.assert_same_hardy(d, sub, "hz", zs=True)
        H.assert_same_hardy(db, sub, "hb")
        H.assert_same_hardy(db, sub, "hbm", midp=True, zs=True)


@pytest.mark.parametrize("setting", H.SETTINGS, ids=["_".join(s) for s in H.SETTINGS])
def test_hwe_decisions(cli, fileset_a, setting):
    """every variant's decision: the prune lists hold exactly the variants the filter left, and the log line's count is the rule's in exact
    arithmetic (after the assertion that no variant sits within 1e-5 of its threshold)"""
    d, raw = fileset_a
    tag = "w_" + "_".join(setting).replace("-", "m")
    want = H.expected_removals(raw, setting)
    three(cli, d, ["--hwe"] + setting + H.PRUNE, tag)
    same_lists(d, tag)
    listed = sum(len(T.read_id_list(os.path.join(str(d), "dev", tag + ext))) for ext in (".prune.in", ".prune.out"))
    assert listed == raw.shape[0] - int(want.sum())
    # a different `midp` for the report beside it: two sets of p-values from one load
    three(cli, d, ["--hwe"] + setting + ["--hardy"] + ([] if "midp" in setting else ["midp"]) + H.PRUNE, tag + "_h")
    same_lists(d, tag + "_h")
    for sub in ("host", "dev"):
        H.assert_same_hardy(d, sub, tag + "_h", midp="midp" not in setting)


def test_low_threshold_branch(cli, fileset_b):
    d, raw = fileset_b
    for setting in (["1e-300", "0"], ["1e-400", "0"]):
        tag = "b_" + setting[0].replace("-", "m")
        want = H.expected_removals(raw, setting)
        assert want[H.V_ALL_HET]
        three(cli, d, ["--hwe"] + setting + H.PRUNE, tag)
        same_lists(d, tag)
        listed = sum(len(T.read_id_list(os.path.join(str(d), "dev", tag + ext))) for ext in (".prune.in", ".prune.out"))
        assert listed == raw.shape[0] - int(want.sum())


def test_filter_order_and_mind_restart(cli, fileset_a):
    """--geno, then --hardy over what it leaves, then --hwe, then --maf: the three removal counts show the order; and the same after --mind has
    removed samples and the run has started over"""
    d, _ = fileset_a
    three(cli, d, ["--geno", "0.03", "--hwe", "1e-3", "0", "--maf", "0.05", "--hardy"] + H.PRUNE, "order")
    same_lists(d, "order")
    three(cli, d, ["--mind", "0.021", "--geno", "0.03", "--hwe", "1e-2", "0.01", "midp", "keep-fewhet", "--maf", "0.05", "--hardy"] + H.PRUNE, "mind")
    same_lists(d, "mind")
    for sub in ("host", "dev"):
        H.assert_same_hardy(d, sub, "order")
        H.assert_same_hardy(d, sub, "mind")
        lines = H.log_lines(os.path.join(str(d), sub, "order.log"))
        assert [l.split(":")[0].split(" ")[0] for l in lines[:3]] == ["--geno", "--hardy", "--hwe"] and "allele frequency" in lines[3], lines
        assert "(--mind)" in open(os.path.join(str(d), sub, "mind.log")).read()


def test_strictness_error_and_observation_warning(cli, fileset_a):
    d, _ = fileset_a
    three(cli, d, ["--hwe", "0.9"] + H.PRUNE, "strict", want_rc=7)
    three(cli, d, ["--hwe", "1e-3", "0"] + H.PRUNE, "warn")
    for sub in ("host", "dev"):
        H.assert_same_log(d, sub, "strict")
        assert any(l.startswith("Error: --hwe filter is suspiciously strict") for l in H.log_lines(os.path.join(str(d), sub, "strict.log")))
        assert any(l.startswith("Warning: --hwe observation counts vary") for l in H.log_lines(os.path.join(str(d), sub, "warn.log")))
    same_lists(d, "warn")


def test_half_a_million_samples(cli, fileset_c):
    d, raw, golden = fileset_c
    exact = lambda a, b, c, midp: golden[(a, b, c)][1 if midp else 0]   # noqa: E731
    three(cli, d, ["--hardy"], "c")
    three(cli, d, ["--hardy", "midp", "--hwe", "1e-6", "0.001"] + H.PRUNE, "cm")
    for sub in ("host", "dev"):
        H.assert_same_hardy(d, sub, "c", exact=exact)
        H.assert_same_hardy(d, sub, "cm", midp=True, exact=exact)
    same_lists(d, "cm")
    # the rule on the golden values: ln p against ln(1e-6) (1 + 2^-44) - 500 ln 10
    removed = sum(1 for (a, b, c), (lp, _) in golden.items() if lp < H.threshold_ln(["1e-6", "0.001"], 500000))
    assert all(abs(lp - H.threshold_ln(["1e-6", "0.001"], 500000)) > 1e-5 for lp, _ in golden.values())
    line = [l for l in H.log_lines(os.path.join(str(d), "dev", "cm.log")) if l.startswith("--hwe")][0]
    assert ("%d variant" % removed) in line, (line, removed)
