"""plink2-hip --het on the CPU: every accepted form gets past the argument checks (exit 0, or 16 "no usable HIP device" where there is no GPU,
and 0 on any machine through the host's pass), `cols=` and what else is not built is refused by name (exit 63), what the reference rejects
is rejected with its message and its exit code, and the data --het does not cover is refused from the tables, before any device is touched."""
import os

import numpy as np
import pytest

import ldtools as T
import het_tools as H


@pytest.fixture(scope="module")
def cli():
    import __graft_entry__ as ge
    return ge.load_package().build_cli()


def _files(d, chroms=None, m=40, n=60, nonfounders=()):
    raw = T.synth_raw_codes(m, n, seed=3, missing_rate=0.02)
    T.write_pgen_fixed(str(d / "d"), raw, chroms or ["1"] * m, np.arange(m) * 10 + 1)
    T.write_bed(str(d / "d"), raw, chroms or ["1"] * m, np.arange(m) * 10 + 1)
    if nonfounders:
        with open(str(d / "d.psam"), "w") as f:
            f.write("#IID\tPAT\tMAT\tSEX\n")
            for s in range(n):
                f.write("s%d\t%s\t%s\t2\n" % (s, "p1" if s in nonfounders else "0", "p2" if s in nonfounders else "0"))


def past_the_argument_checks(r):
    # 0 where there is a GPU; 16 = "no usable HIP device" where there is none: past every argument and table check either way
    assert r.returncode in (0, 16), r.stdout
    assert (r.returncode == 0) or ("no usable HIP device" in r.stdout), r.stdout
    assert "not supported" not in r.stdout and "Unrecognized" not in r.stdout and "Invalid" not in r.stdout, r.stdout


PRUNE = ["--indep-pairwise", "50", "5", "0.2"]
ACCEPTED = [["--het"], ["--het", "zs"], ["--het", "small-sample"], ["--het", "zs", "small-sample"], ["--het", "small-sample", "zs"]]


@pytest.mark.parametrize("args", ACCEPTED, ids=lambda a: " ".join(a))
def test_accepted_forms(cli, tmp_path, args):
    _files(tmp_path)
    for src in ("--pfile", "--bfile"):
        past_the_argument_checks(H.run_cli(cli, [src, "d"] + args + PRUNE + ["--out", "o"], tmp_path))     # beside the prune
        past_the_argument_checks(H.run_cli(cli, [src, "d"] + args + ["--out", "o"], tmp_path))             # alone: a valid run
        past_the_argument_checks(H.run_cli(cli, [src, "d"] + args + ["--geno", "0.1", "--maf", "0.05", "--mind", "0.5", "--out", "o"], tmp_path))
    # the host's pass needs no device at all: --het alone ends with exit 0 on any machine, and so does --het beside an r^2 command's refusal-free parse
    r = H.run_cli(cli, ["--pfile", "d"] + args + ["--debug-host-filter", "--out", "o"], tmp_path)
    ext = ".het.zst" if "zs" in args else ".het"
    assert r.returncode == 0 and ("--het: Results written to o%s ." % ext) in r.stdout and os.path.getsize(str(tmp_path / ("o" + ext))) > 20, r.stdout


def test_het_alone_is_a_command(cli, tmp_path):
    _files(tmp_path)
    r = H.run_cli(cli, ["--pfile", "d", "--out", "o"], tmp_path)
    assert r.returncode == 8 and "no command given" in r.stdout
    r = H.run_cli(cli, ["--pfile", "d", "--het", "--dry-run", "--out", "o"], tmp_path)
    assert r.returncode == 0 and "dry-run: --het: host pass: --dry-run" in r.stdout, r.stdout


def test_cols_is_refused_by_name(cli, tmp_path):
    _files(tmp_path)
    for mod in ("cols=hom,f", "cols=+het", "cols="):
        r = H.run_cli(cli, ["--pfile", "d", "--het", mod, "--out", "o"], tmp_path)
        assert r.returncode == 63 and ("'%s' modifier of --het" % mod) in r.stdout, (r.returncode, r.stdout)
        assert not os.path.exists(str(tmp_path / "o.het"))
    r = H.run_cli(cli, ["--pfile", "d", "--het", "--read-freq", "x.afreq", "--out", "o"], tmp_path)
    assert r.returncode == 63 and "--read-freq is not supported" in r.stdout, (r.returncode, r.stdout)


@pytest.mark.parametrize("mods", (["bogus"], ["zs", "Small-Sample"], ["zs", "small-sample", "zs", "zs"], ["0.1"]), ids=lambda a: " ".join(a))
def test_what_the_reference_rejects(cli, tmp_path, mods):
    """the reference's message and exit status (its own output is the yardstick where the binary is there)"""
    _files(tmp_path)
    r = H.run_cli(cli, ["--pfile", "d", "--het"] + mods + ["--out", "o"], tmp_path)
    assert r.returncode != 0 and not os.path.exists(str(tmp_path / "o.het"))
    errors = [l for l in r.stdout.split("\n") if l.startswith("Error:")]
    if len(mods) > 3:
        assert errors == ["Error: --het accepts at most 3 arguments."], r.stdout
    else:
        bad = [m for m in mods if m not in ("zs", "small-sample")][0]
        assert errors == ["Error: Invalid --het argument '%s'." % bad], r.stdout
    if T.have_ref():
        ref = T.run_ref(["--pfile", "d", "--het"] + mods + ["--out", "r"], str(tmp_path))
        assert ref.returncode == r.returncode, (ref.returncode, r.returncode, ref.stdout[-400:])
        assert [l for l in ref.stdout.split("\n") if l.startswith("Error:")] == errors, ref.stdout[-400:]


def test_small_sample_needs_founders(cli, tmp_path):
    _files(tmp_path, nonfounders=set(range(60)))
    r = H.run_cli(cli, ["--pfile", "d", "--het", "small-sample", "--out", "o"], tmp_path)
    assert r.returncode == 7 and "Error: '--het small-sample' requires founders." in r.stdout, (r.returncode, r.stdout)
    if T.have_ref():
        ref = T.run_ref(["--pfile", "d", "--het", "small-sample", "--out", "r"], str(tmp_path))
        assert ref.returncode == 7 and "Error: '--het small-sample' requires founders." in ref.stdout, ref.stdout[-400:]
    # without the modifier the reference asks for decent allele frequencies: fewer than 50 founders are an error unless --bad-freqs is given,
    # and then every allele frequency is 1/2 and the report is written
    r = H.run_cli(cli, ["--pfile", "d", "--het", "--out", "o"], tmp_path)
    assert r.returncode == 13 and "less than 50 founders are available" in r.stdout and "--bad-freqs" in r.stdout, (r.returncode, r.stdout)
    r = H.run_cli(cli, ["--pfile", "d", "--het", "--bad-freqs", "--out", "o"], tmp_path)
    assert r.returncode == 0, r.stdout
    if T.have_ref():
        ref = T.run_ref(["--pfile", "d", "--het", "--out", "r"], str(tmp_path))
        errors = lambda out: out[out.index("Error:"):].split("End time")[0].rstrip()   # noqa: E731
        assert ref.returncode == 13 and errors(ref.stdout) == errors(H.run_cli(cli, ["--pfile", "d", "--het", "--out", "o2"], tmp_path).stdout), ref.stdout[-900:]
        ref = T.run_ref(["--pfile", "d", "--het", "--bad-freqs", "--out", "r"], str(tmp_path))
        assert ref.returncode == 0 and open(str(tmp_path / "r.het"), "rb").read() == open(str(tmp_path / "o.het"), "rb").read()


def test_fewer_than_fifty_samples(cli, tmp_path):
    raw = T.synth_raw_codes(40, 30, seed=3, missing_rate=0.02)
    T.write_pgen_fixed(str(tmp_path / "d"), raw, ["1"] * 40, np.arange(40) * 10 + 1)
    r = H.run_cli(cli, ["--pfile", "d", "--het", "--out", "o"], tmp_path)
    assert r.returncode == 13 and "less than 50 samples are available" in r.stdout, (r.returncode, r.stdout)
    for extra in (["--bad-freqs"], ["small-sample"]):
        r = H.run_cli(cli, ["--pfile", "d", "--het"] + extra + ["--debug-host-filter", "--out", "o"], tmp_path)
        assert r.returncode == 0, r.stdout
        if T.have_ref():
            ref = T.run_ref(["--pfile", "d", "--het"] + extra + ["--out", "r"], str(tmp_path))
            assert ref.returncode == 0 and open(str(tmp_path / "r.het"), "rb").read() == open(str(tmp_path / "o.het"), "rb").read(), extra
    if T.have_ref():
        ref = T.run_ref(["--pfile", "d", "--het", "--out", "r"], str(tmp_path))
        r = H.run_cli(cli, ["--pfile", "d", "--het", "--out", "o"], tmp_path)
        errors = lambda out: out[out.index("Error:"):].split("End time")[0].rstrip()   # noqa: E731
        assert ref.returncode == 13 and errors(ref.stdout) == errors(r.stdout), ref.stdout[-900:]


def test_chromosome_zero_beside_the_prune_is_refused(cli, tmp_path):
    """the prune strips unplaced variants from its list, --het counts them as autosomal: one list is kept, so the combination is refused by name;
    alone, --het takes them as the reference does"""
    _files(tmp_path, chroms=["0"] * 5 + ["1"] * 35)
    r = H.run_cli(cli, ["--pfile", "d", "--het"] + PRUNE + ["--out", "o"], tmp_path)
    assert r.returncode == 63 and "chromosome 0" in r.stdout and "snp0" in r.stdout, (r.returncode, r.stdout)
    r = H.run_cli(cli, ["--pfile", "d", "--het", "--debug-host-filter", "--out", "o"], tmp_path)
    assert r.returncode == 0, r.stdout
    if T.have_ref():
        ref = T.run_ref(["--pfile", "d", "--het", "--out", "r"], str(tmp_path))
        assert ref.returncode == 0 and open(str(tmp_path / "r.het"), "rb").read() == open(str(tmp_path / "o.het"), "rb").read()


def test_dosage_tracks_are_refused(cli, tmp_path):
    if not T.have_ref():
        pytest.skip("needs the reference binary (it writes the fileset)")
    cp = T.run_ref(["--dummy", "60", "40", "dosage-freq=0.4", "--seed", "3", "--make-pgen", "--out", "dos"], str(tmp_path))
    assert cp.returncode == 0, cp.stdout[-800:]
    for args in (["--het"], ["--het", "small-sample"], ["--het"] + PRUNE, ["--het", "--debug-host-filter"]):
        r = H.run_cli(cli, ["--pfile", "dos"] + args + ["--out", "o"], tmp_path)
        assert r.returncode == 63 and "dosage" in r.stdout and "dos.pgen" in r.stdout, (r.returncode, r.stdout)


def test_beside_the_r2_commands_the_host_pass_runs_first(cli, tmp_path):
    """--r2-unphased plans its engine before the load: --het beside it is served by the host's pass, whose file is complete before any device is
    asked for"""
    _files(tmp_path)
    r = H.run_cli(cli, ["--pfile", "d", "--het", "--r2-unphased", "square", "--out", "o"], tmp_path)
    past_the_argument_checks(r)
    assert "--het: Results written to o.het ." in r.stdout, r.stdout
    alone = H.run_cli(cli, ["--pfile", "d", "--het", "--debug-host-filter", "--out", "a"], tmp_path)
    assert alone.returncode == 0 and open(str(tmp_path / "o.het"), "rb").read() == open(str(tmp_path / "a.het"), "rb").read()
