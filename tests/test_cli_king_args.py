"""plink2-hip --make-king-table / --king-table-filter on the CPU: every accepted form gets past the argument checks and --dry-run prints the
parsed columns, the filter and the decision between the device's path and the host's pass; what the reference rejects is rejected with its
message and its exit code (the reference's own output is the yardstick where the binary is there); what is not built is refused by name
(exit 63)."""
import os

import numpy as np
import pytest

import het_tools as H
import ldtools as T


@pytest.fixture(scope="module")
def cli():
    import __graft_entry__ as ge
    return ge.load_package().build_cli()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("king_args")
    m, n = 40, 60
    raw = T.synth_raw_codes(m, n, seed=3, missing_rate=0.02)
    T.write_pgen_fixed(str(d / "d"), raw, ["1"] * m, np.arange(m) * 10 + 1)
    T.write_bed(str(d / "d"), raw, ["1"] * m, np.arange(m) * 10 + 1)
    T.write_pgen_fixed(str(d / "x"), raw, ["1"] * 30 + ["X"] * 10, np.arange(m) * 10 + 1)
    T.write_pgen_fixed(str(d / "nf"), raw, ["1"] * m, np.arange(m) * 10 + 1)
    with open(str(d / "nf.psam"), "w") as f:
        f.write("#IID\tPAT\tMAT\tSEX\n")
        for s in range(n):
            f.write("s%d\t%s\t%s\t2\n" % (s, "p1" if s == 4 else "0", "p2" if s == 4 else "0"))
    return d


PRUNE = ["--indep-pairwise", "50", "5", "0.2"]
DEFAULT = 0x4ed   # maybefid, id, maybesid, nsnp, hethet, ibs0, kinship
ACCEPTED = [
    (["--make-king-table"], DEFAULT, "filter none"),
    (["--make-king-table", "zs"], DEFAULT, ", zs, filter none"),
    (["--make-king-table", "counts"], DEFAULT, ", counts, filter none"),
    (["--make-king-table", "counts", "zs", "cols=id,nsnp,hethet,ibs0,ibs1,ibs,kinship"], 0x7e4, ", counts, zs, filter none"),
    (["--make-king-table", "cols=+ibs1,-hethet"], (DEFAULT | 0x100) & ~0x40, "filter none"),
    (["--make-king-table", "cols=fid,id,sid,kinship"], 0x416, "filter none"),
    (["--make-king-table", "cols=nsnp,kinship"], 0x420, "filter none"),
    (["--make-king-table", "--king-table-filter", "0.0884"], DEFAULT, "filter 0.0884"),
    (["--king-table-filter", "-0.25", "--make-king-table", "counts"], DEFAULT, ", counts, filter -0.25"),
    (["--make-king-table", "--king-table-filter", "0.5"], DEFAULT, "filter 0.5"),
]


@pytest.mark.parametrize("args,cols,rest", ACCEPTED, ids=lambda a: " ".join(a) if isinstance(a, list) else None)
def test_accepted_forms_and_the_dry_run_decision(cli, files, args, cols, rest):
    for src in ("--pfile", "--bfile"):
        r = H.run_cli(cli, [src, "d"] + args + ["--dry-run", "--out", "o"], files)
        assert r.returncode == 0, r.stdout
        assert ("dry-run: --make-king-table: cols 0x%x" % cols) in r.stdout and rest in r.stdout and "from the resident image" in r.stdout, r.stdout
        assert not os.path.exists(str(files / "o.kin0"))
    r = H.run_cli(cli, ["--pfile", "d"] + args + PRUNE + ["--dry-run", "--out", "o"], files)      # beside the prune
    assert r.returncode == 0 and "from the resident image" in r.stdout, r.stdout
    r = H.run_cli(cli, ["--pfile", "d"] + args + ["--geno", "0.1", "--maf", "0.05", "--mind", "0.5", "--het", "small-sample", "--dry-run", "--out", "o"], files)
    assert r.returncode == 0 and "from the resident image" in r.stdout, r.stdout


@pytest.mark.parametrize("src,extra,why", (
    ("x", [], "chrX / chrY / MT variants"),
    ("nf", [], "non-founders among the kept samples"),
    ("d", ["--gpus", "2"], "more than one GPU"),
    ("d", ["--debug-host-filter"], "--debug-host-filter"),
))
def test_dry_run_names_the_fall_back(cli, files, src, extra, why):
    r = H.run_cli(cli, ["--pfile", src, "--make-king-table"] + extra + ["--dry-run", "--out", "fb"], files)
    assert r.returncode == 0 and "dry-run: --make-king-table:" in r.stdout and ("host pass: " + why) in r.stdout, r.stdout
    assert not os.path.exists(str(files / "fb.kin0"))


def test_the_host_pass_needs_no_device(cli, files):
    r = H.run_cli(cli, ["--pfile", "d", "--make-king-table", "--debug-host-filter", "--out", "h"], files)
    assert r.returncode == 0 and "Results written to h.kin0 ." in r.stdout and os.path.getsize(str(files / "h.kin0")) > 1000, r.stdout
    r = H.run_cli(cli, ["--pfile", "d", "--out", "o"], files)
    assert r.returncode == 8 and "no command given" in r.stdout


def errors(out):
    text = out[out.index("Error:"):].split("End time")[0]
    return text.split("For more info")[0].rstrip()


REJECTED = [
    (["--make-king-table", "cols=fid,nsnp"], "'maybesid', and 'sid' require 'id'"),
    (["--make-king-table", "cols=maybesid,kinship"], "'maybesid', and 'sid' require 'id'"),
    (["--king-table-filter", "0.1", "--make-king-table", "cols=nsnp,kinship"], "--king-table-filter requires --make-king-table cols= to include the 'id'"),
    (["--make-king-table", "cols=id,nsnp", "cols=id,kinship"], "Error: Multiple --make-king-table cols= modifiers."),
    (["--make-king-table", "--king-table-filter", "0.51"], "Error: Invalid --king-table-filter argument '0.51'."),
    (["--make-king-table", "--king-table-filter", "abc"], "Error: Invalid --king-table-filter argument 'abc'."),
    (["--make-king-table", "--king-table-filter"], "Error: Missing --king-table-filter argument."),
    (["--make-king-table", "--king-table-filter", "0.1", "0.2"], "Error: --king-table-filter only accepts 1 argument."),
    (["--make-king-table", "no-idheader"], "'no-idheader' modifier retired"),
    (["--make-king-table", "bogus"], "Error: Invalid --make-king-table argument 'bogus'."),
    (["--make-king-table", "Counts"], "Error: Invalid --make-king-table argument 'Counts'."),
    (["--make-king-table", "zs", "counts", "zs", "counts", "zs"], "Error: --make-king-table accepts at most 4 arguments."),
    (["--make-king-table", "cols=id,bogus"], "Error: Unrecognized ID 'bogus' in --make-king-table column set descriptor."),
]


@pytest.mark.parametrize("args,message", REJECTED, ids=lambda a: " ".join(a) if isinstance(a, list) else None)
def test_what_the_reference_rejects(cli, files, args, message):
    r = H.run_cli(cli, ["--pfile", "d"] + args + ["--out", "rej"], files)
    assert r.returncode != 0 and message in r.stdout and not os.path.exists(str(files / "rej.kin0")), (r.returncode, r.stdout)
    if T.have_ref():
        ref = T.run_ref(["--pfile", "d"] + args + ["--out", "rejr"], str(files))
        assert ref.returncode == r.returncode, (ref.returncode, r.returncode, ref.stdout[-400:])
        assert errors(ref.stdout) == errors(r.stdout), (ref.stdout[-500:], r.stdout[-500:])


@pytest.mark.parametrize("args,name", (
    (["--make-king", "square"], "--make-king "),
    (["--king-cutoff", "0.177"], "--king-cutoff "),
    (["--make-king-table", "--king-cutoff", "0.177"], "--king-cutoff "),
    (["--king-cutoff-table", "x.kin0", "0.177"], "--king-cutoff-table "),
    (["--make-king-table", "--king-table-subset", "x.kin0"], "--king-table-subset "),
    (["--make-king-table", "--king-table-require", "x.txt"], "--king-table-require "),
    (["--make-king-table", "--king-table-require-xor", "x.txt"], "--king-table-require-xor "),
    (["--make-king-table", "rel-check"], "'rel-check' modifier of --make-king-table"),
    (["--make-king-table", "concordance-check"], "'concordance-check' modifier of --make-king-table"),
    (["--make-king-table", "--parallel", "1", "2"], "--parallel with --make-king-table"),
), ids=lambda a: " ".join(a) if isinstance(a, list) else None)
def test_refused_by_name(cli, files, args, name):
    r = H.run_cli(cli, ["--pfile", "d"] + args + ["--out", "ref63"], files)
    assert r.returncode == 63 and name in r.stdout and "not supported by plink2-hip" in r.stdout, (r.returncode, r.stdout)
    assert not os.path.exists(str(files / "ref63.kin0"))


def test_filter_without_the_table(cli, files):
    r = H.run_cli(cli, ["--pfile", "d", "--king-table-filter", "0.1"] + PRUNE + ["--out", "o"], files)
    assert r.returncode == 8 and "--king-table-filter must be used with --make-king-table" in r.stdout, r.stdout


def test_beside_the_r2_commands_the_host_pass_runs_first(cli, files):
    """--r2-unphased plans its engine before the load: the table beside it is served by the host's pass, whose file is complete before any
    device is asked for (exit 16 where there is none)"""
    r = H.run_cli(cli, ["--pfile", "d", "--make-king-table", "--r2-unphased", "square", "--out", "r2"], files)
    assert r.returncode in (0, 16) and ((r.returncode == 0) or ("no usable HIP device" in r.stdout)), r.stdout
    assert "Results written to r2.kin0 ." in r.stdout, r.stdout
    alone = H.run_cli(cli, ["--pfile", "d", "--make-king-table", "--debug-host-filter", "--out", "r2a"], files)
    assert alone.returncode == 0 and open(str(files / "r2.kin0"), "rb").read() == open(str(files / "r2a.kin0"), "rb").read()
