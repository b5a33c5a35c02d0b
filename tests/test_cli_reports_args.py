"""plink2-hip --missing / --freq / --geno-counts on the CPU: every accepted form gets past the argument checks (exit 0, or 16 "no usable HIP
device" where there is no GPU), every modifier that is not built is refused by name (exit 63), what the reference rejects is rejected with its
message and its exit code, and the data the reports do not cover is refused from the tables, before any device is touched."""
import os

import numpy as np
import pytest

import ldtools as T
import reports_tools as RT


@pytest.fixture(scope="module")
def cli():
    import __graft_entry__ as ge
    return ge.load_package().build_cli()


def _files(d, chroms=None, m=40, n=60, pheno=None):
    raw = T.synth_raw_codes(m, n, seed=3, missing_rate=0.02)
    T.write_pgen_fixed(str(d / "d"), raw, chroms or ["1"] * m, np.arange(m) * 10 + 1)
    T.write_bed(str(d / "d"), raw, chroms or ["1"] * m, np.arange(m) * 10 + 1)
    if pheno is not None:
        with open(str(d / "d.psam"), "w") as f:
            f.write("#IID\tSEX\tBMI\n")
            for s in range(n):
                f.write("s%d\t2\t%s\n" % (s, pheno(s)))
        lines = [l.split() for l in open(str(d / "d.fam")).read().splitlines()]
        open(str(d / "d.fam"), "w").write("".join(" ".join(t[:5] + [pheno(s) if pheno(s) != "NA" else "-9"]) + "\n" for s, t in enumerate(lines)))


def past_the_argument_checks(r):
    # 0 where there is a GPU; 16 = "no usable HIP device" where there is none: past every argument and table check either way
    assert r.returncode in (0, 16), r.stdout
    assert (r.returncode == 0) or ("no usable HIP device" in r.stdout), r.stdout
    assert "not supported" not in r.stdout and "Unrecognized" not in r.stdout and "Invalid" not in r.stdout, r.stdout


PRUNE = ["--indep-pairwise", "50", "5", "0.2"]
ACCEPTED = [
    ["--missing"], ["--missing", "zs"], ["--missing", "sample-only"], ["--missing", "variant-only"], ["--missing", "zs", "variant-only"], ["--missing", "sample-only", "zs"],
    ["--freq"], ["--freq", "zs"], ["--freq", "counts"], ["--freq", "counts", "zs"], ["--freq", "zs", "counts"],
    ["--geno-counts"], ["--geno-counts", "zs"],
    ["--missing", "--freq", "--geno-counts"], ["--freq", "counts", "--missing", "variant-only", "--geno-counts", "zs"],
]


@pytest.mark.parametrize("args", ACCEPTED, ids=lambda a: " ".join(a))
def test_accepted_forms(cli, tmp_path, args):
    _files(tmp_path)
    for src in ("--pfile", "--bfile"):
        past_the_argument_checks(RT.run_cli(cli, [src, "d"] + args + PRUNE + ["--out", "o"], tmp_path))     # beside a command
        past_the_argument_checks(RT.run_cli(cli, [src, "d"] + args + ["--out", "o"], tmp_path))             # reports alone: a valid run
    # the host's pass needs no device at all: a run of reports alone ends with exit 0 on any machine
    r = RT.run_cli(cli, ["--pfile", "d"] + args + ["--debug-host-filter", "--out", "o"], tmp_path)
    assert r.returncode == 0 and "written to o." in r.stdout, r.stdout


def test_no_command_and_no_report_is_still_an_error(cli, tmp_path):
    _files(tmp_path)
    r = RT.run_cli(cli, ["--pfile", "d", "--out", "o"], tmp_path)
    assert r.returncode == 8 and "no command given" in r.stdout, r.stdout
    r = RT.run_cli(cli, ["--pfile", "d", "--glm", "--out", "o"], tmp_path)
    assert r.returncode == 8 and "Unrecognized flag" in r.stdout, r.stdout


REFUSED_MODIFIERS = [
    (["--missing", "scols=fid,nmiss"], "scols=fid,nmiss"), (["--missing", "vcols=chrom,nmiss"], "vcols=chrom,nmiss"), (["--missing", "zs", "vcols=+pos"], "vcols=+pos"),
    (["--freq", "cols=+pos"], "cols=+pos"), (["--freq", "counts", "cols=chrom,ref"], "cols=chrom,ref"), (["--freq", "bins-only", "refbins=0.1,0.5"], "bins-only"),
    (["--freq", "refbins=0.1,0.5"], "refbins=0.1,0.5"), (["--freq", "refbins-file=b.txt"], "refbins-file=b.txt"), (["--freq", "alt1bins=0.1"], "alt1bins=0.1"),
    (["--freq", "alt1bins-file=b.txt"], "alt1bins-file=b.txt"), (["--geno-counts", "cols=chrom,homref"], "cols=chrom,homref"), (["--geno-counts", "zs", "cols=+pos"], "cols=+pos"),
    (["--freq", "case-control"], "case-control"),   # (retired: the reference says so and then writes the plain report)
    (["--freq", "--nonfounders"], "--nonfounders"), (["--missing", "--nonfounders"], "--nonfounders"),
]


@pytest.mark.parametrize("args,named", REFUSED_MODIFIERS, ids=lambda a: " ".join(a) if isinstance(a, list) else a)
def test_other_modifiers_are_refused_by_name(cli, tmp_path, args, named):
    _files(tmp_path)
    for tail in (PRUNE, []):
        r = RT.run_cli(cli, ["--pfile", "d"] + args + tail + ["--out", "o"], tmp_path)
        assert r.returncode == 63 and named in r.stdout and "not supported" in r.stdout, (r.returncode, r.stdout)
    assert not any(f.startswith("o.") and not f.endswith(".log") for f in os.listdir(str(tmp_path)))


REFERENCE_REJECTS = [
    (["--missing", "sample-only", "variant-only"], "Error: --missing 'sample-only' and 'variant-only' cannot be used together."),
    (["--missing", "variant-only", "zs", "sample-only"], "Error: --missing 'sample-only' and 'variant-only' cannot be used together."),
    (["--missing", "samples"], "Error: Invalid --missing argument 'samples'."),
    (["--freq", "count"], "Error: Invalid --freq argument 'count'."),
    (["--geno-counts", "counts"], "Error: Invalid --geno-counts argument 'counts'."),
    (["--geno-counts", "zs", "zs", "zs"], "Error: --geno-counts accepts at most 2 arguments."),
    (["--missing", "zs", "zs", "zs", "zs", "zs"], "Error: --missing accepts at most 4 arguments."),
    (["--freq", "zs", "zs", "zs", "zs", "zs", "zs"], "Error: --freq accepts at most 5 arguments."),
]


@pytest.mark.parametrize("args,message", REFERENCE_REJECTS, ids=lambda a: " ".join(a) if isinstance(a, list) else None)
def test_what_the_reference_rejects_is_rejected_alike(cli, tmp_path, args, message):
    _files(tmp_path)
    r = RT.run_cli(cli, ["--pfile", "d"] + args + ["--out", "o"], tmp_path)
    assert r.returncode == 8 and message in r.stdout.replace("\n", " "), (r.returncode, r.stdout)
    if T.have_ref():
        ref = T.run_ref(["--pfile", "d"] + args + ["--out", "r"], str(tmp_path))
        assert ref.returncode == r.returncode and message in ref.stdout.replace("\n", " "), (ref.returncode, ref.stdout[-600:])


@pytest.mark.parametrize("chrom,flag", [("X", "--missing"), ("Y", "--freq"), ("MT", "--geno-counts"), ("chrX", "--freq")])
def test_sex_chromosomes_are_refused_unless_filtered_away(cli, tmp_path, chrom, flag):
    _files(tmp_path, chroms=["1"] * 30 + [chrom] * 10)
    for tail in (PRUNE, ["--debug-host-filter"], []):
        r = RT.run_cli(cli, ["--pfile", "d", flag] + tail + ["--out", "o"], tmp_path)
        assert r.returncode == 63 and ("'%s'" % chrom) in r.stdout and flag in r.stdout and "not supported" in r.stdout, (r.returncode, r.stdout)
    for keep in (["--chr", "1"], ["--autosome"], ["--not-chr", chrom]):
        past_the_argument_checks(RT.run_cli(cli, ["--bfile", "d", flag] + keep + PRUNE + ["--out", "o"], tmp_path))
        r = RT.run_cli(cli, ["--pfile", "d", flag] + keep + ["--debug-host-filter", "--out", "o"], tmp_path)
        assert r.returncode == 0, r.stdout


def test_a_phenotype_is_refused_for_smiss_only(cli, tmp_path):
    _files(tmp_path, pheno=lambda s: "NA" if s % 2 else "%.1f" % (20 + s))
    for src in ("--pfile", "--bfile"):
        for args in (["--missing"], ["--missing", "sample-only"], ["--freq", "--missing", "zs"]):
            r = RT.run_cli(cli, [src, "d"] + args + ["--out", "o"], tmp_path)
            assert r.returncode == 63 and "phenotype" in r.stdout and ".smiss" in r.stdout, (r.returncode, r.stdout)
        for args in (["--missing", "variant-only"], ["--freq"], ["--geno-counts"]):
            r = RT.run_cli(cli, [src, "d"] + args + ["--debug-host-filter", "--out", "o"], tmp_path)
            assert r.returncode == 0, r.stdout
    # a .fam whose sixth column holds no value has no phenotype (the reference: "No phenotype data present"); a named .psam column is kept even so
    _files(tmp_path, pheno=lambda s: "NA")
    r = RT.run_cli(cli, ["--pfile", "d", "--missing", "--out", "o"], tmp_path)
    assert r.returncode == 63 and "'BMI'" in r.stdout, (r.returncode, r.stdout)
    r = RT.run_cli(cli, ["--bfile", "d", "--missing", "--debug-host-filter", "--out", "o"], tmp_path)
    assert r.returncode == 0, r.stdout
    if T.have_ref():
        ref = T.run_ref(["--bfile", "d", "--missing", "--out", "r"], str(tmp_path))
        assert ref.returncode == 0 and open(str(tmp_path / "r.smiss"), "rb").read() == open(str(tmp_path / "o.smiss"), "rb").read()


def test_dosage_tracks_are_refused(cli, tmp_path):
    if not T.have_ref():
        pytest.skip("needs the reference binary (it writes the fileset)")
    cp = T.run_ref(["--dummy", "60", "40", "dosage-freq=0.4", "--seed", "3", "--make-pgen", "--out", "dos"], str(tmp_path))
    assert cp.returncode == 0, cp.stdout[-800:]
    for args in (["--freq"], ["--missing", "variant-only"], ["--geno-counts"], ["--freq"] + PRUNE, ["--freq", "--debug-host-filter"]):
        r = RT.run_cli(cli, ["--pfile", "dos"] + args + ["--out", "o"], tmp_path)
        assert r.returncode == 63 and "dosage" in r.stdout and "dos.pgen" in r.stdout, (r.returncode, r.stdout)
