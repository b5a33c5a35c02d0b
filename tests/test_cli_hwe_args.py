"""plink2-hip --hwe / --hardy on the CPU: every accepted form gets past the argument checks, what the reference rejects is rejected with its
message and its exit code (the reference binary's own output is the yardstick where it is built), and what plink2-hip does not build -- chrX,
variants with several ALT alleles, --hardy's other modifiers -- is refused by name with exit 63, before any device is touched."""
import os

import numpy as np
import pytest

import hwe_tools as H
import ldtools as T


@pytest.fixture(scope="module")
def cli():
    import __graft_entry__ as ge
    return ge.load_package().build_cli()


def _files(d, chroms=None, m=40, n=60):
    raw = T.synth_raw_codes(m, n, seed=3, missing_rate=0.02)
    T.write_pgen_fixed(str(d / "d"), raw, chroms or ["1"] * m, np.arange(m) * 10 + 1)
    T.write_bed(str(d / "d"), raw, chroms or ["1"] * m, np.arange(m) * 10 + 1)


def past_the_argument_checks(r):
    # 0 where there is a GPU; 16 = "no usable HIP device" where there is none: past every argument and table check either way
    assert r.returncode in (0, 16), r.stdout
    assert (r.returncode == 0) or ("no usable HIP device" in r.stdout), r.stdout
    assert "not supported" not in r.stdout and "Unrecognized" not in r.stdout and "Invalid" not in r.stdout, r.stdout


PRUNE = ["--indep-pairwise", "50", "5", "0.2"]
ACCEPTED = [["--hwe", "1e-6", "0.001"], ["--hwe", "1e-3", "0"], ["--hwe", "0.001", "0", "midp"], ["--hwe", "midp", "1e-3", "0", "keep-fewhet"],
            ["--hwe", "keep-fewhet", "1e-10"], ["--hwe", "1e-400", "0"], ["--hwe", "0", "0"], ["--hwe", "1", "0.01"],
            ["--hardy"], ["--hardy", "zs"], ["--hardy", "midp"], ["--hardy", "midp", "zs"], ["--hwe", "1e-3", "0", "--hardy", "midp"]]


@pytest.mark.parametrize("args", ACCEPTED, ids=lambda a: " ".join(a))
def test_accepted_forms(cli, tmp_path, args):
    _files(tmp_path)
    for src in ("--pfile", "--bfile"):
        past_the_argument_checks(H.run_cli(cli, [src, "d"] + args + PRUNE + ["--out", "o"], tmp_path))
        past_the_argument_checks(H.run_cli(cli, [src, "d"] + args + ["--geno", "0.1", "--maf", "0.05"] + PRUNE + ["--out", "o"], tmp_path))
    # the host's pass needs no device: --hardy alone, and --hwe in front of --het, end with exit 0 on any machine
    tail = [] if "--hardy" in args else ["--het", "--bad-freqs"]
    r = H.run_cli(cli, ["--pfile", "d"] + args + tail + ["--debug-host-filter", "--out", "o"], tmp_path)
    assert r.returncode == 0, r.stdout
    if "--hardy" in args:
        ext = ".hardy.zst" if "zs" in args else ".hardy"
        assert ("written to o%s ." % ext) in r.stdout.replace("\n", " ") and os.path.getsize(str(tmp_path / ("o" + ext))) > 20, r.stdout
    else:
        assert "removed due to Hardy-Weinberg exact test (founders only)." in r.stdout.replace("\n", " "), r.stdout


def test_hardy_is_a_command_and_hwe_is_not(cli, tmp_path):
    _files(tmp_path)
    r = H.run_cli(cli, ["--pfile", "d", "--hwe", "1e-3", "0", "--out", "o"], tmp_path)
    assert r.returncode == 8 and "no command given" in r.stdout
    r = H.run_cli(cli, ["--pfile", "d", "--hardy", "--debug-host-filter", "--out", "o"], tmp_path)
    assert r.returncode == 0 and os.path.exists(str(tmp_path / "o.hardy")), r.stdout


REJECTED = [
    (["--hwe"], "Error: Missing --hwe argument."),
    (["--hwe", "1e-3", "0", "midp", "keep-fewhet", "0"], "Error: --hwe accepts at most 4 arguments."),
    (["--hwe", "midp"], "Error: No --hwe p-value threshold specified."),
    (["--hwe", "abc"], "Error: Invalid --hwe argument sequence."),
    (["--hwe", "1e-3", "0", "0"], "Error: Invalid --hwe argument sequence."),
    (["--hwe", "1e-3", "x"], "Error: Invalid --hwe argument sequence."),
    (["--hwe", "-0.1"], "Error: Invalid --hwe argument sequence."),
    (["--hwe", "1.5"], "Error: Invalid --hwe threshold '1.5' (must be in [0, 1])."),
    (["--hwe", "1"], "Error: --hwe threshold cannot be 1 unless a nonzero sample size term is"),
    (["--hwe", "1", "0"], "Error: --hwe threshold cannot be 1 unless a nonzero sample size term is"),
    (["--hwe", "0.51", "midp"], "Error: --hwe threshold must be smaller than 0.5 when using mid-p adjustment."),
    (["--hwe", "0.7", "0", "midp"], "Error: --hwe threshold must be smaller than 0.5 when using mid-p adjustment."),
    (["--hwe", "1e-3", "-0.5"], "Error: Invalid --hwe sample size term '-0.5' (must be nonnegative)."),
    (["--hardy", "bogus"], "Error: Invalid --hardy argument 'bogus'."),
    (["--hardy", "zs", "midp", "zs", "midp", "zs", "midp"], "Error: --hardy accepts at most 5 arguments."),
]


@pytest.mark.parametrize("args,message", REJECTED, ids=[" ".join(a) for a, _ in REJECTED])
def test_what_the_reference_rejects(cli, tmp_path, args, message):
    _files(tmp_path)
    tail = [] if args[0] == "--hardy" else ["--hardy"]
    r = H.run_cli(cli, ["--pfile", "d"] + args + tail + ["--out", "o"], tmp_path)
    errors = [l for l in r.stdout.split("\n") if l.startswith("Error:")]
    assert r.returncode == 8 and errors == [message] and not os.path.exists(str(tmp_path / "o.hardy")), (r.returncode, r.stdout)
    if T.have_ref():
        ref = T.run_ref(["--pfile", "d"] + args + tail + ["--out", "r"], str(tmp_path))
        assert ref.returncode != 0
        ref_errors = [l for l in ref.stdout.split("\n") if l.startswith("Error:")]
        assert ref_errors == errors, (ref_errors, errors)
        # (the reference's exit status for a malformed command line, whatever it is, is one status: ours for the same class is 8)
        other = T.run_ref(["--pfile", "d", "--hardy", "bogus", "--out", "r"], str(tmp_path))
        assert ref.returncode == other.returncode, (ref.returncode, other.returncode)


@pytest.mark.parametrize("mod", ["cols=chrom,p", "cols=+pos", "log10", "redundant"])
def test_other_hardy_modifiers_are_refused_by_name(cli, tmp_path, mod):
    _files(tmp_path)
    r = H.run_cli(cli, ["--pfile", "d", "--hardy", mod, "--out", "o"], tmp_path)
    assert r.returncode == 63 and ("'%s' modifier of --hardy" % mod) in r.stdout and not os.path.exists(str(tmp_path / "o.hardy")), (r.returncode, r.stdout)


@pytest.mark.parametrize("args", [["--hardy"], ["--hwe", "1e-3", "0"] + PRUNE, ["--hardy", "--debug-host-filter"]], ids=lambda a: " ".join(a))
def test_chrx_is_refused_by_name(cli, tmp_path, args):
    _files(tmp_path, chroms=["1"] * 30 + ["X"] * 10)
    r = H.run_cli(cli, ["--pfile", "d"] + args + ["--out", "o"], tmp_path)
    assert r.returncode == 63 and "chrX" in r.stdout and "'snp30'" in r.stdout and not os.path.exists(str(tmp_path / "o.hardy")), (r.returncode, r.stdout)
    # filtered out, it is no obstacle
    r = H.run_cli(cli, ["--pfile", "d", "--autosome", "--hardy", "--debug-host-filter", "--out", "o"], tmp_path)
    assert r.returncode == 0 and len(open(str(tmp_path / "o.hardy")).read().split("\n")) == 32, r.stdout


def test_chry_and_mt_are_neither_tested_nor_listed(cli, tmp_path):
    _files(tmp_path, chroms=["1"] * 30 + ["Y"] * 4 + ["MT"] * 6)
    r = H.run_cli(cli, ["--pfile", "d", "--hardy", "--out", "o"], tmp_path)   # (the host's pass takes such a run on any machine)
    assert r.returncode == 0 and "--hardy: Skipping 10 haploid variants." in r.stdout, r.stdout
    got = open(str(tmp_path / "o.hardy"), "rb").read()
    assert len(got.split(b"\n")) == 32
    if T.have_ref():
        ref = T.run_ref(["--pfile", "d", "--hardy", "--out", "r"], str(tmp_path))
        assert ref.returncode == 0 and "--hardy: Skipping 10 haploid variants." in ref.stdout
        assert open(str(tmp_path / "r.hardy"), "rb").read() == got


def test_multiallelic_variants_are_refused_by_name(cli, tmp_path):
    if not T.have_ref():
        pytest.skip("needs the reference binary (it imports the fileset)")
    import het_tools
    het_tools.write_multiallelic_fileset(tmp_path)
    for args in (["--hardy"], ["--hwe", "1e-3", "0", "--het"], ["--hwe", "1e-3", "0"] + PRUNE):
        r = H.run_cli(cli, ["--pfile", "v"] + args + ["--out", "o"], tmp_path)
        assert r.returncode == 63 and "multiallelic variant ('" in r.stdout and "--max-alleles 2 leaves them out" in r.stdout, (r.returncode, r.stdout)
    r = H.run_cli(cli, ["--pfile", "v", "--max-alleles", "2", "--hardy", "--debug-host-filter", "--out", "o"], tmp_path)
    assert r.returncode == 0, r.stdout
    ref = T.run_ref(["--pfile", "v", "--max-alleles", "2", "--hardy", "--out", "r"], str(tmp_path))
    assert ref.returncode == 0 and open(str(tmp_path / "r.hardy"), "rb").read() == open(str(tmp_path / "o.hardy"), "rb").read()
