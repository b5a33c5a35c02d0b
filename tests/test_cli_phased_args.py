"""plink2-hip --r2-phased / --r-phased: what the front-end takes and what it refuses (no GPU needed: every refusal comes before a device
is touched; an accepted form gets as far as the device, which a CPU-only machine does not have)."""
import subprocess

import numpy as np
import pytest

import ldtools as T


@pytest.fixture(scope="module")
def cli():
    import __graft_entry__ as ge
    return ge.load_package().build_cli()


def _run(cli, cwd, args):
    return subprocess.run([cli] + args, cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)


def _files(tmp_path, chroms=None, alt=None):
    m, n = 40, 24
    raw = T.synth_raw_codes(m, n, seed=3, missing_rate=0.02)
    T.write_pgen_fixed(str(tmp_path / "d"), raw, chroms or ["1"] * m, np.arange(m) * 10 + 1)
    T.write_bed(str(tmp_path / "d"), raw, chroms or ["1"] * m, np.arange(m) * 10 + 1)
    if alt:
        lines = open(str(tmp_path / "d.pvar")).read().split("\n")
        lines[3] = lines[3][:-1] + alt
        open(str(tmp_path / "d.pvar"), "w").write("\n".join(lines))


ACCEPTED = [
    ["--r2-phased"],
    ["--r-phased"],
    ["--r2-phased", "cols=+d,+dprime,+dprimeabs,+maj,+freq", "--ld-window-kb", "5", "--ld-window-r2", "0"],
    ["--r-phased", "ref-based", "zs", "--ld-window", "10"],
    ["--r2-phased", "allow-ambiguous-allele", "--ld-window-cm", "1", "--ld-window-r2", "0.5"],
    ["--r2-phased", "--ld-snp", "snp3"],
    ["--r2-phased", "--ld-snps", "snp3-snp6,snp9"],
]


@pytest.mark.parametrize("args", ACCEPTED)
@pytest.mark.parametrize("src", ["--pfile", "--bfile"])
def test_accepted_forms_reach_the_device(cli, tmp_path, src, args):
    _files(tmp_path)
    r = _run(cli, tmp_path, [src, "d"] + args + ["--out", "o"])
    # 0 where there is a GPU; 16 = "no usable HIP device" where there is none: past every argument check either way
    assert r.returncode in (0, 16), r.stdout
    assert (r.returncode == 0) or ("no usable HIP device" in r.stdout), r.stdout
    assert "not supported" not in r.stdout and "Unrecognized" not in r.stdout


REFUSED = [
    (["--r2-phased", "square"], "matrix shapes"),
    (["--r2-phased", "triangle", "bin4"], "matrix shapes"),
    (["--r-phased", "bin"], "matrix shapes"),
    (["--r2-phased", "inter-chr"], "inter-chr is not supported"),
    (["--r2-phased", "--parallel", "1", "2"], "--parallel with --r2-phased / --r-phased is not supported"),
    (["--r-phased", "--gpus", "2"], "--gpus above 1 with --r2-phased / --r-phased is not supported"),
]


@pytest.mark.parametrize("args,needle", REFUSED)
def test_refused_forms_exit_63_and_say_why(cli, tmp_path, args, needle):
    _files(tmp_path)
    r = _run(cli, tmp_path, ["--pfile", "d"] + args + ["--out", "o"])
    assert r.returncode == 63 and needle in r.stdout.replace("\n", " "), (r.returncode, r.stdout)


def test_refused_data_exit_63_and_say_why(cli, tmp_path):
    # variants on a sex chromosome or MT -- unless filtered away
    for chrom, flag in (("X", "--r2-phased"), ("Y", "--r-phased"), ("MT", "--r2-phased")):
        _files(tmp_path, chroms=["1"] * 30 + [chrom] * 10)
        r = _run(cli, tmp_path, ["--pfile", "d", flag, "--out", "o"])
        assert r.returncode == 63 and "chrX / chrY / MT variants is not supported" in r.stdout, (chrom, r.returncode, r.stdout)
        r = _run(cli, tmp_path, ["--pfile", "d", flag, "--chr", "1", "--out", "o"])
        assert r.returncode in (0, 16), (chrom, r.stdout)
    # a variant with two ALT alleles
    _files(tmp_path, alt="C,G")
    r = _run(cli, tmp_path, ["--pfile", "d", "--r2-phased", "--out", "o"])
    assert r.returncode == 63 and "multiallelic variants is not supported" in r.stdout, (r.returncode, r.stdout)


def test_dosage_files_are_refused(cli, tmp_path):
    if not T.have_ref():
        pytest.skip("oracle/_ref/plink2 not built (it writes the dosage file)")
    cp = T.run_ref(["--dummy", "20", "30", "dosage-freq=0.2", "--seed", "1", "--make-pgen", "--out", "dos"], str(tmp_path))
    assert cp.returncode == 0, cp.stdout
    r = _run(cli, tmp_path, ["--pfile", "dos", "--r2-phased", "--out", "o"])
    # (the input stage refuses such files for every command: the statistic would be computed from hardcalls)
    assert r.returncode == 63 and "dosage" in r.stdout, (r.returncode, r.stdout)


def test_phased_and_unphased_are_mutually_exclusive(cli, tmp_path):
    _files(tmp_path)
    for args in (["--r2-phased", "--r2-unphased"], ["--r2-unphased", "--r-phased"], ["--r2-phased", "--r-phased"]):
        r = _run(cli, tmp_path, ["--pfile", "d"] + args + ["--out", "o"])
        assert r.returncode == 8 and "mutually" in r.stdout, (args, r.returncode, r.stdout)
    # the unphased flags still point D / D' requests at the phased ones
    r = _run(cli, tmp_path, ["--pfile", "d", "--r2-unphased", "cols=+d", "--out", "o"])
    assert r.returncode == 8 and "Use --r2-phased" in r.stdout
