"""plink2-hip --mind on the CPU: the flag's parsing (the reference's three error messages, exit 8), what is refused (exit 63), and -- through
--dry-run, which takes the host pass and needs no GPU -- the decision itself: the --mind log lines and <out>.mindrem.id byte for byte against the
reference binary's, on .bed, fixed-width .pgen and the reference-written variable-width .pgen."""
import os
import subprocess

import numpy as np
import pytest

import ldtools as T
import mind_tools as MT


@pytest.fixture(scope="module")
def cli():
    import __graft_entry__ as ge
    return ge.load_package().build_cli()


def _run(cli, cwd, args):
    return subprocess.run([cli] + args, cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)


def _files(tmp_path, chroms=None):
    m, n = 40, 60
    raw = T.synth_raw_codes(m, n, seed=3, missing_rate=0.02)
    T.write_pgen_fixed(str(tmp_path / "d"), raw, chroms or ["1"] * m, np.arange(m) * 10 + 1)
    T.write_bed(str(tmp_path / "d"), raw, chroms or ["1"] * m, np.arange(m) * 10 + 1)


PRUNE = ["--indep-pairwise", "50", "5", "0.2"]
PARSE_ERRORS = [
    (["--mind", "0.1", "0.2"], "Error: Invalid --mind argument sequence."),
    (["--mind", "abc"], "Error: Invalid --mind argument 'abc'."),
    (["--mind", "0.1x"], "Error: Invalid --mind argument '0.1x'."),
    (["--mind", "1.5"], "Error: Invalid --mind argument '1.5' (must be in [0, 1])."),
    (["--mind", "-0.5"], "Error: Invalid --mind argument '-0.5' (must be in [0, 1])."),
]


@pytest.mark.parametrize("args,message", PARSE_ERRORS)
def test_parse_errors_are_the_references(cli, tmp_path, args, message):
    _files(tmp_path)
    r = _run(cli, tmp_path, ["--pfile", "d"] + args + PRUNE + ["--dry-run", "--out", "o"])
    assert r.returncode == 8 and message in r.stdout, (r.returncode, r.stdout)
    if T.have_ref():
        ref = T.run_ref(["--pfile", "d"] + args + PRUNE + ["--out", "r"], str(tmp_path))
        assert ref.returncode == 8 and message in ref.stdout.replace("\n", " "), (ref.returncode, ref.stdout[-600:])


@pytest.mark.parametrize("modifier", ["dosage", "hh-missing"])
def test_modifiers_are_refused_by_name(cli, tmp_path, modifier):
    _files(tmp_path)
    for args in (["--mind", modifier], ["--mind", "0.05", modifier]):
        r = _run(cli, tmp_path, ["--pfile", "d"] + args + PRUNE + ["--dry-run", "--out", "o"])
        assert r.returncode == 63 and ("'%s'" % modifier) in r.stdout and "--mind" in r.stdout, (r.returncode, r.stdout)


def test_chry_is_refused_unless_filtered_away(cli, tmp_path):
    _files(tmp_path, chroms=["1"] * 30 + ["Y"] * 10)
    r = _run(cli, tmp_path, ["--pfile", "d", "--mind", "0.1"] + PRUNE + ["--dry-run", "--out", "o"])
    assert r.returncode == 63 and "chrY" in r.stdout and "--mind" in r.stdout, (r.returncode, r.stdout)
    for src in ("--pfile", "--bfile"):
        r = _run(cli, tmp_path, [src, "d", "--mind", "0.1", "--chr", "1"] + PRUNE + ["--out", "o"])
        # 0 where there is a GPU; 16 = "no usable HIP device" where there is none: past every argument check either way
        assert r.returncode in (0, 16), r.stdout
        assert (r.returncode == 0) or ("no usable HIP device" in r.stdout), r.stdout
        assert "not supported" not in r.stdout and "Unrecognized" not in r.stdout


def test_mind_1_changes_nothing(cli, tmp_path):
    _files(tmp_path)
    base = _run(cli, tmp_path, ["--pfile", "d"] + PRUNE + ["--dry-run", "--out", "a"])
    one = _run(cli, tmp_path, ["--pfile", "d", "--mind", "1"] + PRUNE + ["--dry-run", "--out", "b"])
    assert base.returncode == 0 and one.returncode == 0, (base.stdout, one.stdout)
    plan = [l for l in base.stdout.split("\n") if l.startswith("dry-run:")]
    assert plan and plan == [l for l in one.stdout.split("\n") if l.startswith("dry-run:")]
    assert MT.MIND_LINE not in one.stdout and "--mind" not in "".join(plan) and not os.path.exists(str(tmp_path / "b.mindrem.id"))


def test_default_threshold_is_a_tenth(cli, tmp_path):
    """--mind without a number is --mind 0.1 (a sample with 5 of 40 calls missing goes: the bound is 4)"""
    m, n = 40, 60
    raw = T.synth_raw_codes(m, n, seed=3, missing_rate=0.0).copy()
    raw[:4, 7] = 3
    raw[:5, 9] = 3
    T.write_pgen_fixed(str(tmp_path / "d"), raw, ["1"] * m, np.arange(m) * 10 + 1)
    for args in (["--mind"], ["--mind", "0.1"]):
        r = _run(cli, tmp_path, ["--pfile", "d"] + args + PRUNE + ["--dry-run", "--out", "o"])
        assert r.returncode == 0 and "1 sample removed due to missing genotype data (--mind)." in r.stdout, r.stdout
        assert "ID written to o.mindrem.id ." in r.stdout
        assert open(str(tmp_path / "o.mindrem.id")).read() == "#IID\ns9\n"
        assert "founders=59" in r.stdout


@pytest.fixture(scope="module")
def planted_dir(tmp_path_factory):
    if not T.have_ref():
        pytest.skip("needs the reference binary (oracle/_ref/plink2)")
    d = tmp_path_factory.mktemp("mind_planted")
    raw = MT.planted_codes()
    MT.write_fileset(d, raw)
    return d, raw


@pytest.mark.parametrize("fmt", list(MT.FORMATS))
def test_host_pass_decides_like_the_reference(cli, planted_dir, fmt):
    d, raw = planted_dir
    args = MT.FORMATS[fmt] + ["--mind", "0.1"] + MT.PRUNE
    ref = T.run_ref(args + ["--threads", "2", "--out", fmt], str(d / "ref"))
    got = _run(cli, d / "host", args + ["--dry-run", "--timing", "--out", fmt])
    assert ref.returncode == 0 and got.returncode == 0, (ref.stdout[-800:], got.stdout[-800:])
    # the reference's own list says what the fileset was planted for
    want_ids = ["s%d" % s for s in MT.expected_removed(raw)]
    assert sorted(MT.expected_removed(raw)) == sorted((MT.S_101,) + MT.S_30PCT)
    assert MT.read_mindrem(str(d / "ref" / (fmt + ".mindrem.id"))) == want_ids
    assert "s%d" % MT.S_100 not in want_ids
    want_lines = MT.mind_lines(ref.stdout)
    assert want_lines == ["4 samples removed due to missing genotype data (--mind).", "IDs written to %s.mindrem.id ." % fmt]
    assert MT.mind_lines(got.stdout) == want_lines, got.stdout
    assert open(str(d / "host" / (fmt + ".mindrem.id")), "rb").read() == open(str(d / "ref" / (fmt + ".mindrem.id")), "rb").read()
    assert "sample filter (--mind): host pass" in got.stdout and "founders=146 " in got.stdout, got.stdout
    # a .fam always has an FID column (WriteSampleIds: "#FID<tab>IID"); the .psam here has none ("#IID")
    assert open(str(d / "host" / (fmt + ".mindrem.id"))).read().startswith("#FID\tIID\ns3\ts3\n" if fmt == "bed" else "#IID\ns3\n")
