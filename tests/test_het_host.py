"""plink2-hip --het, the host's pass (--debug-host-filter), against the reference binary on the CPU: <out>.het (and .het.zst, decompressed)
and the log lines -- the warning about skipped variants in its singular and plural, word-wrapped as the reference wraps it, the
`Excluding ... non-autosomes` line, `--het: Results written to ...` and the errors -- byte for byte.  A fileset is a fixture only where the
reference writes the same bytes with --threads 1 and --threads 4 (het_tools.reference_runs); every case asserts that first, so a seed that
stops qualifying shows as such and not as a difference of plink2-hip's."""
import os

import numpy as np
import pytest

import ldtools as T
import het_tools as H


@pytest.fixture(scope="module")
def cli():
    import __graft_entry__ as ge
    return ge.load_package().build_cli()


@pytest.fixture(scope="module")
def filesets(tmp_path_factory):
    """rate -> directory: 0 % / 1 % / 5 % missing calls, each with a sample missing everything, two monomorphic variants and one nobody has a call
    at; the 1 % set has non-founders"""
    assert T.have_ref()
    out = {}
    for rate in (0.0, 0.01, 0.05):
        d = tmp_path_factory.mktemp("het_r%d" % int(rate * 100))
        raw = H.codes(rate)
        assert (raw[:, H.S_ALL_MISSING] == 3).all() and (raw[H.V_ALL_MISSING] == 3).all() and all(((raw[v] == 0) | (raw[v] == 3)).all() for v in H.V_MONO)
        H.write_fileset(d, raw, nonfounders=(7, 8, 30) if rate == 0.01 else ())
        out[rate] = d
    return out


@pytest.fixture(scope="module")
def sexed(tmp_path_factory):
    """1 % missing, 30 chrX and 10 MT variants behind the autosomes, both sexes"""
    assert T.have_ref()
    d = tmp_path_factory.mktemp("het_x")
    H.write_fileset(d, H.codes(0.01), names=H.chrom_names(H.M, x=30, mt=10), sexes=[1 + (s % 2) for s in range(H.N)])
    open(str(d / "mono.txt"), "w").write("snp%d\nsnp%d\n" % H.V_MONO)
    open(str(d / "one.txt"), "w").write("snp%d\nsnp50\n" % H.V_MONO[0])
    return d


@pytest.fixture(scope="module")
def multiallelic(tmp_path_factory):
    assert T.have_ref()
    d = tmp_path_factory.mktemp("het_multi")
    first, second, alt_ct = H.write_multiallelic_fileset(d, nonfounders=(3, 9))
    return d


def compare(cli, d, args, tag, zs=False):
    ref, qualifies = H.reference_runs(d, args, tag, zs)
    assert ref.returncode == 0, ref.stdout[-800:]
    assert qualifies, "the reference's --threads 1 and --threads 4 outputs differ: this fileset is no fixture (pick another seed)"
    host = H.run_cli(cli, args + ["--debug-host-filter", "--timing", "--out", tag], d / "host")
    assert host.returncode == 0, host.stdout[-1500:]
    assert "[timing] --het: host pass" in host.stdout and "from the resident image" not in host.stdout, host.stdout[-800:]
    H.assert_same_as_reference(d, "host", tag, zs)
    return ref, host


@pytest.mark.parametrize("rate", (0.0, 0.01, 0.05))
@pytest.mark.parametrize("fmt", list(H.FORMATS))
@pytest.mark.parametrize("mods", ([], ["small-sample"]), ids=("default", "small-sample"))
def test_formats_missing_rates_and_nonfounders(cli, filesets, rate, fmt, mods):
    """the warning: two monomorphic variants by default (the variable-width file's all-missing variant makes three, as in the reference),
    three under small-sample everywhere"""
    d = filesets[rate]
    tag = "t" + fmt[:1] + fmt[-1] + ("s" if mods else "")
    ref, host = compare(cli, d, H.FORMATS[fmt] + ["--het"] + mods, tag)
    warning = [l for l in H.het_lines(str(d / "host" / (tag + ".log"))) if l.startswith("Warning:")]
    want = 3 if (mods or fmt == "pgen-varwidth") else 2
    assert warning and warning[0].startswith("Warning: %d variants skipped because they were monomorphic." % want), warning
    rows = H.read_het(str(d / "host" / (tag + ".het"))).decode().split("\n")
    ids = ("#FID\tIID", "s%d\ts%d" % (H.S_ALL_MISSING, H.S_ALL_MISSING)) if fmt == "bed" else ("#IID", "s%d" % H.S_ALL_MISSING)   # (the .fam has a FID column)
    assert rows[0] == ids[0] + "\tO(HOM)\tE(HOM)\tOBS_CT\tF" and rows[1 + H.S_ALL_MISSING] == ids[1] + "\t0\t0\t0\tnan", rows[:8]


def test_zs(cli, filesets):
    compare(cli, filesets[0.01], ["--pfile", "../d", "--het", "zs"], "z", zs=True)


def test_singular_warning(cli, sexed):
    ref, host = compare(cli, sexed, ["--pfile", "../d", "--extract", "../one.txt", "--het"], "one")
    assert "Warning: 1 variant skipped because it was monomorphic." in host.stdout
    compare(cli, sexed, ["--pfile", "../v", "--extract", "../one.txt", "--het", "small-sample"], "ones")


def test_only_monomorphic_variants_left(cli, sexed):
    """every variant skipped: the report is still written, nobody has an observation (`nan`), as in the reference"""
    ref, host = compare(cli, sexed, ["--pfile", "../d", "--extract", "../mono.txt", "--het"], "mono")
    rows = H.read_het(str(sexed / "host" / "mono.het")).decode().split("\n")
    assert rows[1] == "s0\t0\t0\t0\tnan", rows[:3]


@pytest.mark.parametrize("fmt", list(H.FORMATS))
def test_chrx_and_mt_are_excluded(cli, sexed, fmt):
    tag = "x" + fmt[:1] + fmt[-1]
    ref, host = compare(cli, sexed, H.FORMATS[fmt] + ["--het"], tag)
    assert "Excluding 40 variants on non-autosomes from --het." in host.stdout


def test_only_non_autosomal_variants_left(cli, sexed):
    args = ["--pfile", "../d", "--chr", "X,MT", "--het"]
    ref, qualifies = H.reference_runs(sexed, args, "xo")
    host = H.run_cli(cli, args + ["--debug-host-filter", "--out", "xo"], sexed / "host")
    assert ref.returncode == host.returncode == 7 and qualifies, (ref.returncode, host.returncode, host.stdout[-600:])
    want = ["Excluding 40 variants on non-autosomes from --het.", "Error: No variants remaining for --het.",
            "Error: --het requires at least one polymorphic autosomal variant."]
    assert H.het_lines(str(sexed / "ref" / "xo.log")) == want and H.het_lines(str(sexed / "host" / "xo.log")) == want
    assert not os.path.exists(str(sexed / "host" / "xo.het"))


@pytest.mark.parametrize("args,tag", (
    (["--pfile", "../d", "--autosome", "--geno", "0.02", "--maf", "0.1", "--het"], "fp"),
    (["--bfile", "../d", "--autosome", "--geno", "0.02", "--maf", "0.1", "--het", "small-sample"], "fb"),
    (["--pfile", "../v", "--autosome", "--maf", "0.2", "--mind", "0.5", "--het"], "fv"),
), ids=("pgen", "bed-small-sample", "varwidth-mind"))
def test_the_variant_set_is_the_filtered_one(cli, sexed, args, tag):
    ref, host = compare(cli, sexed, args, tag)
    plain = H.read_het(str(sexed / "ref" / "xpd.het")) if os.path.exists(str(sexed / "ref" / "xpd.het")) else None
    assert "removed due to" in "\n".join(H.het_lines(str(sexed / "host" / (tag + ".log"))))
    assert plain is None or plain != H.read_het(str(sexed / "host" / (tag + ".het"))), "the filters changed nothing: the case shows nothing"


@pytest.mark.parametrize("mods", ([], ["small-sample"]), ids=("default", "small-sample"))
def test_multiallelic_variants(cli, multiallelic, mods):
    """2-4 alleles, altx/alty hets, non-founders, a variant with one allele alone among the calls and one nobody has a call at"""
    compare(cli, multiallelic, ["--pfile", "../v", "--het"] + mods, "m" + ("s" if mods else ""))
