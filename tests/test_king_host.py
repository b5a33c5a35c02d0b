"""plink2-hip --make-king-table, the host's pass, against the reference binary on the CPU: <out>.kin0 (and .kin0.zst, decompressed; .kin0.id
where `id` is not among the columns) and the log lines -- `Excluding ... non-autosomes from KING-robust calculation.`, `--make-king-table: N
variants processed.`, `Results written to ...`, `--king-table-filter: ...` and the errors -- byte for byte, on .bed, fixed-width and
variable-width .pgen, with non-founders, multiallelic variants, chrX / MT beside the autosomes, filters in front, FID / SID columns present
and absent, two samples, and the two error cases."""
import os

import numpy as np
import pytest

import het_tools as H
import king_tools as K
import ldtools as T

HOST = ["--debug-host-filter", "--timing"]


@pytest.fixture(scope="module")
def cli():
    import __graft_entry__ as ge
    return ge.load_package().build_cli()


def planted(rate=0.04):
    raw = H.codes(rate).copy()           # a sample without a call (5), a variant without one (11), two monomorphic variants
    raw[:, 9] = np.where(raw[:, 9] == 1, 2, raw[:, 9])   # never het
    raw[:, 31] = raw[:, 30]              # identical samples
    return raw


@pytest.fixture(scope="module")
def fileset(tmp_path_factory):
    """120 samples x 400 variants, 30 on chrX and 10 on MT, both sexes, samples 7, 8 and 30 with parents"""
    assert T.have_ref()
    d = tmp_path_factory.mktemp("king_host")
    H.write_fileset(d, planted(), names=H.chrom_names(H.M, x=30, mt=10), sexes=[1 + (s % 2) for s in range(H.N)], nonfounders=(7, 8, 30))
    open(str(d / "two.txt"), "w").write("s3\ns40\n")
    open(str(d / "one.txt"), "w").write("s3\n")
    open(str(d / "some.txt"), "w").write("".join("s%d\n" % s for s in range(0, H.N, 3)))
    return d


@pytest.fixture(scope="module")
def with_ids(tmp_path_factory):
    """60 founders, autosomes only; d: .psam with FID and SID columns, e: neither"""
    assert T.have_ref()
    d = tmp_path_factory.mktemp("king_ids")
    raw = planted()[:200, :60]
    names = ["1"] * 200
    for prefix in ("d", "e"):
        T.write_pgen_fixed(str(d / prefix), raw, names, H.positions(names))
    with open(str(d / "d.psam"), "w") as f:
        f.write("#FID\tIID\tSID\tSEX\n")
        for s in range(60):
            f.write("f%d\ts%d\tx%d\t2\n" % (s // 4, s, s % 3))
    H.make_dirs(d)
    return d


@pytest.fixture(scope="module")
def multiallelic(tmp_path_factory):
    assert T.have_ref()
    d = tmp_path_factory.mktemp("king_multi")
    H.write_multiallelic_fileset(d, nonfounders=(3, 9))
    return d


def compare(cli, d, args, tag, zs=False, id_file=False, forced=True):
    ref = T.run_ref(args + ["--out", tag], str(d / "ref"))
    assert ref.returncode == 0, ref.stdout[-800:]
    host = H.run_cli(cli, args + (HOST if forced else ["--timing"]) + ["--out", tag], d / "host")
    assert host.returncode == 0, host.stdout[-1500:]
    assert "[timing] --make-king-table: host pass" in host.stdout and "from the resident image" not in host.stdout, host.stdout[-800:]
    K.assert_same_as_reference(d, "host", tag, zs, id_file)
    return ref, host


@pytest.mark.parametrize("fmt", list(H.FORMATS))
@pytest.mark.parametrize("mods", ([], ["counts"], ["cols=id,nsnp,hethet,ibs0,ibs1,ibs,kinship"], ["--king-table-filter", "0.1"]), ids=("default", "counts", "ibs1", "filter"))
def test_formats_nonfounders_and_chrx_mt(cli, fileset, fmt, mods):
    """every case has non-founders among its samples and 40 non-autosomal variants behind the autosomes: the host's pass without being forced"""
    tag = "t" + fmt[:1] + fmt[-1] + (mods[0][:2].strip("-") if mods else "")
    ref, host = compare(cli, fileset, H.FORMATS[fmt] + ["--make-king-table"] + mods, tag, forced=False)
    assert "Excluding 40 variants on non-autosomes from KING-robust calculation." in host.stdout
    assert "--make-king-table: 360 variants processed." in host.stdout
    assert "non-founders among the kept samples" in host.stdout
    text = open(str(fileset / "host" / (tag + ".kin0"))).read()
    if not mods:
        assert "\tnan\n" in text and "\t-inf\n" in text
    if mods and mods[0] == "--king-table-filter":
        assert "\tnan\n" in text and "-inf" not in text and "--king-table-filter: " in host.stdout


def test_zs(cli, fileset):
    compare(cli, fileset, ["--pfile", "../d", "--make-king-table", "zs", "counts"], "z", zs=True)


def test_the_variant_and_sample_sets_are_the_filtered_ones(cli, fileset):
    plain = open(str(fileset / "ref" / "tpd.kin0"), "rb").read() if os.path.exists(str(fileset / "ref" / "tpd.kin0")) else None
    ref, host = compare(cli, fileset, ["--pfile", "../d", "--autosome", "--geno", "0.03", "--maf", "0.1", "--make-king-table"], "fg")
    assert "removed due to" in "\n".join(K.king_lines(str(fileset / "host" / "fg.log")))
    assert plain is None or plain != open(str(fileset / "host" / "fg.kin0"), "rb").read()
    compare(cli, fileset, ["--bfile", "../d", "--autosome", "--geno", "0.05", "--maf", "0.2", "--make-king-table", "counts"], "fb")
    ref, host = compare(cli, fileset, ["--pfile", "../d", "--keep", "../some.txt", "--autosome", "--maf", "0.05", "--make-king-table", "counts"], "fk")
    assert open(str(fileset / "host" / "fk.kin0")).read().count("\n") == 1 + 40 * 39 // 2
    compare(cli, fileset, ["--pfile", "../v", "--keep", "../some.txt", "--not-chr", "X", "--mind", "0.5", "--make-king-table"], "fm")


def test_two_samples(cli, fileset):
    ref, host = compare(cli, fileset, ["--pfile", "../d", "--keep", "../two.txt", "--make-king-table"], "two")
    assert open(str(fileset / "host" / "two.kin0")).read().split("\n")[1].startswith("s40\ts3\t")


def test_fewer_than_two_samples(cli, fileset):
    args = ["--pfile", "../d", "--keep", "../one.txt", "--make-king-table"]
    ref = T.run_ref(args + ["--out", "one"], str(fileset / "ref"))
    host = H.run_cli(cli, args + HOST + ["--out", "one"], fileset / "host")
    assert ref.returncode == host.returncode == 13, (ref.returncode, host.returncode, host.stdout[-600:])
    want = ["Error: --make-king-table requires at least 2 samples."]
    assert K.king_lines(str(fileset / "ref" / "one.log")) == want and K.king_lines(str(fileset / "host" / "one.log")) == want
    assert not os.path.exists(str(fileset / "host" / "one.kin0"))


def test_no_autosomal_variant_left(cli, fileset):
    args = ["--pfile", "../d", "--chr", "X,MT", "--make-king-table"]
    ref = T.run_ref(args + ["--out", "xo"], str(fileset / "ref"))
    host = H.run_cli(cli, args + HOST + ["--out", "xo"], fileset / "host")
    assert ref.returncode == host.returncode == 13, (ref.returncode, host.returncode, host.stdout[-600:])
    want = ["Excluding 40 variants on non-autosomes from KING-robust calculation.", "Error: No variants remaining for KING-robust calculation."]
    assert K.king_lines(str(fileset / "ref" / "xo.log")) == want and K.king_lines(str(fileset / "host" / "xo.log")) == want
    assert not os.path.exists(str(fileset / "host" / "xo.kin0"))


@pytest.mark.parametrize("src,mods,tag,id_file", (
    ("../d", [], "a", False),                                  # FID and SID columns in the file: maybefid / maybesid print them
    ("../d", ["cols=id,kinship"], "b", False),                 # ... and 'id' alone does not
    ("../d", ["cols=fid,id,sid,nsnp"], "c", False),
    ("../e", [], "g", False),                                  # neither column in the file
    ("../e", ["cols=fid,id,sid,nsnp,kinship"], "h", False),    # ... printed as 0 all the same
    ("../d", ["cols=nsnp,hethet,kinship"], "i", True),         # no 'id': the samples go to .kin0.id
    ("../e", ["counts", "cols=ibs0,ibs"], "j", True),
), ids=("both", "id-only", "fid-sid", "neither", "forced", "idfile", "idfile-plain"))
def test_fid_and_sid_columns(cli, with_ids, src, mods, tag, id_file):
    ref, host = compare(cli, with_ids, ["--pfile", src, "--make-king-table"] + mods, tag, id_file=id_file)
    head = open(str(with_ids / "host" / (tag + ".kin0"))).readline()
    if tag == "a":
        assert head.startswith("#FID1\tIID1\tSID1\tFID2\tIID2\tSID2\tNSNP")
    if tag == "g":
        assert head.startswith("#IID1\tIID2\tNSNP")
    if id_file:
        assert " and %s.kin0.id ." % tag in host.stdout


@pytest.mark.parametrize("mods", ([], ["counts", "cols=id,nsnp,ibs1,ibs,kinship"]), ids=("default", "counts-ibs1"))
def test_multiallelic_variants(cli, multiallelic, mods):
    """2-4 alleles, altx/alty calls (homozygous-ALT on the main track), non-founders: the host's pass without being forced"""
    ref, host = compare(cli, multiallelic, ["--pfile", "../v", "--make-king-table"] + mods, "m" + ("c" if mods else ""), forced=False)
