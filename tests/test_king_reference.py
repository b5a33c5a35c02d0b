"""The yardstick of the king tests, pinned before any device is involved: the numpy definition of king_tools and a formatter written from
it reproduce the reference's .kin0 byte for byte on a planted fileset -- 70 samples, 300 variants of which 15 lie on chrX and 5 on MT (left
out by the reference), 4 % missing calls, a sample without any call (`nan` lines), a sample without a het call (`-inf` lines), two identical
samples and a variant nobody has a call at -- with the default columns, with `counts`, with the ibs1 / ibs column sets (the orientation of
HET1_HOM2 included) and under --king-table-filter.  The reference writes the same file with one thread and with its default."""
import os

import numpy as np
import pytest

import king_tools as K
import ldtools as T


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    assert T.have_ref()
    d = tmp_path_factory.mktemp("king_ref")
    raw, chroms, bps = K.planted_codes()
    iids = K.write_fileset(str(d / "d"), raw, chroms, bps)
    c = K.counts(raw[K.autosomal(chroms)])
    return d, raw, c, iids


def ref_table(d, extra, out):
    cp, prefix = K.run_ref_king(str(d), ["--pfile", "d"], extra, out)
    assert cp.returncode == 0, cp.stdout[-800:]
    return open(prefix + ".kin0").read(), open(prefix + ".log").read()


def test_the_planted_cases_are_there(planted):
    d, raw, c, iids = planted
    k = K.kinship(c)
    low = np.tril(np.ones(k.shape, dtype=bool), -1)
    assert np.isnan(k[5, :5]).all() and np.isneginf(k[low]).any() and (k[31, 30] == 0.5 or K.nsnp(c)[31, 30] == 0)
    assert (c["het_row_hom_col"][low] != c["hom_row_het_col"][low]).any(), "an orientation test needs asymmetric counts"
    assert not K.nsnp(c)[5].any()


@pytest.mark.parametrize("extra,cols,report_counts", (
    ([], K.DEFAULT_COLS, False),
    (["counts"], K.DEFAULT_COLS, True),
    (["cols=id,nsnp,hethet,ibs0,ibs1,ibs,kinship"], ("id", "nsnp", "hethet", "ibs0", "ibs1", "ibs", "kinship"), False),
    (["counts", "cols=id,nsnp,hethet,ibs0,ibs1,ibs,kinship"], ("id", "nsnp", "hethet", "ibs0", "ibs1", "ibs", "kinship"), True),
), ids=("default", "counts", "ibs1-ibs", "ibs1-ibs-counts"))
def test_definition_and_formatter_give_the_reference_bytes(planted, extra, cols, report_counts):
    d, raw, c, iids = planted
    got, log = ref_table(d, extra, "t%d" % (len(extra) * 2 + int(report_counts)))
    want, _ = K.kin0_text(c, iids, cols, report_counts)
    assert got.count("\n") == 1 + 70 * 69 // 2
    assert got == want
    assert "Excluding 20 variants on non-autosomes from KING-robust calculation." in log
    assert "--make-king-table: 280 variants processed." in log


def test_het1_hom2_counts_the_second_sample_of_the_line(planted):
    d, raw, c, iids = planted
    got, _ = ref_table(d, ["counts", "cols=id,ibs1"], "o")
    lines = got.split("\n")
    assert lines[0] == "#IID1\tIID2\tHET1_HOM2\tHET2_HOM1" and lines[1].split("\t")[:2] == ["s1", "s0"]
    auto = raw[K.autosomal(K.planted_codes()[1])]
    s0_het_s1_hom = int(((auto[:, 0] == 1) & ((auto[:, 1] == 0) | (auto[:, 1] == 2))).sum())
    s1_het_s0_hom = int(((auto[:, 1] == 1) & ((auto[:, 0] == 0) | (auto[:, 0] == 2))).sum())
    assert s0_het_s1_hom != s1_het_s0_hom
    assert lines[1].split("\t")[2:] == [str(s0_het_s1_hom), str(s1_het_s0_hom)]


def test_filter_keeps_nan_and_drops_minus_inf(planted):
    d, raw, c, iids = planted
    got, log = ref_table(d, ["--king-table-filter", "0.1"], "f")
    want, filtered = K.kin0_text(c, iids, king_filter=0.1)
    assert got == want
    total = 70 * 69 // 2
    assert (total - filtered, filtered) == (96, 2319)   # (this fileset's figures)
    assert ("--king-table-filter: %d relationships reported (%d filtered out)." % (total - filtered, filtered)) in log
    assert "\tnan\n" in got and "-inf" not in got and "-inf" in ref_table(d, [], "u")[0]


def test_one_thread_and_the_default_write_the_same_file(planted):
    d, raw, c, iids = planted
    one, _ = ref_table(d, ["--threads", "1"], "th1")
    dflt, _ = ref_table(d, [], "thd")
    assert one == dflt
