"""plink2-hip --missing / --freq / --geno-counts from the host's pass, on the CPU (no device is touched: runs of reports alone with
--debug-host-filter), against the reference binary file for file as bytes, log lines included: .bed, fixed-width and variable-width .pgen;
after --mind; before --geno / --maf; with non-founders (--freq counts founders, the other two everybody); 'zs'; and a VCF-imported file with
2-5 ALT alleles through --freq, --freq counts and --missing."""
import os
import re
import subprocess

import numpy as np
import pytest

import ldtools as T
import reports_tools as RT
from test_pgen_reader import make_multiallelic_vcf


@pytest.fixture(scope="module")
def cli():
    import __graft_entry__ as ge
    return ge.load_package().build_cli()


@pytest.fixture(scope="module")
def fileset(tmp_path_factory):
    if not T.have_ref():
        pytest.skip("needs the reference binary (oracle/_ref/plink2)")
    d = tmp_path_factory.mktemp("reports_host")
    raw = RT.codes()
    RT.check_fixture(raw)
    RT.write_fileset(d, raw)
    return d, raw


def both(cli, d, args, tag, extra_cli=()):
    ref = T.run_ref(args + ["--threads", "2", "--out", tag], str(d / "ref"))
    got = RT.run_cli(cli, args + ["--debug-host-filter", "--timing", "--out", tag] + list(extra_cli), d / "host")
    return ref, got


def check(d, ref, got, tag, exts, want_lines):
    assert ref.returncode == 0 and got.returncode == 0, (ref.stdout[-800:], got.stdout[-1500:])
    assert re.search(r"reports: host pass \([0-9.]+ s; --debug-host-filter\)", got.stdout) and "reports: from the device" not in got.stdout, got.stdout[-1500:]
    RT.same_bytes(d, "host", tag, exts)
    want = RT.report_lines(str(d / "ref" / (tag + ".log")))
    assert len(want) == want_lines, want
    assert RT.report_lines(str(d / "host" / (tag + ".log"))) == want


@pytest.mark.parametrize("fmt", list(RT.FORMATS))
def test_reports_alone_match_the_reference(cli, fileset, fmt):
    d, raw = fileset
    ref, got = both(cli, d, RT.FORMATS[fmt] + RT.REPORTS, fmt)
    check(d, ref, got, fmt, RT.EXTS, 4)
    # what the fixture was built for shows in the reference's own files
    afreq = open(str(d / "ref" / (fmt + ".afreq"))).read().split("\n")
    assert afreq[1 + RT.V_ALL_MISSING].endswith("\tnan\t0") and afreq[1].startswith("0\t")
    assert afreq[1 + RT.V_MONO].split("\t")[-2] == "0" and float(afreq[1 + RT.V_ALT_MAJOR].split("\t")[-2]) > 0.5
    smiss = open(str(d / "ref" / (fmt + ".smiss"))).read().split("\n")
    assert smiss[1 + RT.S_COMPLETE].split("\t")[-3:] == ["1", str(RT.M), "0.00333333"]
    assert len(smiss) == RT.N + 2
    want_cols = {"bed": "#CHROM\tID\tREF\tALT\tPROVISIONAL_REF?\tALT_FREQS\tOBS_CT"}.get(fmt, "#CHROM\tID\tREF\tALT\tALT_FREQS\tOBS_CT")
    assert afreq[0] == want_cols


def test_freq_counts_and_the_two_halves_of_missing(cli, fileset):
    d, _ = fileset
    ref, got = both(cli, d, RT.FORMATS["pgen-fixed"] + ["--freq", "counts", "--missing", "variant-only"], "cnt")
    check(d, ref, got, "cnt", (".acount", ".vmiss"), 2)
    assert not os.path.exists(str(d / "ref" / "cnt.smiss")) and not os.path.exists(str(d / "host" / "cnt.smiss"))
    ref, got = both(cli, d, RT.FORMATS["bed"] + ["--missing", "sample-only"], "so")
    check(d, ref, got, "so", (".smiss",), 1)
    assert not os.path.exists(str(d / "ref" / "so.vmiss")) and not os.path.exists(str(d / "host" / "so.vmiss"))


@pytest.mark.parametrize("fmt", list(RT.FORMATS))
def test_reports_come_after_mind(cli, fileset, fmt):
    d, raw = fileset
    ref, got = both(cli, d, RT.FORMATS[fmt] + ["--mind", "0.1"] + RT.REPORTS, RT.TAG[fmt] + "m")
    check(d, ref, got, RT.TAG[fmt] + "m", RT.EXTS + (".mindrem.id",), 5)
    smiss = open(str(d / "ref" / (RT.TAG[fmt] + "m.smiss"))).read().split("\n")
    assert len(smiss) == RT.N - len(RT.S_30PCT) + 2                      # the removed samples are not listed ...
    vmiss = open(str(d / "ref" / (RT.TAG[fmt] + "m.vmiss"))).read().split("\n")
    assert vmiss[1].split("\t")[3] == str(RT.N - len(RT.S_30PCT))        # ... and not counted


def test_reports_come_before_geno_and_maf(cli, fileset):
    d, raw = fileset
    # (the filters run for a command's sake: the reference prunes, plink2-hip plans the same prune with --dry-run, which needs no device)
    args = RT.FORMATS["pgen-fixed"] + RT.REPORTS + ["--geno", "0.05", "--maf", "0.1"] + RT.PRUNE
    ref, got = both(cli, d, args, "filt", extra_cli=["--dry-run"])
    check(d, ref, got, "filt", RT.EXTS, 6)
    want = RT.report_lines(str(d / "ref" / "filt.log"))
    assert want[4].startswith("--geno: ") and not want[4].startswith("--geno: 0 ") and "allele frequency" in want[5] and not want[5].startswith("0 ")
    # ... and a run of reports alone filters no variant, as the reference does not
    ref, got = both(cli, d, RT.FORMATS["pgen-fixed"] + RT.REPORTS + ["--geno", "0.05", "--maf", "0.1"], "filt0")
    check(d, ref, got, "filt0", RT.EXTS, 4)
    # the reports still list every variant, the removed ones included
    assert len(open(str(d / "ref" / "filt.vmiss")).read().split("\n")) == RT.M + 2


def test_freq_counts_founders_and_missing_everybody(cli, tmp_path):
    if not T.have_ref():
        pytest.skip("needs the reference binary (oracle/_ref/plink2)")
    raw = RT.codes(seed=9)
    RT.check_fixture(raw)
    nonfounders = (5, 17, 18, 40, 59)
    RT.write_fileset(tmp_path, raw, nonfounders=nonfounders)
    for fmt in ("bed", "pgen-varwidth"):
        ref, got = both(cli, tmp_path, RT.FORMATS[fmt] + RT.REPORTS, fmt)
        check(tmp_path, ref, got, fmt, RT.EXTS, 4)
        afreq = [l.split("\t") for l in open(str(tmp_path / "ref" / (fmt + ".afreq"))).read().split("\n")[1:-1]]
        vmiss = [l.split("\t") for l in open(str(tmp_path / "ref" / (fmt + ".vmiss"))).read().split("\n")[1:-1]]
        gcount = [l.split("\t") for l in open(str(tmp_path / "ref" / (fmt + ".gcount"))).read().split("\n")[1:-1]]
        assert all(v[3] == str(RT.N) for v in vmiss)
        differ = [q for q in range(RT.M) if int(afreq[q][-1]) != 2 * (int(vmiss[q][3]) - int(vmiss[q][2]))]
        assert differ, "the founders' and everybody's counts agree on every line: the fileset tells nothing apart"
        assert all(sum(int(x) for x in g[-6:-3]) + int(g[-1]) == RT.N for g in gcount)     # --geno-counts: everybody
    # "--freq counts" with non-founders needs --ac-founders, as for the reference
    args = RT.FORMATS["pgen-fixed"] + ["--freq", "counts"]
    ref, got = both(cli, tmp_path, args, "acf")
    assert ref.returncode == got.returncode == 7 and "nonfounders are present" in got.stdout, (ref.returncode, got.returncode, got.stdout[-600:])
    ref, got = both(cli, tmp_path, args + ["--ac-founders"], "acf2")
    check(tmp_path, ref, got, "acf2", (".acount",), 1)


def test_zs_reports_decompress_to_the_reference_text(cli, fileset):
    d, _ = fileset
    plain = T.run_ref(RT.FORMATS["pgen-fixed"] + RT.REPORTS + ["--out", "zsplain"], str(d / "ref"))
    assert plain.returncode == 0
    got = RT.run_cli(cli, RT.FORMATS["pgen-fixed"] + ["--freq", "zs", "--geno-counts", "zs", "--missing", "zs", "--debug-host-filter", "--out", "zs"], d / "host")
    assert got.returncode == 0, got.stdout[-1500:]
    for ext in RT.EXTS:
        assert ("zs%s.zst ." % ext) in got.stdout, got.stdout
        back = subprocess.run([T.REF_BIN, "--zst-decompress", "zs" + ext + ".zst"], cwd=str(d / "host"), stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=120)
        assert back.returncode == 0 and back.stdout == open(str(d / "ref" / ("zsplain" + ext)), "rb").read(), ext


def test_multiallelic_variants_through_freq_and_missing(cli, tmp_path):
    if not T.have_ref():
        pytest.skip("needs the reference binary (oracle/_ref/plink2)")
    m, n = 120, 70
    alt_ct, lo, hi = make_multiallelic_vcf(str(tmp_path / "d.vcf"), m, n, seed=12, max_alt=5, missing=0.04)
    assert set(int(a) for a in alt_ct) >= {2, 3, 4, 5}
    T.ref_import_vcf(str(tmp_path / "d.vcf"), str(tmp_path / "d"))
    for sub in ("ref", "host"):
        os.makedirs(str(tmp_path / sub))
    ref, got = both(cli, tmp_path, ["--pfile", "../d", "--freq", "--missing"], "f")
    check(tmp_path, ref, got, "f", (".afreq", ".smiss", ".vmiss"), 3)
    ref, got = both(cli, tmp_path, ["--pfile", "../d", "--freq", "counts", "--missing", "variant-only"], "c")
    check(tmp_path, ref, got, "c", (".acount", ".vmiss"), 2)
    # the counts are the file's: allele a of variant v is named by this many of the VCF's allele pairs
    acount = [l.split("\t") for l in open(str(tmp_path / "ref" / "c.acount")).read().split("\n")[1:-1]]
    for v in (1, 2, 3):
        want = [int(((lo[v] == a).sum() + (hi[v] == a).sum())) for a in range(1, int(alt_ct[v]) + 1)]
        assert [int(x) for x in acount[v][-2].split(",")] == want, v
    # --geno-counts would have to count the genotype pairs of such a variant: refused by name, and taken again once --max-alleles leaves them out
    r = RT.run_cli(cli, ["--pfile", "../d", "--geno-counts", "--debug-host-filter", "--out", "g"], tmp_path / "host")
    assert r.returncode == 63 and "--geno-counts" in r.stdout and "multiallelic" in r.stdout, r.stdout
    ref, got = both(cli, tmp_path, ["--pfile", "../d", "--geno-counts", "--max-alleles", "2"], "g2")
    check(tmp_path, ref, got, "g2", (".gcount",), 1)
