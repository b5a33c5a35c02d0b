"""plink2-hip's load on the CPU: which refusal a run reports when two compete, and what the filters' survivor counts are.  Every stage of
load_inputs() walks the variant table through one filter; a refusal about a chromosome fires when the chromosome's first variant is reached,
even where --extract / --exclude leave none of its variants, and a refusal about a variant of an earlier chromosome wins over it.  Every case
ends in load_inputs() or runs under --dry-run: no device, no reference binary.  EXPECT holds the exit code and the `Error:` / `dry-run:` /
`--extract:` / `--exclude:` lines of every case as the CLI printed them before the stages shared that filter; nothing here is computed from the
code under test."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ldtools as T

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pgen")
PRUNE = ["--indep-pairwise", "50", "5", "0.2", "--bad-ld"]
N, M = 40, 60
KEPT_LINES = ("Error:", "dry-run:", "--extract:", "--exclude:")


@pytest.fixture(scope="module")
def cli():
    import __graft_entry__ as ge
    return ge.load_package().build_cli()


def _small(d, name, chroms, nonfounders=(), alleles=None):
    """<d>/<name> as .bed and fixed-width .pgen: N samples, len(chroms) <= M variants snp0 ..; nonfounders: samples with parents;
    alleles: (REF, ALT) of every variant instead of A / C"""
    m = len(chroms)
    assert m <= M
    raw = T.synth_raw_codes(m, N, seed=3, missing_rate=0.02)
    bps = np.arange(m) * 10 + 1
    T.write_pgen_fixed(str(d / name), raw, chroms, bps)
    T.write_bed(str(d / name), raw, chroms, bps)
    if nonfounders:
        with open(str(d / (name + ".psam")), "w") as f:
            f.write("#IID\tPAT\tMAT\tSEX\n")
            for s in range(N):
                f.write("s%d\t%s\t%s\t2\n" % (s, "p1" if s in nonfounders else "0", "p2" if s in nonfounders else "0"))
        with open(str(d / (name + ".fam")), "w") as f:
            for s in range(N):
                f.write("s%d s%d %s %s 2 -9\n" % (s, s, "p1" if s in nonfounders else "0", "p2" if s in nonfounders else "0"))
    if alleles:
        with open(str(d / (name + ".pvar")), "w") as f:
            f.write("#CHROM\tPOS\tID\tREF\tALT\n")
            for i in range(m):
                f.write("%s\t%d\tsnp%d\t%s\t%s\n" % (chroms[i], bps[i], i, alleles[0], alleles[1]))
        with open(str(d / (name + ".bim")), "w") as f:
            for i in range(m):
                f.write("%s\tsnp%d\t0\t%d\t%s\t%s\n" % (chroms[i], i, bps[i], alleles[1], alleles[0]))


def _multi(d, name, chroms):
    """<d>/<name>.pvar / .psam, written by hand, beside a copy of the committed multiallelic .pgen (400 variants, 120 samples; a quarter of the
    variants have two or three ALT alleles, snp3 the first of them).  Returns the IDs of the multiallelic variants."""
    shutil.copy(os.path.join(GOLD, "phased_multi.pgen"), str(d / (name + ".pgen")))
    z = np.load(os.path.join(GOLD, "phased_multi.npz"))
    alt_ct = z["alt_ct"]
    assert len(chroms) == len(alt_ct) and alt_ct[3] == 2 and (alt_ct[:3] == 1).all()
    with open(str(d / (name + ".pvar")), "w") as f:
        f.write("#CHROM\tPOS\tID\tREF\tALT\n")
        for i, c in enumerate(chroms):
            f.write("%s\t%d\tsnp%d\tA\t%s\n" % (c, 1000 + 97 * i, i, ",".join("CGT"[:alt_ct[i]])))
    with open(str(d / (name + ".psam")), "w") as f:
        f.write("#IID\tSEX\n")
        for s in range(z["first"].shape[1]):
            f.write("s%d\t2\n" % s)
    return ["snp%d" % i for i in np.flatnonzero(alt_ct > 1)]


def _ids(d, name, ids):
    open(str(d / name), "w").write("".join("%s\n" % i for i in ids))


def write_files(d):
    r = lambda a, b: ["snp%d" % i for i in range(a, b)]
    _small(d, "x", ["1"] * 30 + ["2"] * 10 + ["X"] * 20)                 # a chrX block behind the autosomes
    _ids(d, "x_block.txt", r(40, 60))
    _small(d, "bad", ["1"] * 30 + ["contig7"] * 10 + ["2"] * 20)         # a chromosome of invalid code (no --allow-extra-chr)
    _ids(d, "bad_block.txt", r(30, 40))
    _small(d, "y", ["1"] * 30 + ["Y"] * 10 + ["2"] * 20)
    _small(d, "zero", ["0"] * 1 + ["1"] * 39 + ["2"] * 20)               # one unplaced variant
    _ids(d, "zero_block.txt", r(0, 1))
    _small(d, "xindel", ["X"] * 30, alleles=("AT", "A"))                 # a table of chrX indels
    _small(d, "nf", ["1"] * 40 + ["2"] * 20, nonfounders=(3, 9, 21))
    _small(d, "mt", ["1"] * 40 + ["MT"] * 20)
    _ids(d, "keep_some.txt", r(0, 50) + ["none_such"])
    _ids(d, "drop_some.txt", r(2, 12) + r(45, 55))
    multi = _multi(d, "m1x", ["1"] * 300 + ["X"] * 100)                  # multiallelic variants on chromosome 1 ahead of chrX
    _ids(d, "multi.txt", multi)
    _multi(d, "mx1", ["X"] * 100 + ["1"] * 300)                          # ... and behind it (snp3 is on chrX then: the first on chromosome 1 is snp107)
    _multi(d, "m12", ["1"] * 200 + ["2"] * 200)
    _ids(d, "keep_multi.txt", r(0, 300))
    _ids(d, "drop_multi.txt", r(0, 20) + r(290, 310))
    return d


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return write_files(tmp_path_factory.mktemp("refusal_order"))


BOTH = ("--bfile", "--pfile")
PFILE = ("--pfile",)   # (a .bim has no multiallelic variants)
# id -> (input forms, fileset, the other arguments)
CASES = {
    # 1. --geno-counts: a multiallelic variant on chromosome 1 ahead of a chrX block
    "gcount_multi_before_x": (PFILE, "m1x", ["--geno-counts"]),
    "gcount_multi_excluded_then_x": (PFILE, "m1x", ["--geno-counts", "--exclude", "multi.txt"]),
    # 2. --mind and a chromosome of invalid code
    "mind_invalid_chrom_all_excluded": (BOTH, "bad", ["--mind", "0.1", "--exclude", "bad_block.txt"] + PRUNE + ["--dry-run"]),
    "mind_invalid_chrom_not_chr": (BOTH, "bad", ["--mind", "0.1", "--not-chr", "contig7"] + PRUNE + ["--dry-run"]),
    # 3. --mind and chrY
    "mind_chry": (BOTH, "y", ["--mind", "0.1"] + PRUNE + ["--dry-run"]),
    "mind_chry_not_chr": (BOTH, "y", ["--mind", "0.1", "--not-chr", "y"] + PRUNE + ["--dry-run"]),
    # 4. --maf beside the prune, every chrX variant excluded by ID
    "maf_x_all_excluded": (BOTH, "x", ["--maf", "0.05", "--exclude", "x_block.txt"] + PRUNE),
    "maf_x_autosome": (BOTH, "x", ["--maf", "0.05", "--exclude", "x_block.txt", "--autosome"] + PRUNE + ["--dry-run"]),
    # 5. --hwe: a multiallelic variant and a chrX variant, in both orders
    "hwe_multi_before_x": (PFILE, "m1x", ["--hwe", "1e-6"] + PRUNE),
    "hwe_x_before_multi": (PFILE, "mx1", ["--hwe", "1e-6"] + PRUNE),
    # 6. --het / --make-king-table beside the prune with a chromosome 0 variant
    "het_chr0": (BOTH, "zero", ["--het", "--bad-freqs"] + PRUNE),
    "het_chr0_excluded": (BOTH, "zero", ["--het", "--bad-freqs", "--exclude", "zero_block.txt"] + PRUNE + ["--dry-run"]),
    "king_chr0": (BOTH, "zero", ["--make-king-table"] + PRUNE),
    "king_chr0_excluded": (BOTH, "zero", ["--make-king-table", "--exclude", "zero_block.txt"] + PRUNE + ["--dry-run"]),
    # 7. table filters that leave nothing
    "all_excluded_chr_max_alleles": (BOTH, "x", ["--chr", "5", "--max-alleles", "2"] + PRUNE),
    "all_excluded_autosome_snps_only": (BOTH, "xindel", ["--autosome", "--snps-only"] + PRUNE),
    # 8. the survivor counts of --extract / --exclude beside --max-alleles
    "survivors": (BOTH, "x", ["--extract", "keep_some.txt", "--exclude", "drop_some.txt", "--max-alleles", "2"] + PRUNE + ["--dry-run"]),
    "survivors_multi": (PFILE, "m12", ["--extract", "keep_multi.txt", "--exclude", "drop_multi.txt", "--max-alleles", "2"] + PRUNE + ["--dry-run"]),
}
# 9. the dry run's decisions: non-founders among the samples, an MT block among the variants
for _fs in ("nf", "mt"):
    CASES["dry_missing_" + _fs] = (BOTH, _fs, ["--missing", "--dry-run"])
    CASES["dry_het_" + _fs] = (BOTH, _fs, ["--het", "--bad-freqs", "--dry-run"])
    CASES["dry_king_" + _fs] = (BOTH, _fs, ["--make-king-table", "--dry-run"])
    CASES["dry_geno_" + _fs] = (BOTH, _fs, ["--geno", "0.1"] + PRUNE + ["--dry-run"])


def case_runs():
    for name, (forms, fileset, args) in CASES.items():
        for form in forms:
            yield name + "/" + form, [form, fileset] + args


def run_case(cli, d, args):
    """(exit code, the kept lines of stdout)"""
    r = subprocess.run([cli] + args + ["--out", "o"], cwd=str(d), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    lines = [l for l in r.stdout.split("\n") if l.startswith(KEPT_LINES)]
    return r.returncode, lines


EXPECT = {'gcount_multi_before_x/--pfile': (63, ["Error: --geno-counts with a multiallelic variant ('snp3') is not supported by plink2-hip: --max-alleles 2 leaves them out."]),
 'gcount_multi_excluded_then_x/--pfile': (63,
                                          ["Error: --geno-counts with chrX, chrY or MT variants ('X') is not supported by plink2-hip: filter them out (--autosome, --chr, --not-chr) or use "
                                           'plink2.']),
 'mind_invalid_chrom_all_excluded/--bfile': (6, ["Error: Invalid chromosome code 'contig7'. (Use --allow-extra-chr to force it to be accepted.)"]),
 'mind_invalid_chrom_all_excluded/--pfile': (6, ["Error: Invalid chromosome code 'contig7'. (Use --allow-extra-chr to force it to be accepted.)"]),
 'mind_invalid_chrom_not_chr/--bfile': (0,
                                        ['dry-run: sample filter (--mind): host pass over 50 variants',
                                         'dry-run: founders=40 variants=50 window=50 step=5 window_is_bp=0 r2=0x1.999999999999ap-3 order=2 subcontigs=2 candidate_pairs=625']),
 'mind_invalid_chrom_not_chr/--pfile': (0,
                                        ['dry-run: sample filter (--mind): host pass over 50 variants',
                                         'dry-run: founders=40 variants=50 window=50 step=5 window_is_bp=0 r2=0x1.999999999999ap-3 order=2 subcontigs=2 candidate_pairs=625']),
 'mind_chry/--bfile': (63, ["Error: --mind with chrY variants ('Y') is not supported by plink2-hip: filter them out (--autosome, --not-chr y) or pre-filter with plink2."]),
 'mind_chry/--pfile': (63, ["Error: --mind with chrY variants ('Y') is not supported by plink2-hip: filter them out (--autosome, --not-chr y) or pre-filter with plink2."]),
 'mind_chry_not_chr/--bfile': (0,
                               ['dry-run: sample filter (--mind): host pass over 50 variants',
                                'dry-run: founders=40 variants=50 window=50 step=5 window_is_bp=0 r2=0x1.999999999999ap-3 order=2 subcontigs=2 candidate_pairs=625']),
 'mind_chry_not_chr/--pfile': (0,
                               ['dry-run: sample filter (--mind): host pass over 50 variants',
                                'dry-run: founders=40 variants=50 window=50 step=5 window_is_bp=0 r2=0x1.999999999999ap-3 order=2 subcontigs=2 candidate_pairs=625']),
 'maf_x_all_excluded/--bfile': (63,
                                ["Error: --maf / --max-maf / --mac / --max-mac / --geno on chrX, chrY or MT ('X') are not supported by plink2-hip: filter them out (--autosome, --chr) or "
                                 'pre-filter with plink2.']),
 'maf_x_all_excluded/--pfile': (63,
                                ["Error: --maf / --max-maf / --mac / --max-mac / --geno on chrX, chrY or MT ('X') are not supported by plink2-hip: filter them out (--autosome, --chr) or "
                                 'pre-filter with plink2.']),
 'maf_x_autosome/--bfile': (0,
                            ["dry-run: variant filters: from the device's count pass",
                             '--exclude: 40 variants remaining.',
                             'dry-run: founders=40 variants=40 window=50 step=5 window_is_bp=0 r2=0x1.999999999999ap-3 order=2 subcontigs=2 candidate_pairs=480']),
 'maf_x_autosome/--pfile': (0,
                            ["dry-run: variant filters: from the device's count pass",
                             '--exclude: 40 variants remaining.',
                             'dry-run: founders=40 variants=40 window=50 step=5 window_is_bp=0 r2=0x1.999999999999ap-3 order=2 subcontigs=2 candidate_pairs=480']),
 'hwe_multi_before_x/--pfile': (63, ["Error: --hwe / --hardy with a multiallelic variant ('snp3') are not supported by plink2-hip: --max-alleles 2 leaves them out."]),
 'hwe_x_before_multi/--pfile': (63, ["Error: --hwe / --hardy with a chrX variant ('snp0') are not supported by plink2-hip: filter chrX out (--autosome, --not-chr) or use plink2."]),
 'het_chr0/--bfile': (63, ["Error: --het beside the prune with chromosome 0 variants ('snp0') is not supported by plink2-hip: run --het on its own, or filter them out (--not-chr 0)."]),
 'het_chr0/--pfile': (63, ["Error: --het beside the prune with chromosome 0 variants ('snp0') is not supported by plink2-hip: run --het on its own, or filter them out (--not-chr 0)."]),
 'het_chr0_excluded/--bfile': (0,
                               ['dry-run: --het: host pass: --dry-run',
                                '--exclude: 59 variants remaining.',
                                'dry-run: founders=40 variants=59 window=50 step=5 window_is_bp=0 r2=0x1.999999999999ap-3 order=2 subcontigs=2 candidate_pairs=931']),
 'het_chr0_excluded/--pfile': (0,
                               ['dry-run: --het: host pass: --dry-run',
                                '--exclude: 59 variants remaining.',
                                'dry-run: founders=40 variants=59 window=50 step=5 window_is_bp=0 r2=0x1.999999999999ap-3 order=2 subcontigs=2 candidate_pairs=931']),
 'king_chr0/--bfile': (63,
                       ["Error: --make-king-table beside the prune with chromosome 0 variants ('snp0') is not supported by plink2-hip: run it on its own, or filter them out (--not-chr "
                        '0).']),
 'king_chr0/--pfile': (63,
                       ["Error: --make-king-table beside the prune with chromosome 0 variants ('snp0') is not supported by plink2-hip: run it on its own, or filter them out (--not-chr "
                        '0).']),
 'king_chr0_excluded/--bfile': (0,
                                ['dry-run: --make-king-table: cols 0x4ed, filter none; from the resident image',
                                 '--exclude: 59 variants remaining.',
                                 'dry-run: founders=40 variants=59 window=50 step=5 window_is_bp=0 r2=0x1.999999999999ap-3 order=2 subcontigs=2 candidate_pairs=931']),
 'king_chr0_excluded/--pfile': (0,
                                ['dry-run: --make-king-table: cols 0x4ed, filter none; from the resident image',
                                 '--exclude: 59 variants remaining.',
                                 'dry-run: founders=40 variants=59 window=50 step=5 window_is_bp=0 r2=0x1.999999999999ap-3 order=2 subcontigs=2 candidate_pairs=931']),
 'all_excluded_chr_max_alleles/--bfile': (7, ['Error: All 60 variants in x.bim excluded by --chr + --max-alleles.']),
 'all_excluded_chr_max_alleles/--pfile': (7, ['Error: All 60 variants in x.pvar excluded by --chr + --max-alleles.']),
 'all_excluded_autosome_snps_only/--bfile': (7, ['Error: All 30 variants in xindel.bim excluded by --autosome + --snps-only.']),
 'all_excluded_autosome_snps_only/--pfile': (7, ['Error: All 30 variants in xindel.pvar excluded by --autosome + --snps-only.']),
 'survivors/--bfile': (0,
                       ['--extract: 50 variants remaining.',
                        '--exclude: 35 variants remaining.',
                        'dry-run: founders=40 variants=30 window=50 step=5 window_is_bp=0 r2=0x1.999999999999ap-3 order=2 subcontigs=2 candidate_pairs=235',
                        'dry-run: chrX variants=5 chrY variants=0 (separate engines)']),
 'survivors/--pfile': (0,
                       ['--extract: 50 variants remaining.',
                        '--exclude: 35 variants remaining.',
                        'dry-run: founders=40 variants=30 window=50 step=5 window_is_bp=0 r2=0x1.999999999999ap-3 order=2 subcontigs=2 candidate_pairs=235',
                        'dry-run: chrX variants=5 chrY variants=0 (separate engines)']),
 'survivors_multi/--pfile': (0,
                             ['--extract: 211 variants remaining.',
                              '--exclude: 190 variants remaining.',
                              'dry-run: founders=120 variants=190 window=50 step=5 window_is_bp=0 r2=0x1.999999999999ap-3 order=2 subcontigs=2 candidate_pairs=6674']),
 'dry_missing_nf/--bfile': (0, ["dry-run: reports: host pass: non-founders among the kept samples (--geno counts them, the device's rows hold founders only)"]),
 'dry_missing_nf/--pfile': (0, ["dry-run: reports: host pass: non-founders among the kept samples (--geno counts them, the device's rows hold founders only)"]),
 'dry_het_nf/--bfile': (0, ["dry-run: --het: host pass: non-founders among the kept samples (--geno counts them, the device's rows hold founders only)"]),
 'dry_het_nf/--pfile': (0, ["dry-run: --het: host pass: non-founders among the kept samples (--geno counts them, the device's rows hold founders only)"]),
 'dry_king_nf/--bfile': (0,
                         ["dry-run: --make-king-table: cols 0x4ed, filter none; host pass: non-founders among the kept samples (the table lists them, the device's rows hold founders "
                          'only)']),
 'dry_king_nf/--pfile': (0,
                         ["dry-run: --make-king-table: cols 0x4ed, filter none; host pass: non-founders among the kept samples (the table lists them, the device's rows hold founders "
                          'only)']),
 'dry_geno_nf/--bfile': (0,
                         ["dry-run: variant filters: host pass: non-founders among the kept samples (--geno counts them, the device's rows hold founders only)",
                          'dry-run: founders=37 variants=60 window=50 step=5 window_is_bp=0 r2=0x1.999999999999ap-3 order=2 subcontigs=2 candidate_pairs=970']),
 'dry_geno_nf/--pfile': (0,
                         ["dry-run: variant filters: host pass: non-founders among the kept samples (--geno counts them, the device's rows hold founders only)",
                          'dry-run: founders=37 variants=60 window=50 step=5 window_is_bp=0 r2=0x1.999999999999ap-3 order=2 subcontigs=2 candidate_pairs=970']),
 'dry_missing_mt/--bfile': (63, ["Error: --missing with chrX, chrY or MT variants ('MT') is not supported by plink2-hip: filter them out (--autosome, --chr, --not-chr) or use plink2."]),
 'dry_missing_mt/--pfile': (63, ["Error: --missing with chrX, chrY or MT variants ('MT') is not supported by plink2-hip: filter them out (--autosome, --chr, --not-chr) or use plink2."]),
 'dry_het_mt/--bfile': (0, ['dry-run: --het: host pass: --dry-run']),
 'dry_het_mt/--pfile': (0, ['dry-run: --het: host pass: --dry-run']),
 'dry_king_mt/--bfile': (0, ['dry-run: --make-king-table: cols 0x4ed, filter none; host pass: chrX / chrY / MT variants (their rows are built for engines of their own)']),
 'dry_king_mt/--pfile': (0, ['dry-run: --make-king-table: cols 0x4ed, filter none; host pass: chrX / chrY / MT variants (their rows are built for engines of their own)']),
 'dry_geno_mt/--bfile': (63,
                         ["Error: --maf / --max-maf / --mac / --max-mac / --geno on chrX, chrY or MT ('MT') are not supported by plink2-hip: filter them out (--autosome, --chr) or "
                          'pre-filter with plink2.']),
 'dry_geno_mt/--pfile': (63,
                         ["Error: --maf / --max-maf / --mac / --max-mac / --geno on chrX, chrY or MT ('MT') are not supported by plink2-hip: filter them out (--autosome, --chr) or "
                          'pre-filter with plink2.'])}


@pytest.mark.parametrize("run", [k for k, _ in case_runs()])
def test_refusal_and_counts(cli, files, run):
    got = run_case(cli, files, dict(case_runs())[run])
    assert got == EXPECT[run], got


def test_the_cases_say_what_they_are_about():
    """the properties the literals of EXPECT stand for, read off the literals themselves"""
    e = EXPECT
    assert e["gcount_multi_before_x/--pfile"][0] == 63 and "multiallelic variant ('snp3')" in e["gcount_multi_before_x/--pfile"][1][0]
    assert e["gcount_multi_excluded_then_x/--pfile"][0] == 63 and "chrX, chrY or MT variants ('X')" in e["gcount_multi_excluded_then_x/--pfile"][1][0]
    assert "multiallelic variant ('snp3')" in e["hwe_multi_before_x/--pfile"][1][0] and "chrX variant ('snp0')" in e["hwe_x_before_multi/--pfile"][1][0]
    for form in BOTH:
        assert e["mind_invalid_chrom_all_excluded/" + form][0] == 6 and e["mind_invalid_chrom_not_chr/" + form][0] == 0
        assert e["mind_chry/" + form][0] == 63 and e["mind_chry_not_chr/" + form][0] == 0
        assert e["maf_x_all_excluded/" + form][0] == 63 and e["maf_x_autosome/" + form][0] == 0
        assert e["het_chr0/" + form][0] == 63 and "run --het on its own" in e["het_chr0/" + form][1][0] and e["het_chr0_excluded/" + form][0] == 0
        assert e["king_chr0/" + form][0] == 63 and "run it on its own" in e["king_chr0/" + form][1][0] and e["king_chr0_excluded/" + form][0] == 0
        assert e["all_excluded_chr_max_alleles/" + form][0] == 7 and "excluded by --chr + --max-alleles." in e["all_excluded_chr_max_alleles/" + form][1][0]
        assert e["all_excluded_autosome_snps_only/" + form][0] == 7 and "excluded by --autosome + --snps-only." in e["all_excluded_autosome_snps_only/" + form][1][0]
