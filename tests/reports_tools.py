"""Filesets and helpers of the report tests (--missing / --freq / --geno-counts): test_cli_reports_args.py and test_reports_host.py on the CPU,
test_reports_device.py on the GPU."""
import os
import subprocess

import numpy as np

import ldtools as T

M, N = 300, 60
CHR0 = 4                      # the first variants lie on chromosome 0: the reports list them, the prune ignores them
V_COMPLETE, V_ALL_MISSING, V_MONO, V_ALT_MAJOR = 10, 11, 12, 13
S_COMPLETE = 7                # the sample without a missing call (the all-missing variant aside, which nobody has)
S_30PCT = (3, 41)             # samples --mind 0.1 removes
FORMATS = {"bed": ["--bfile", "../d"], "pgen-fixed": ["--pfile", "../d"], "pgen-varwidth": ["--pfile", "../v"]}
TAG = {"bed": "b", "pgen-fixed": "f", "pgen-varwidth": "v"}   # short --out names: the reference wraps its log lines at 79 characters
REPORTS = ["--freq", "--geno-counts", "--missing"]
EXTS = (".afreq", ".gcount", ".smiss", ".vmiss")
PRUNE = ["--indep-pairwise", "60kb", "0.3"]


def codes(seed=5):
    """(M, N) REF-based codes with what the reports' edge cases need; check_fixture() asserts it is all there"""
    rng = np.random.default_rng(seed)
    raw = T.synth_raw_codes(M, N, seed, missing_rate=0.0, ld_copy_prob=0.6, redraw=0.05).copy()
    raw[rng.random((M, N)) < 0.03] = 3
    for s in S_30PCT:
        raw[rng.random(M) < 0.3, s] = 3
    raw[:, S_COMPLETE] = np.where(raw[:, S_COMPLETE] == 3, 0, raw[:, S_COMPLETE])
    raw[V_COMPLETE, :] = np.where(raw[V_COMPLETE, :] == 3, 1, raw[V_COMPLETE, :])
    raw[V_MONO, :] = np.where(raw[V_MONO, :] == 3, 3, 0)
    raw[V_ALT_MAJOR, :] = np.where(np.arange(N) % 5 == 0, 1, 2)
    raw[V_ALL_MISSING, :] = 3
    return raw


def chrom_names():
    return ["0"] * CHR0 + ["1"] * 150 + ["2"] * (M - CHR0 - 150)


def check_fixture(raw):
    """the properties the tests rely on, asserted on the codes themselves"""
    miss_v = (raw == 3).sum(axis=1)
    miss_s = (raw == 3).sum(axis=0)
    assert raw.shape == (M, N)
    assert miss_v[V_COMPLETE] == 0                                  # a variant with no missing call
    assert ((miss_v > 0) & (miss_v < N)).any()                      # one with some
    assert miss_v[V_ALL_MISSING] == N and (miss_v == N).sum() == 1  # one with every call missing: the `nan` line
    called = raw[V_MONO][raw[V_MONO] != 3]
    assert called.size and (called == 0).all()                      # a monomorphic one
    alt = (raw[V_ALT_MAJOR] == 1).sum() + 2 * (raw[V_ALT_MAJOR] == 2).sum()
    ref = (raw[V_ALT_MAJOR] == 1).sum() + 2 * (raw[V_ALT_MAJOR] == 0).sum()
    assert alt > ref                                                # an ALT-major one
    assert chrom_names()[:CHR0] == ["0"] * CHR0 and CHR0 > 0        # chromosome-0 variants
    assert miss_s[S_COMPLETE] == 1 and raw[V_ALL_MISSING, S_COMPLETE] == 3   # a sample whose only missing call is the variant nobody has
    assert all(miss_s[s] > 0.2 * M for s in S_30PCT) and (miss_s > 0.1 * M).sum() == len(S_30PCT)
    hom_ref = (raw == 0).sum(axis=1)
    assert ((raw == 1).sum(axis=1) > 0).any() and (hom_ref > 0).any() and ((raw == 2).sum(axis=1) > 0).any()


def positions(seed=6):
    rng = np.random.default_rng(seed)
    pos = np.zeros(M, dtype=np.int64)
    start = 0
    for cnt in (CHR0, 150, M - CHR0 - 150):
        pos[start:start + cnt] = np.sort(rng.choice(np.arange(1000000, 1400000), size=cnt, replace=False))
        start += cnt
    return pos


def write_fileset(d, raw, nonfounders=()):
    """<d>/d as .bed and fixed-width .pgen and, written by the reference, <d>/v as variable-width .pgen; sub-directories ref / dev / host for the
    tools' outputs (FORMATS: ../d, ../v), so that both write the same <out> name into their log lines.  nonfounders: samples with parents"""
    prefix = os.path.join(str(d), "d")
    T.write_bed(prefix, raw, chrom_names(), positions())
    T.write_pgen_fixed(prefix, raw, chrom_names(), positions())
    if nonfounders:
        lines = open(prefix + ".fam").read().splitlines()
        for s in nonfounders:
            t = lines[s].split()
            t[2], t[3] = "s0", "s1"
            lines[s] = " ".join(t)
        open(prefix + ".fam", "w").write("\n".join(lines) + "\n")
        with open(prefix + ".psam", "w") as f:
            f.write("#IID\tPAT\tMAT\tSEX\n")
            for s in range(raw.shape[1]):
                f.write("s%d\t%s\t%s\t2\n" % (s, "s0" if s in nonfounders else "0", "s1" if s in nonfounders else "0"))
    mk = T.run_ref(["--pfile", "d", "--make-pgen", "--out", "v"], str(d))
    assert mk.returncode == 0, mk.stdout[-800:]
    for sub in ("ref", "dev", "host"):
        os.makedirs(os.path.join(str(d), sub), exist_ok=True)
    return prefix


def run_cli(cli, args, cwd):
    return subprocess.run([cli] + args, cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)


REPORT_LOG = ("--freq: Allele", "--freq counts: Allele", "--geno-counts: Genotype", "--missing: Sample", "--missing: Variant", "--geno: ", "removed due to allele frequency",
              "removed due to missing genotype data (--mind)")


def report_lines(log_path):
    """the reports' log lines and the filters' around them, in the order they were logged (from <out>.log: the reference's console output carries progress text)"""
    return [l.strip() for l in open(log_path).read().split("\n") if any(k in l for k in REPORT_LOG)]


def same_bytes(d, sub, tag, exts):
    """every <tag><ext> of sub-directory `sub` against the reference's, as bytes; the reference's must not be trivial"""
    for ext in exts:
        a, b = os.path.join(str(d), "ref", tag + ext), os.path.join(str(d), sub, tag + ext)
        assert os.path.getsize(a) > 10, a
        assert os.path.exists(b), b
        assert open(a, "rb").read() == open(b, "rb").read(), (sub, tag + ext)
