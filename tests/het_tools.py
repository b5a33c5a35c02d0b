"""Filesets and helpers of the --het tests: test_cli_het_args.py and test_het_host.py on the CPU, test_het_device.py on the GPU.

The reference sums a sample's expected heterozygosity in doubles, per thread, so the last bits of its sums -- and, rarely, the sixth digit it
prints -- depend on its thread count.  A fileset is a fixture only where the reference writes the same bytes with --threads 1 and --threads 4
(reference_runs()); every test checks that itself before it compares plink2-hip's output with the reference's, line by line."""
import os
import subprocess

import numpy as np

import ldtools as T

M, N = 400, 120
V_MONO = (10, 200)            # monomorphic variants (every call REF)
V_ALL_MISSING = 11            # a variant nobody has a call at
S_ALL_MISSING = 5             # a sample that misses every call
FORMATS = {"bed": ["--bfile", "../d"], "pgen-fixed": ["--pfile", "../d"], "pgen-varwidth": ["--pfile", "../v"]}
PRUNE = ["--indep-pairwise", "60kb", "0.3"]
HET_LOG = ("--het", "skipped because", "--read-freq", "allele frequency estimates", "non-autosomes", "removed due to")


def codes(rate, seed=3, mono=V_MONO, all_missing_variant=True, all_missing_sample=True, m=M, n=N):
    """(m, n) REF-based codes: `rate` of the calls missing, and on top the planted variants and the planted sample"""
    rng = np.random.default_rng(seed)
    raw = T.synth_raw_codes(m, n, seed, missing_rate=0.0, ld_copy_prob=0.6, redraw=0.05, maf_lo=0.05).copy()
    if rate:
        raw[rng.random((m, n)) < rate] = 3
    for v in mono:
        raw[v, :] = np.where(raw[v, :] == 3, 3, 0)
    if all_missing_variant:
        raw[V_ALL_MISSING, :] = 3
    if all_missing_sample:
        raw[:, S_ALL_MISSING] = 3
    return raw


def chrom_names(m=M, x=0, mt=0):
    """two autosomes, then x variants on chrX and mt on MT"""
    a = m - x - mt
    return ["1"] * (a // 2) + ["2"] * (a - a // 2) + ["X"] * x + ["MT"] * mt


def positions(names, seed=6):
    rng = np.random.default_rng(seed)
    pos = np.zeros(len(names), dtype=np.int64)
    start = 0
    while start < len(names):
        end = start
        while end < len(names) and names[end] == names[start]:
            end += 1
        pos[start:end] = np.sort(rng.choice(np.arange(1000000, 1400000), size=end - start, replace=False))
        start = end
    return pos


def write_fileset(d, raw, names=None, nonfounders=(), varwidth=True, sexes=None):
    """<d>/d as .bed and fixed-width .pgen and, written by the reference, <d>/v as variable-width .pgen; sub-directories ref / ref1 / dev / host
    for the tools' outputs (FORMATS: ../d, ../v), so that all write the same <out> name into their log lines.  nonfounders: samples with parents"""
    names = chrom_names(raw.shape[0]) if names is None else names
    prefix = os.path.join(str(d), "d")
    T.write_bed(prefix, raw, names, positions(names))
    T.write_pgen_fixed(prefix, raw, names, positions(names), sexes=sexes)
    if sexes is not None:
        lines = [l.split() for l in open(prefix + ".fam").read().splitlines()]
        for s, t in enumerate(lines):
            t[4] = str(sexes[s])
        open(prefix + ".fam", "w").write("\n".join(" ".join(t) for t in lines) + "\n")
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
                f.write("s%d\t%s\t%s\t%s\n" % (s, "s0" if s in nonfounders else "0", "s1" if s in nonfounders else "0", "2" if sexes is None else str(sexes[s])))
    if varwidth:
        mk = T.run_ref(["--pfile", "d", "--make-pgen", "--out", "v"], str(d))
        assert mk.returncode == 0, mk.stdout[-800:]
    make_dirs(d)
    return prefix


def make_dirs(d):
    for sub in ("ref", "ref1", "dev", "host"):
        os.makedirs(os.path.join(str(d), sub), exist_ok=True)


def write_multiallelic_fileset(d, m=300, n=90, seed=4, nonfounders=()):
    """<d>/v: a variable-width .pgen imported by the reference from a VCF whose variants have 1-3 ALT alleles (a third of them several), with
    missing calls, altx/alty hets, one variant with a single allele observed and one nobody has a call at"""
    first, second, alt_ct = T.synth_multiallelic_haps(m, n, seed, max_alt=3, multi_rate=0.35, missing_rate=0.03)
    multi = np.flatnonzero(alt_ct > 1)
    assert len(multi) > 20 and (alt_ct == 3).any() and (alt_ct == 2).any()
    assert ((first > 0) & (second > 0) & (first != second)).any(), "no altx/alty het"
    first[multi[0]] = np.where(first[multi[0]] < 0, -1, 2)      # one allele alone (an ALT one) among the calls
    second[multi[0]] = np.where(second[multi[0]] < 0, -1, 2)
    first[multi[1]] = -1                                         # every call missing
    second[multi[1]] = -1
    names = chrom_names(m)
    vcf = os.path.join(str(d), "m.vcf")
    T.write_vcf_haps(vcf, first, second, alt_ct, names, positions(names), unphased=np.ones((m, n), dtype=bool))
    T.ref_import_vcf(vcf, os.path.join(str(d), "v"))
    if nonfounders:
        lines = open(os.path.join(str(d), "v.psam")).read().splitlines()
        out = ["#IID\tPAT\tMAT\tSEX"]
        for s, l in enumerate(lines[1:]):
            iid = l.split("\t")[0]
            out.append("%s\t%s\t%s\tNA" % (iid, "s0" if s in nonfounders else "0", "s1" if s in nonfounders else "0"))
        open(os.path.join(str(d), "v.psam"), "w").write("\n".join(out) + "\n")
    make_dirs(d)
    return first, second, alt_ct


def run_cli(cli, args, cwd):
    return subprocess.run([cli] + args, cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)


def het_lines(log_path):
    """the log lines of --het and of the filters in front of it, in the order they were logged (from <out>.log: the reference's console output
    carries progress text); the echo of the command line, which is indented, is left out"""
    return [l.rstrip() for l in open(log_path).read().split("\n") if l and (not l.startswith(" ")) and (not l.startswith("[timing]")) and any(k in l for k in HET_LOG)]


def read_het(path):
    if path.endswith(".zst"):
        return subprocess.run([T.REF_BIN, "--zst-decompress", os.path.basename(path)], cwd=os.path.dirname(path), stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                              check=True, timeout=120).stdout
    return open(path, "rb").read()


def reference_runs(d, args, tag, zs=False):
    """the reference with --threads 4 (<d>/ref) and --threads 1 (<d>/ref1); returns (the --threads 4 run, whether the fileset qualifies: both
    runs end alike and write the same .het bytes)"""
    ref = T.run_ref(args + ["--threads", "4", "--out", tag], os.path.join(str(d), "ref"))
    ref1 = T.run_ref(args + ["--threads", "1", "--out", tag], os.path.join(str(d), "ref1"))
    ext = ".het.zst" if zs else ".het"
    a, b = os.path.join(str(d), "ref", tag + ext), os.path.join(str(d), "ref1", tag + ext)
    same = (ref.returncode == ref1.returncode) and (os.path.exists(a) == os.path.exists(b))
    if same and os.path.exists(a):
        same = read_het(a) == read_het(b)
    return ref, same


def assert_same_as_reference(d, sub, tag, zs=False):
    """<d>/<sub>/<tag>.het[.zst] against the reference's, line by line (every line must match), and the --het log lines"""
    ext = ".het.zst" if zs else ".het"
    want = read_het(os.path.join(str(d), "ref", tag + ext)).split(b"\n")
    path = os.path.join(str(d), sub, tag + ext)
    assert os.path.exists(path), path
    got = read_het(path).split(b"\n")
    assert len(want) > 3
    bad = [(i, w, g) for i, (w, g) in enumerate(zip(want, got)) if w != g]
    assert not bad and len(got) == len(want), (sub, tag, len(want), len(got), bad[:5])
    want_log = het_lines(os.path.join(str(d), "ref", tag + ".log"))
    got_log = het_lines(os.path.join(str(d), sub, tag + ".log"))
    assert got_log == want_log, (sub, tag, want_log, got_log)
