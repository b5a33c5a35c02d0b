"""Filesets and helpers of the --mind tests (test_cli_mind_args.py on the CPU, test_mind.py on the GPU)."""
import os

import numpy as np

import ldtools as T

M, N = 1000, 150
CHR0 = 5                     # the first variants lie on chromosome 0: they count for --mind, the prune ignores them
S_100, S_101 = 17, 64        # the samples with exactly 100 and exactly 101 missing calls
S_30PCT = (3, 77, 149)       # ... and with about 30 %
BLOCK = (200, 520)           # block=True: the planted samples' missing calls sit in these variants
FORMATS = {"bed": ["--bfile", "../d"], "pgen-fixed": ["--pfile", "../d"], "pgen-varwidth": ["--pfile", "../v"]}
PRUNE = ["--indep-pairwise", "60kb", "0.3"]
MIND_LINE = "removed due to missing genotype data (--mind)"


def planted_codes(block=False, seed=21):
    """(M, N) REF-based codes: 1 % background missingness, and on top one sample with exactly 100 missing calls (none of them on chromosome 0),
    one with exactly 101 (two of them on chromosome 0) and three with about 30 %.  With --mind 0.1 MindFilter's bound is
    (int32_t)(1000 x 0.1 x (1 + 2^-44)) = 100 over ALL 1,000 variants: the 101 sample and the three go, the 100 sample stays -- unless chromosome 0
    is left out of the numerator (the 101 sample would stay: 99 of 995) or of the denominator (the 100 sample would go: bound 99)."""
    rng = np.random.default_rng(seed)
    raw = T.synth_raw_codes(M, N, seed, missing_rate=0.0, ld_copy_prob=0.6, redraw=0.05).copy()
    raw[rng.random((M, N)) < 0.01] = 3
    lo, hi = BLOCK if block else (CHR0, M)
    for s, k, on_chr0 in ((S_100, 100, 0), (S_101, 101, 2)):
        raw[:, s] = np.where(raw[:, s] == 3, 0, raw[:, s])
        rows = np.concatenate([np.arange(on_chr0), rng.choice(np.arange(lo, hi), size=k - on_chr0, replace=False)])
        raw[rows, s] = 3
        assert int((raw[:, s] == 3).sum()) == k
    for s in S_30PCT:
        if block:
            raw[rng.choice(np.arange(lo, hi), size=300, replace=False), s] = 3
        else:
            raw[rng.random(M) < 0.3, s] = 3
        assert 250 <= int((raw[:, s] == 3).sum()) <= 350
    return raw


def positions(seed=21):
    """chromosome names and sorted positions of the M variants: chromosome 0 first, then 1, 2 and 5"""
    m = M
    names = ["0"] * CHR0 + ["1"] * 400 + ["2"] * 350 + ["5"] * (m - CHR0 - 750)
    rng = np.random.default_rng(seed + 1)
    pos = np.zeros(m, dtype=np.int64)
    start = 0
    for cnt in (CHR0, 400, 350, m - CHR0 - 750):
        pos[start:start + cnt] = np.sort(rng.choice(np.arange(3000000, 3400000), size=cnt, replace=False))
        start += cnt
    return names, pos


def write_fileset(d, raw, with_varwidth=True):
    """<d>/d as .bed and fixed-width .pgen (every sample a founder) and, written by the reference, <d>/v as variable-width .pgen; run the
    tools from sub-directories (FORMATS: ../d, ../v) so that both write the same <out> name into their log lines"""
    assert raw.shape[0] == M
    names, pos = positions()
    prefix = os.path.join(str(d), "d")
    T.write_bed(prefix, raw, names, pos)
    T.write_pgen_fixed(prefix, raw, names, pos)
    if with_varwidth:
        mk = T.run_ref(["--pfile", "d", "--make-pgen", "--out", "v"], str(d))
        assert mk.returncode == 0, mk.stdout[-800:]
    for sub in ("ref", "dev", "host"):
        os.makedirs(os.path.join(str(d), sub), exist_ok=True)
    return prefix


def expected_removed(raw, mind=0.1):
    """the samples MindFilter removes, from the codes (plink2_filter.cc:3340-3355)"""
    bound = int(raw.shape[0] * (mind * (1 + 2.0 ** -44)))
    return [s for s in range(raw.shape[1]) if int((raw[:, s] == 3).sum()) > bound]


def mind_lines(stdout):
    """the --mind log lines: the count and, when samples went, where their IDs were written"""
    return [l.strip() for l in stdout.split("\n") if (MIND_LINE in l) or (".mindrem.id" in l)]


def removed_due_to_lines(stdout):
    return [l.strip() for l in stdout.split("\n") if "removed due to" in l]


def read_mindrem(path):
    """IIDs of a .mindrem.id (header line dropped); None when the file does not exist"""
    if not os.path.exists(path):
        return None
    lines = open(path).read().split("\n")
    assert lines[0].startswith("#") and lines[-1] == ""
    return [l.split("\t")[-1] for l in lines[1:-1]]
