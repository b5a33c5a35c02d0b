"""The exact Hardy-Weinberg test in integers, the triple sets and the filesets of the --hwe / --hardy tests: test_hwe_exact_host.py,
test_cli_hwe_args.py and test_hwe_host.py on the CPU, test_hwe_device.py and test_hwe_cli_device.py on the GPU.

The statistic: counts (hom1, het, hom2), n = hom1 + het + hom2, rare = 2 min(hom1, hom2) + het.  Conditional on n and rare the het count k
(of rare's parity, 0 <= k <= rare) has weight w(k) = 2^k n! / (r! k! c!), r = (rare - k) / 2, c = n - k - r, and
p = sum{w(k): w(k) <= w(het)} / sum w(k); `midp` takes half of every w(k) == w(het) off the numerator.  Here every w(k) is an integer (the
multinomial coefficient times 2^k), so the comparisons and the ties are exact, and ln p is taken of a ratio of two integers with 50 digits."""
import json
import os
import subprocess
from decimal import Decimal, getcontext
from math import comb

import numpy as np

import ldtools as T

getcontext().prec = 60
_LN2 = Decimal(2).ln()
GOLDEN_LARGE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hwe_large.json")


def weights(hom1, het, hom2):
    """[(k, w(k))] over every het count of the variant's n and rare, w(k) exact integers up to one common factor, and the observed one's index"""
    n = hom1 + het + hom2
    r0 = min(hom1, hom2)
    rare = 2 * r0 + het
    k = rare & 1
    r = (rare - k) // 2
    c = n - k - r
    # the true w(k_min): from an integer, every step's division by (k + 2)(k + 1) is exact
    w = comb(n, r) * comb(n - r, k) * (1 << k)
    out = []
    while True:
        out.append((k, w))
        if r == 0:
            break
        num, den = 4 * r * c, (k + 2) * (k + 1)
        w, rem = divmod(w * num, den)
        assert rem == 0
        k, r, c = k + 2, r - 1, c - 1
    obs = (het - (rare & 1)) // 2
    assert out[obs][0] == het
    return out, obs


def ln_int(x):
    """ln of a positive integer to ~55 digits (its leading 256 bits decide)"""
    sh = max(0, x.bit_length() - 256)
    return (Decimal(x >> sh)).ln() + sh * _LN2


def exact_ln_p(hom1, het, hom2, midp=False):
    """(ln p as a Decimal, whether a het count other than het - 2, het, het + 2 ties with the observed one exactly)"""
    ws, obs = weights(hom1, het, hom2)
    w_obs = ws[obs][1]
    tail = sum(w for _, w in ws if w <= w_obs)
    ties = sum(w for _, w in ws if w == w_obs)
    total = sum(w for _, w in ws)
    far_tie = any((w == w_obs) and (abs(i - obs) > 1) for i, (_, w) in enumerate(ws))
    if midp:
        num, den = 2 * tail - ties, 2 * total
    else:
        num, den = tail, total
    return ln_int(num) - ln_int(den), far_tie


def bound(n, ln_p):
    """|computed - exact| may be at most this: n / 2 recurrence steps of 4 roundings each, two positive sums, a quotient and a log"""
    return (4 * n + 64) * 2.0 ** -52 + 4 * abs(float(ln_p)) * 2.0 ** -52


def small_triples(n_max=32):
    return [(a, b, n - a - b) for n in range(n_max + 1) for a in range(n + 1) for b in range(n + 1 - a)]


def random_triples(count, n_mid, seed):
    """seeded Hardy-Weinberg draws at about n_mid samples over MAF 0.02-0.5; a third with het calls turned homozygous (deficit), a third
    with homozygous calls turned het (excess), either allele the rarer one"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        n = int(rng.integers(n_mid * 7 // 8, n_mid * 9 // 8 + 1))
        q = float(rng.uniform(0.02, 0.5))
        a, b, c = (int(x) for x in rng.multinomial(n, [(1 - q) ** 2, 2 * q * (1 - q), q * q]))
        kind = i % 3
        if kind == 1:
            mv = int(b * rng.uniform(0.05, 0.5))
            b -= mv
            a += mv - mv // 2
            c += mv // 2
        elif kind == 2:
            mv = int(min(a, c + 1) * rng.uniform(0.05, 0.5))
            ma, mc = mv, min(c, mv)
            a -= ma
            c -= mc
            b += ma + mc
        if rng.random() < 0.5:
            a, c = c, a
        assert a + b + c == n and min(a, b, c) >= 0
        out.append((a, b, c))
    return out


def golden_large():
    """[(hom1, het, hom2, ln p, ln p with midp, far tie)], the ln p as Decimals (tests/golden/make_golden_hwe.py)"""
    rows = json.load(open(GOLDEN_LARGE))["triples"]
    return [(r["hom1"], r["het"], r["hom2"], Decimal(r["ln_p"]), Decimal(r["ln_p_midp"]), bool(r["far_tie"])) for r in rows]


_ORACLE_CACHE = {}


def oracle_set(name):
    """the shared, computed-once expectation of a triple set: [(hom1, het, hom2, {False: (ln p, far tie), True: ...})]"""
    if name in _ORACLE_CACHE:
        return _ORACLE_CACHE[name]
    if name == "small":
        triples = small_triples(32)
    elif name == "n400":
        triples = random_triples(300, 400, 11)
    elif name == "n3000":
        triples = random_triples(60, 3000, 12)
    elif name == "golden":
        out = [(a, b, c, {False: (lp, ft), True: (lpm, ft)}) for a, b, c, lp, lpm, ft in golden_large()]
        _ORACLE_CACHE[name] = out
        return out
    else:
        raise KeyError(name)
    out = [(a, b, c, {m: exact_ln_p(a, b, c, m) for m in (False, True)}) for a, b, c in triples]
    _ORACLE_CACHE[name] = out
    return out


def check_against_oracle(name, midp, got_ln_p, got_flags):
    """every entry within the bound, flag bit 0 clear where the oracle finds no tie beyond the observed table's neighbours"""
    want = oracle_set(name)
    assert len(got_ln_p) == len(want) == len(got_flags)
    worst = 0.0
    bad = []
    for i, (a, b, c, exp) in enumerate(want):
        lp, far_tie = exp[bool(midp)]
        err = abs(Decimal(float(got_ln_p[i])) - lp) if np.isfinite(got_ln_p[i]) else Decimal("Infinity")
        lim = bound(a + b + c, lp)
        worst = max(worst, float(err) / lim)
        if (not err <= Decimal(lim)) or ((int(got_flags[i]) & 1) and not far_tie) or (int(got_flags[i]) & ~1):
            bad.append(((a, b, c), float(got_ln_p[i]), str(lp)[:30], float(err), lim, int(got_flags[i]), far_tie))
    print("%s midp=%d: %d triples, worst error %.4f of the bound" % (name, int(bool(midp)), len(want), worst))
    assert not bad, (name, midp, len(bad), bad[:5])


# ---- filesets ----
V_ALL_HET, V_ALL_MISSING, V_MONO, V_HALF, V_THIN = 7, 11, 10, 13, 17   # the planted variants of planted_codes()
FORMATS = {"bed": ["--bfile", "../d"], "pgen-fixed": ["--pfile", "../d"], "pgen-varwidth": ["--pfile", "../v"]}
PRUNE = ["--indep-pairwise", "60kb", "0.3"]
SETTINGS = (["1e-3"], ["1e-3", "0", "midp"], ["0.05", "0.001"], ["1e-2", "0.01", "midp", "keep-fewhet"], ["1e-10", "0", "keep-fewhet"], ["0.3"],
            ["1e-300", "0"], ["1e-400", "0"])
HWE_LOG = ("--hwe", "--hardy", "--geno", "removed due to", "observation counts vary")


def planted_codes(m, n, seed, missing_rate=0.02, plant=True):
    """(m, n) REF-based codes: variants 0 mod 4 with a share of their het calls turned homozygous (het deficit), variants 1 mod 4 with a share of
    their homozygous calls turned het (excess), `missing_rate` of the calls missing, and on top one all-het variant, one nobody has a call at,
    one monomorphic, one with half REF and half ALT homozygotes and one that a fifth of the samples have no call at"""
    rng = np.random.default_rng(seed)
    raw = T.synth_raw_codes(m, n, seed, missing_rate=0.0, ld_copy_prob=0.5, redraw=0.05, maf_lo=0.05).copy()
    for v in range(m):
        share = rng.uniform(0.1, 0.6)
        pick = rng.random(n) < share
        if v % 4 == 0:
            hets = pick & (raw[v] == 1)
            raw[v, hets] = np.where(rng.random(int(hets.sum())) < 0.5, 0, 2)
        elif v % 4 == 1:
            raw[v, pick & (raw[v] != 1)] = 1
    if missing_rate:
        raw[rng.random((m, n)) < missing_rate] = 3
    if plant:
        raw[V_ALL_HET, :] = 1
        raw[V_ALL_MISSING, :] = 3
        raw[V_MONO, :] = np.where(raw[V_MONO, :] == 3, 3, 0)
        raw[V_HALF, : n // 2] = 0
        raw[V_HALF, n // 2:] = 2
        raw[V_THIN, : n // 5] = 3
    return raw


def genotype_counts(raw):
    """(hom REF, het, hom ALT) per variant"""
    return tuple((raw == c).sum(axis=1).astype(np.uint32) for c in (0, 1, 2))


def chrom_names(m):
    return ["1"] * (m // 2) + ["2"] * (m - m // 2)


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


def make_dirs(d, subs=("ref", "dev", "host")):
    for sub in subs:
        os.makedirs(os.path.join(str(d), sub), exist_ok=True)


def write_fileset(d, raw, names=None, varwidth=True, bed_only=False):
    """<d>/d as .bed and fixed-width .pgen and, written by the reference, <d>/v as variable-width .pgen; sub-directories ref / dev / host for
    the tools' outputs (FORMATS: ../d, ../v), so that all write the same <out> name into their log lines"""
    names = chrom_names(raw.shape[0]) if names is None else names
    prefix = os.path.join(str(d), "d")
    T.write_bed(prefix, raw, names, positions(names))
    if not bed_only:
        T.write_pgen_fixed(prefix, raw, names, positions(names))
        if varwidth:
            mk = T.run_ref(["--pfile", "d", "--make-pgen", "--out", "v"], str(d))
            assert mk.returncode == 0, mk.stdout[-800:]
    make_dirs(d)
    return prefix


def run_cli(cli, args, cwd):
    return subprocess.run([cli] + args, cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)


def log_lines(log_path):
    """the log lines of --hwe / --hardy and of the filters around them, in the order they were logged, re-joined across the word wrap; the echo of
    the command line (indented) and the timing lines are left out"""
    text = open(log_path).read()
    keep, on = [], False
    for l in text.split("\n"):
        if l.startswith(" ") or l.startswith("[timing]") or l.startswith("Options in effect") or l.startswith("Start time") or l.startswith("End time"):
            on = False
            continue
        start = any(l.startswith(k) for k in ("--hwe", "--hardy", "--geno", "Warning: --hwe", "Error: --hwe", "If you are performing", "Alternatively, if")) or \
            ("removed due to allele frequency" in l)
        if start:
            keep.append(l.rstrip())
            on = True
        elif on and l and not l.startswith("--") and not l[0].isdigit() and not l.startswith("Error") and not l.startswith("Warning"):
            keep[-1] += "\n" + l.rstrip()   # a wrapped line's continuation
        else:
            on = False
    return keep


def read_text(path):
    if path.endswith(".zst"):
        return subprocess.run([T.REF_BIN, "--zst-decompress", os.path.basename(path)], cwd=os.path.dirname(path), stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                              check=True, timeout=120).stdout
    return open(path, "rb").read()


def _round6(x):
    from decimal import Context, ROUND_HALF_EVEN
    return Context(prec=6, rounding=ROUND_HALF_EVEN).plus(x)


def near_rounding_boundary(p):
    """whether the exact p lies within a relative 1e-9 of a boundary between two 6-digit decimals"""
    if p == 0:
        return False
    t = p.scaleb(5 - p.adjusted())          # in [1e5, 1e6)
    frac = t - int(t)
    return abs(frac - Decimal("0.5")) <= Decimal("1e-9") * t


def qualify_hardy(ref_bytes, midp, exact=None):
    """The conditions fixed in advance for the byte comparison of a .hardy file.  Returns the set of line numbers whose exact p lies within 1e-9
    (relative) of a 6-digit rounding boundary -- at most 1 % of the file: there every field but P is compared -- after asserting that on every
    other line the reference's own P is the exact value rounded to 6 digits.  (Decimal's exponent range is wide enough for p = 1e-150000.)"""
    lines = ref_bytes.decode().split("\n")
    assert lines[0].startswith("#CHROM") and lines[-1] == ""
    loose = set()
    for i, l in enumerate(lines[1:-1], start=1):
        t = l.split("\t")
        a, b, c = int(t[4]), int(t[5]), int(t[6])
        lp = exact(a, b, c, midp) if exact else exact_ln_p(a, b, c, midp)[0]
        p = lp.exp()
        if near_rounding_boundary(p):
            loose.add(i)
            continue
        assert Decimal(t[9]) == _round6(p), ("the reference's own P is not the exact value", l, str(p)[:20])
    assert len(loose) * 100 <= len(lines) - 2, (len(loose), len(lines))
    return loose


def assert_same_hardy(d, sub, tag, midp=False, zs=False, exact=None):
    """<d>/<sub>/<tag>.hardy[.zst] against the reference's, byte for byte (P apart on the lines qualify_hardy() names), and the log lines"""
    ext = ".hardy.zst" if zs else ".hardy"
    want = read_text(os.path.join(str(d), "ref", tag + ext))
    path = os.path.join(str(d), sub, tag + ext)
    assert os.path.exists(path), path
    got = read_text(path)
    loose = qualify_hardy(want, midp, exact)   # (exact: ln p of a triple from elsewhere, where the evaluation here would take minutes)
    wl, gl = want.split(b"\n"), got.split(b"\n")
    assert len(wl) == len(gl) and len(wl) > 3, (len(wl), len(gl))
    bad = []
    for i, (w, g) in enumerate(zip(wl, gl)):
        if i in loose:
            w, g = w.rsplit(b"\t", 1)[0], g.rsplit(b"\t", 1)[0]
        if w != g:
            bad.append((i, w, g))
    assert not bad, (sub, tag, len(bad), bad[:5])
    assert_same_log(d, sub, tag)


def assert_same_log(d, sub, tag):
    want_log = log_lines(os.path.join(str(d), "ref", tag + ".log"))
    got_log = log_lines(os.path.join(str(d), sub, tag + ".log"))
    assert want_log and got_log == want_log, (sub, tag, want_log, got_log)


def assert_same_het_counts(d, sub, tag):
    """the integer columns of <tag>.het (O(HOM) and OBS_CT per sample) against the reference's: they are sums over exactly the variants the
    filters left, so they show every decision; the float columns, whose last digit depends on the reference's thread count, are left to the
    --het tests"""
    def cols(path):
        rows = [l.split("\t") for l in open(path).read().split("\n") if l]
        k = rows[0].index("O(HOM)")
        return [(r[:k], r[k], r[k + 2]) for r in rows]
    want, got = cols(os.path.join(str(d), "ref", tag + ".het")), cols(os.path.join(str(d), sub, tag + ".het"))
    assert len(want) > 3 and got == want, (sub, tag, [(w, g) for w, g in zip(want, got) if w != g][:5])


def threshold_ln(setting, n):
    """ln of the threshold a variant with n calls is held to under `--hwe <setting>`: ln(thr) (1 + 2^-44) + n k (-ln 10)"""
    nums = [s for s in setting if s not in ("midp", "keep-fewhet")]
    mant, _, ex = nums[0].lower().partition("e")
    ln_thr = Decimal(mant).ln() + (Decimal(int(ex)) * Decimal(10).ln() if ex else 0)
    k = Decimal(nums[1]) if len(nums) > 1 else Decimal(0)
    return ln_thr * (1 + Decimal(2) ** -44) - n * k * Decimal(10).ln()


def expected_removals(raw, setting, tested=None):
    """per variant: removed by `--hwe <setting>` by the rule in exact arithmetic -- after asserting that no tested variant's exact ln p lies
    within 1e-5 of its threshold (the reference promises float32-level agreement there, no more)"""
    midp, fewhet = "midp" in setting, "keep-fewhet" in setting
    a, b, c = genotype_counts(raw)
    out = np.zeros(raw.shape[0], dtype=bool)
    for v in range(raw.shape[0]):
        if tested is not None and not tested[v]:
            continue
        n = int(a[v]) + int(b[v]) + int(c[v])
        if n == 0 or (fewhet and int(b[v]) ** 2 <= 4 * int(a[v]) * int(c[v])):
            continue
        lp, _ = exact_ln_p(int(a[v]), int(b[v]), int(c[v]), midp)
        thr = threshold_ln(setting, n)
        assert abs(lp - thr) > Decimal("1e-5"), ("a variant sits on its threshold: choose another seed", v, setting, str(lp)[:20])
        out[v] = lp < thr
    return out
