"""The KING-robust table in numpy, the yardstick of the king tests: the five integers per sample pair as matrix products of the indicator
vectors (int64 results; the products themselves run in float64, where they are exact), the kinship double (numpy's float64 division is the IEEE operation the reference's C division is), a formatter of the
.kin0 text written from the definition, and a fileset writer on ldtools.

raw: (variants, samples) uint8 REF-based codes, 0 hom-REF, 1 het, 2 hom-ALT, 3 missing.  In every matrix element [i, j] belongs to the pair
(sample i, sample j); the table lists the pairs j < i with i as the first sample of the line."""
import math
import os

import numpy as np

import ldtools as T
from phased_tools import format_g6 as _format_g6

FIELDS = ("hethet", "het_row_hom_col", "hom_row_het_col", "homhom", "ibs0")
COLSETS = ("maybefid", "fid", "id", "maybesid", "sid", "nsnp", "hethet", "ibs0", "ibs1", "ibs", "kinship")
DEFAULT_COLS = ("maybefid", "id", "maybesid", "nsnp", "hethet", "ibs0", "kinship")


def counts(raw, include=None):
    """dict of (samples, samples) int64 matrices: hethet = t_i.t_j, het_row_hom_col = t_i.h_j, hom_row_het_col = h_i.t_j, homhom = h_i.h_j,
    ibs0 = (h_i.h_j - x_i.x_j) / 2, over the rows of raw whose include entry is non-zero (None: all)"""
    raw = np.asarray(raw)
    if include is not None:
        raw = raw[np.asarray(include) != 0]
    assert raw.shape[0] < (1 << 52)
    # (the products run in float64, where sums of 0 / +-1 terms below 2^53 are exact integers, and come back as int64)
    t = (raw == 1).astype(np.float64).T
    h = ((raw == 0) | (raw == 2)).astype(np.float64).T
    x = (raw == 0).astype(np.float64).T - (raw == 2).astype(np.float64).T

    def dot(a, b):
        return np.rint(a @ b.T).astype(np.int64)

    hh = dot(h, h)
    xx = dot(x, x)
    assert not ((hh - xx) & 1).any()
    return {"hethet": dot(t, t), "het_row_hom_col": dot(t, h), "hom_row_het_col": dot(h, t), "homhom": hh, "ibs0": (hh - xx) // 2}


def nsnp(c):
    return c["hethet"] + c["het_row_hom_col"] + c["hom_row_het_col"] + c["homhom"]


def kinship(c):
    """0.5 - double(4 ibs0 + het_row_hom_col + hom_row_het_col) / double(4 (hethet + min(...))): -inf over 0, nan for 0 / 0"""
    num = (4 * c["ibs0"] + c["het_row_hom_col"] + c["hom_row_het_col"]).astype(np.float64)
    den = (4 * (c["hethet"] + np.minimum(c["het_row_hom_col"], c["hom_row_het_col"]))).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 0.5 - num / den


def block_struct(c, row_first, row_ct, col_first, col_ct, dtype):
    """what ldp_king_counts_block returns for the block: the pairs col < row, zero elsewhere"""
    out = np.zeros((row_ct, col_ct), dtype=dtype)
    rows = np.arange(row_first, row_first + row_ct)[:, None]
    cols = np.arange(col_first, col_first + col_ct)[None, :]
    below = cols < rows
    for f in FIELDS:
        out[f] = np.where(below, c[f][row_first:row_first + row_ct, col_first:col_first + col_ct], 0)
    return out


def hits(c, thr, row_first, row_ct, col_first, col_ct):
    """sorted list of (row, col, hethet, het_row_hom_col, hom_row_het_col, homhom, ibs0) of the block's pairs with not (kinship < thr)"""
    k = kinship(c)
    out = []
    for i in range(row_first, row_first + row_ct):
        for j in range(col_first, min(col_first + col_ct, i)):
            if not (k[i, j] < thr):
                out.append((i, j) + tuple(int(c[f][i, j]) for f in FIELDS))
    return out


def format_g6(x):
    if math.isinf(x):
        return "-inf" if x < 0 else "inf"
    return _format_g6(x)


def kin0_text(c, iids, cols=DEFAULT_COLS, report_counts=False, king_filter=None, fids=None, sids=None):
    """the .kin0 text and the number of filtered lines.  cols: column sets as --make-king-table cols= takes them; fids / sids: per-sample
    lists where the fileset has the column (maybefid / maybesid print it then; fid / sid print "0" without one)"""
    cols = set(cols)
    has_id = "id" in cols
    col_fid = has_id and (("fid" in cols) or (("maybefid" in cols) and fids is not None))
    col_sid = has_id and (("sid" in cols) or (("maybesid" in cols) and sids is not None))
    n = len(iids)

    def ident(s):
        parts = []
        if col_fid:
            parts.append(fids[s] if fids is not None else "0")
        parts.append(iids[s])
        if col_sid:
            parts.append(sids[s] if sids is not None else "0")
        return parts

    head = []
    if has_id:
        for k in ("1", "2"):
            head += (["FID" + k] if col_fid else []) + ["IID" + k] + (["SID" + k] if col_sid else [])
    for name, titles in (("nsnp", ["NSNP"]), ("hethet", ["HETHET"]), ("ibs0", ["IBS0"]), ("ibs1", ["HET1_HOM2", "HET2_HOM1"]), ("ibs", ["IBS"]), ("kinship", ["KINSHIP"])):
        if name in cols:
            head += titles
    lines = ["#" + "\t".join(head)]
    ns = nsnp(c)
    kin = kinship(c)
    filtered = 0
    for i in range(n):
        for j in range(i):
            k = float(kin[i, j])
            if (king_filter is not None) and (k < king_filter):
                filtered += 1
                continue
            f = ident(i) + ident(j) if has_id else []
            hethet, ibs0 = int(c["hethet"][i, j]), int(c["ibs0"][i, j])
            # the table's "1" is the line's SECOND sample (the earlier one): HET1_HOM2 = the earlier sample het, the later one hom
            het1hom2, het2hom1 = int(c["hom_row_het_col"][i, j]), int(c["het_row_hom_col"][i, j])
            nm = int(ns[i, j])
            with np.errstate(divide="ignore"):
                recip = float(np.float64(1.0) / np.float64(nm))

            def frac(v):
                with np.errstate(invalid="ignore"):
                    return format_g6(float(np.float64(recip) * np.float64(v)))

            if "nsnp" in cols:
                f.append(str(nm))
            if "hethet" in cols:
                f.append(str(hethet) if report_counts else frac(hethet))
            if "ibs0" in cols:
                f.append(str(ibs0) if report_counts else frac(ibs0))
            if "ibs1" in cols:
                f += [str(het1hom2), str(het2hom1)] if report_counts else [frac(het1hom2), frac(het2hom1)]
            if "ibs" in cols:
                ham = 2 * ibs0 + het1hom2 + het2hom1
                if report_counts:
                    f.append(str(ham))
                else:
                    with np.errstate(invalid="ignore"):
                        f.append(format_g6(float(np.float64(recip) * np.float64(0.5) * np.float64(ham))))
            if "kinship" in cols:
                f.append(format_g6(k))
            lines.append("\t".join(f))
    return "\n".join(lines) + "\n", filtered


def planted_codes(seed=20):
    """the planted fileset of the reference test: 70 samples x 300 variants (280 autosomal, 15 chrX, 5 MT), 4 % missing, a sample without any
    call, a sample without a het call, two identical samples, a variant nobody has a call at.  Returns (raw, chroms, bps)."""
    n, m = 70, 300
    raw = T.synth_raw_codes(m, n, seed=seed, missing_rate=0.04).copy()
    raw[:, 5] = 3                                # no call at all
    raw[:, 9] = np.where(raw[:, 9] == 1, 0, raw[:, 9])   # never het
    raw[:, 31] = raw[:, 30]                      # identical samples
    raw[100, :] = 3                              # a variant without a call
    chroms = ["1"] * 150 + ["2"] * 130 + ["X"] * 15 + ["MT"] * 5
    bps = [1000 + 100 * i for i in range(m)]
    return raw, chroms, bps


def autosomal(chroms):
    return np.array([c not in ("X", "Y", "XY", "MT", "23", "24", "25", "26") for c in chroms])


def write_fileset(prefix, raw, chroms, bps, fmt="pgen"):
    """fixed-width .pgen (+ .pvar / .psam) or .bed (+ .bim / .fam) through ldtools; returns the sample IDs"""
    if fmt == "bed":
        T.write_bed(prefix, raw, chroms, bps)
    else:
        T.write_pgen_fixed(prefix, raw, chroms, bps)
    return ["s%d" % s for s in range(raw.shape[1])]


def run_ref_king(cwd, file_args, extra=(), out="ref"):
    """the reference's --make-king-table on the fileset; returns (CompletedProcess, path prefix of its outputs)"""
    cp = T.run_ref(list(file_args) + ["--make-king-table"] + list(extra) + ["--out", out], cwd)
    return cp, os.path.join(cwd, out)


# ---------------------------------------------------------------- plink2-hip against the reference
KING_LOG = ("non-autosomes from KING", "--make-king-table:", "Results written to", "--king-table-filter:", "Error:", "removed due to", "KING-robust")


def king_lines(log_path):
    """the log lines of --make-king-table and of the filters in front of it, in the order they were logged (from <out>.log: the reference's
    console output carries progress text); the echo of the command line, which is indented, is left out, and so are the lines of --het: the
    reference makes the table in front of the prune and --het, plink2-hip behind them, on the engine the filters left"""
    return [l.rstrip() for l in open(log_path).read().split("\n") if l and (not l.startswith(" ")) and (not l.startswith("[timing]")) and (not l.startswith("--het:")) and any(k in l for k in KING_LOG)]


def read_table(path):
    import het_tools as H
    return H.read_het(path)


def assert_same_as_reference(d, sub, tag, zs=False, id_file=False):
    """<d>/<sub>/<tag>.kin0[.zst] (and .kin0.id) against the reference's in <d>/ref, byte for byte, and the king log lines"""
    ext = ".kin0.zst" if zs else ".kin0"
    want = read_table(os.path.join(str(d), "ref", tag + ext))
    path = os.path.join(str(d), sub, tag + ext)
    assert os.path.exists(path), path
    got = read_table(path)
    assert want.count(b"\n") >= 1
    if got != want:
        w, g = want.split(b"\n"), got.split(b"\n")
        bad = [(i, a, b) for i, (a, b) in enumerate(zip(w, g)) if a != b]
        raise AssertionError((sub, tag, len(w), len(g), bad[:5]))
    for name in ((tag + ".kin0.id",) if id_file else ()):
        assert open(os.path.join(str(d), "ref", name), "rb").read() == open(os.path.join(str(d), sub, name), "rb").read(), name
    assert os.path.exists(os.path.join(str(d), sub, tag + ".kin0.id")) == id_file
    want_log = king_lines(os.path.join(str(d), "ref", tag + ".log"))
    got_log = king_lines(os.path.join(str(d), sub, tag + ".log"))
    assert got_log == want_log, (sub, tag, want_log, got_log)
