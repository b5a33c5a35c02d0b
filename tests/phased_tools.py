"""Test-side helpers for --r2-phased / --r-phased: the five integers of a pair by brute force from raw codes (numpy), the phase-code
rows of the second engine, the reference binary's table and its number format.

TEST INFRASTRUCTURE ONLY -- the product (plink-ng_amd/) never imports this module."""
import math
import os

import numpy as np

import ldtools as T

STATS_FIELDS = ("valid_obs", "sum0", "sum1", "known_dotprod", "unknown_hethet")


def alt_major(raw):
    """per variant: ALT is the major allele (the reference's choice: allele frequencies over the called samples, REF on a tie)"""
    return T.oracle_prepare(raw)[2].astype(bool)


def phase_rows(present, info):
    """The second engine's rows (include/ldprune_hip.h: ldp_r2_phased_stats_block): per sample 0 = phased het with phaseinfo 0,
    2 = phased het with phaseinfo 1, 1 = anything else; (M, N) uint8 codes for ldtools.pack_2bit."""
    present = np.asarray(present, dtype=bool)
    info = np.asarray(info, dtype=bool)
    return np.where(present, np.where(info, 2, 0), 1).astype(np.uint8)


def brute_dense(raw, present=None, info=None, altmaj=None):
    """ldp_phased_stats_t of every pair i < j as an (M, M) array [j, i] (zero elsewhere), straight from the definitions
    (ComputeR2NondosagePhasedStats, plink2_ld.cc:6545-6588; HardcallPhasedR2Refine :3238-3262), sample by sample, no identity used.
    Without phase (present is None) the counted allele is the non-major one (PgrGetInv1); with phase it is the major one and a
    sample's phaseinfo says 'the counted allele is on the first haplotype' (PgrGetInv1P, pgenlib_read.cc:7016-7042)."""
    raw = np.asarray(raw)
    m = raw.shape[0]
    altmaj = alt_major(raw) if altmaj is None else np.asarray(altmaj, dtype=bool)
    called = raw != 3
    alt_ct = np.where(called, raw, 0).astype(np.int64)
    ref_ct = np.where(called, 2 - raw.astype(np.int64), 0)
    with_phase = present is not None
    # counted allele per variant: ALT when (ALT is major) == with_phase
    count_alt = altmaj if with_phase else ~altmaj
    g = np.where(count_alt[:, None], alt_ct, ref_ct)
    if with_phase:
        present = np.asarray(present, dtype=bool) & (raw == 1)
        # the file's bit says 'ALT first'; where REF is counted the reference complements it
        pinfo = np.where(count_alt[:, None], np.asarray(info, dtype=bool), ~np.asarray(info, dtype=bool))
    known_of = np.zeros((3, 3), dtype=np.int64)
    known_of[2, 2], known_of[2, 1], known_of[1, 2] = 2, 1, 1
    out = np.zeros((m, m), dtype=[(f, "<u4") for f in STATS_FIELDS])
    for j in range(1, m):
        v = called[:j] & called[j]
        gi, gj = g[:j], np.broadcast_to(g[j], (j, raw.shape[1]))
        known = (known_of[gi, gj] * v).sum(axis=1)
        unknown = (v & (gi == 1) & (gj == 1)).sum(axis=1)
        if with_phase:
            both = v & present[:j] & present[j]
            known = known + (both & (pinfo[:j] == pinfo[j])).sum(axis=1)
            unknown = unknown - both.sum(axis=1)
        out["valid_obs"][j, :j] = v.sum(axis=1)
        out["sum0"][j, :j] = (gi * v).sum(axis=1)
        out["sum1"][j, :j] = (gj * v).sum(axis=1)
        out["known_dotprod"][j, :j] = known
        out["unknown_hethet"][j, :j] = unknown
    return out


def brute_stats(raw, first, second, present=None, info=None, altmaj=None):
    """the same for the pairs (first[k], second[k])"""
    return brute_dense(raw, present, info, altmaj)[np.asarray(second, dtype=np.int64), np.asarray(first, dtype=np.int64)]


def all_pairs(m):
    """(first, second) of every pair i < j, ordered by first then second (the .vcor table's order)"""
    i, j = np.triu_indices(m, 1)
    return i.astype(np.uint32), j.astype(np.uint32)


# ---------------------------------------------------------------- the reference's number format
def _banker_round(v):
    t = int(v)
    return t + int((v - t) + (0.500000005 if (t & 1) else 0.499999995))


def _digits(u, digits):
    return ("%0*d" % (digits, u)).rstrip("0") or "0"


def format_g6(x):
    """six significant digits the way the reference's table prints a double (dtoa_g, include/plink2_string.cc:2507-2639), for the
    magnitudes these statistics take (|x| < 1e6)"""
    if x != x:
        return "nan"
    sign = ""
    if x < 0:
        sign, x = "-", -x
    if x == 0.0:
        return sign + "0"
    assert 1e-31 < x < 1e6, "magnitudes these statistics do not take"
    if x < 9.9999949999999e-5:
        xp = 0
        for bound, up, e in ((9.9999949999999e-16, 1.0e16, 16), (9.9999949999999e-8, 100000000.0, 8), (9.9999949999999e-4, 10000.0, 4), (9.9999949999999e-2, 100.0, 2),
                             (9.9999949999999e-1, 10.0, 1)):
            if x < bound:
                x *= up
                xp += e
        t = _banker_round(x * 100000)
        s = "%d" % (t // 100000)
        if t % 100000:
            s += "." + _digits(t % 100000, 5)
        return sign + s + "e-%02d" % xp
    if x >= 0.99999949999999:
        int_digits = 1
        for b in (9.9999949999999, 99.999949999999, 999.99949999999, 9999.9949999999, 99999.949999999):
            if x >= b:
                int_digits += 1
        scale = 10 ** (6 - int_digits)
        t = _banker_round(x * scale)
        q, r = divmod(t, scale)
        s = "%d" % q
        if r:
            s += "." + _digits(r, 6 - int_digits)
        return sign + s
    s = "0."
    if x < 9.9999949999999e-3:
        x *= 100
        s += "00"
    if x < 9.9999949999999e-2:
        x *= 10
        s += "0"
    return sign + s + _digits(_banker_round(x * 1000000), 6)


def table_fields(r2, d, dprime, is_neg, signed, abs_dprime=False):
    """the three value columns of a table line: PHASED_R2 / PHASED_R, D, DPRIME / ABS_DPRIME"""
    v = r2
    if signed:
        v = math.sqrt(r2)
        if is_neg:
            v = -v
    return [format_g6(v), format_g6(d), format_g6(abs(dprime) if abs_dprime else dprime)]


def ref_table(cwd, file_args, flag, extra=(), out="ref"):
    """run the reference; returns {(ID_A, ID_B): [value columns as text]} and the header's value column names"""
    cp = T.run_ref(list(file_args) + [flag] + list(extra) + ["--out", out], cwd)
    if cp.returncode != 0:
        raise RuntimeError("reference plink2 failed:\n" + cp.stdout)
    with open(os.path.join(cwd, out + ".vcor")) as f:
        lines = [ln.rstrip("\n").split("\t") for ln in f]
    hdr = lines[0]
    ia, ib = hdr.index("ID_A"), hdr.index("ID_B")
    iv = [k for k, name in enumerate(hdr) if name.startswith("PHASED_R")][0]
    return {(ln[ia], ln[ib]): ln[iv:] for ln in lines[1:]}, hdr[iv:]
