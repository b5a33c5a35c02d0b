"""Test-side helpers: ctypes binding of the CPU oracle (oracle/ldoracle.c), genotype packing,
PLINK file writers and a runner for the reference binary (oracle/_ref/plink2, when present).

TEST INFRASTRUCTURE ONLY -- the product (plink-ng_amd/) never imports this module.
"""
import ctypes
import os
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(REPO, "oracle")
ORACLE_SO = os.path.join(ORACLE_DIR, "_build", "libldoracle.so")
REF_BIN = os.path.join(ORACLE_DIR, "_ref", "plink2")

K_SMALL_EPSILON = 2.0 ** -44


class LdoVaggs(ctypes.Structure):
    _fields_ = [("nm_ct", ctypes.c_uint32), ("sum", ctypes.c_int32), ("ssq", ctypes.c_uint32),
                ("plusone_ct", ctypes.c_uint32), ("minusone_ct", ctypes.c_uint32)]


class LdoPairStats(ctypes.Structure):
    _fields_ = [("nm", ctypes.c_uint32), ("sum1", ctypes.c_int32), ("ssq1", ctypes.c_uint32),
                ("sum2", ctypes.c_int32), ("ssq2", ctypes.c_uint32), ("dot", ctypes.c_int32)]

    def astuple(self):
        return (self.nm, self.sum1, self.ssq1, self.sum2, self.ssq2, self.dot)


class LdoVhaggs(ctypes.Structure):
    _fields_ = [("nm_ct", ctypes.c_uint32), ("sum", ctypes.c_uint32)]


class LdoHapPairStats(ctypes.Structure):
    _fields_ = [("nm", ctypes.c_uint32), ("sum1", ctypes.c_uint32), ("sum2", ctypes.c_uint32), ("dot", ctypes.c_uint32)]

    def astuple(self):
        return (self.nm, self.sum1, self.sum2, self.dot)


def build_oracle():
    if (not os.path.exists(ORACLE_SO)) or os.path.getmtime(ORACLE_SO) < max(
            os.path.getmtime(os.path.join(ORACLE_DIR, f)) for f in ("ldoracle.c", "ldoracle.h")):
        subprocess.check_call(["make", "-C", ORACLE_DIR, "oracle"], stdout=subprocess.DEVNULL)
    return ORACLE_SO


_oracle = None


def oracle():
    global _oracle
    if _oracle is None:
        lib = ctypes.CDLL(build_oracle())
        u64p = ctypes.POINTER(ctypes.c_uint64)
        u32p = ctypes.POINTER(ctypes.c_uint32)
        f64p = ctypes.POINTER(ctypes.c_double)
        lib.ldo_split_hom_ref2het.argtypes = [u64p, ctypes.c_uint32, u64p, u64p]
        lib.ldo_fill_vaggs.argtypes = [u64p, u64p, ctypes.c_uint32, ctypes.POINTER(LdoVaggs)]
        lib.ldo_is_monomorphic.argtypes = [ctypes.POINTER(LdoVaggs)]
        lib.ldo_pair_stats.argtypes = [u64p, u64p, ctypes.POINTER(LdoVaggs), u64p, u64p, ctypes.POINTER(LdoVaggs),
                                       ctypes.c_uint32, ctypes.POINTER(LdoPairStats)]
        lib.ldo_exceeds.argtypes = [ctypes.POINTER(LdoPairStats), ctypes.c_double]
        lib.ldo_cov_vars.argtypes = [ctypes.POINTER(LdoPairStats), f64p, f64p, f64p]
        lib.ldo_prune_thresh.argtypes = [ctypes.c_double]
        lib.ldo_prune_thresh.restype = ctypes.c_double
        lib.ldo_major_allele.argtypes = [u64p, ctypes.c_uint32, u32p, f64p]
        lib.ldo_invert_geno.argtypes = [u64p, ctypes.c_uint32, u64p]
        lib.ldo_subcontig_split.argtypes = [u32p, u32p, ctypes.c_uint32, ctypes.c_uint32, u32p, u32p]
        lib.ldo_subcontig_split.restype = ctypes.c_uint32
        lib.ldo_indep_pairwise.argtypes = [u64p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, u32p, u32p, f64p,
                                           ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_double,
                                           ctypes.c_int, u64p, u64p]
        lib.ldo_indep_pairwise.restype = ctypes.c_int
        lib.ldo_hapsplit_must_phased.argtypes = [u64p, u64p, u64p, ctypes.c_uint32, u64p, u64p]
        lib.ldo_hapsplit_must_phased.restype = ctypes.c_int
        lib.ldo_hapsplit_haploid.argtypes = [u64p, ctypes.c_uint32, u64p, u64p]
        lib.ldo_fill_vhaggs.argtypes = [u64p, u64p, ctypes.c_uint32, ctypes.POINTER(LdoVhaggs)]
        lib.ldo_fill_vhaggs.restype = ctypes.c_int
        lib.ldo_hap_pair_stats.argtypes = [u64p, u64p, ctypes.POINTER(LdoVhaggs), u64p, u64p, ctypes.POINTER(LdoVhaggs),
                                           ctypes.c_uint32, ctypes.POINTER(LdoHapPairStats)]
        lib.ldo_hap_exceeds.argtypes = [ctypes.POINTER(LdoHapPairStats), ctypes.c_double]
        lib.ldo_indep_pairphase.argtypes = lib.ldo_indep_pairwise.argtypes
        lib.ldo_indep_pairphase.restype = ctypes.c_int
        _oracle = lib
    return _oracle


def _p(arr, ctype):
    return arr.ctypes.data_as(ctypes.POINTER(ctype))


# ---------------------------------------------------------------- genotype packing
def pack_2bit(codes):
    """codes: (M, N) uint8 array of 2-bit codes -> (M, stride_words) uint64, 32 genotypes per word,
    little-endian bit order (sample s -> bits 2*(s%32) of word s//32).  Trailing bits are zero."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    m, n = codes.shape
    stride_words = (n + 31) // 32
    padded = np.zeros((m, stride_words * 32), dtype=np.uint8)
    padded[:, :n] = codes & 3
    quads = padded.reshape(m, stride_words * 8, 4)
    bytes_ = (quads[:, :, 0] | (quads[:, :, 1] << 2) | (quads[:, :, 2] << 4) | (quads[:, :, 3] << 6)).astype(np.uint8)
    return np.ascontiguousarray(bytes_).view(np.uint64).reshape(m, stride_words)


def unpack_2bit(words, n):
    m = words.shape[0]
    b = np.ascontiguousarray(words).view(np.uint8).reshape(m, -1)
    out = np.empty((m, b.shape[1] * 4), dtype=np.uint8)
    for k in range(4):
        out[:, k::4] = (b >> (2 * k)) & 3
    return out[:, :n]


def bitmap_to_bool(bm, n):
    return np.unpackbits(np.ascontiguousarray(bm).view(np.uint8), bitorder="little")[:n].astype(bool)


# ---------------------------------------------------------------- oracle wrappers
def oracle_prepare(raw_codes):
    """raw REF-based codes (0 hom-REF,1 het,2 hom-ALT,3 missing), (M,N) -> (inv packed words, maj_freq, alt_major)"""
    lib = oracle()
    raw = pack_2bit(raw_codes)
    m, n = raw_codes.shape
    inv = np.empty_like(raw)
    mf = np.empty(m, dtype=np.float64)
    altmaj = np.empty(m, dtype=np.uint32)
    for v in range(m):
        am = ctypes.c_uint32()
        f = ctypes.c_double()
        lib.ldo_major_allele(_p(raw[v], ctypes.c_uint64), n, ctypes.byref(am), ctypes.byref(f))
        mf[v] = f.value
        altmaj[v] = am.value
        if am.value:
            lib.ldo_invert_geno(_p(raw[v], ctypes.c_uint64), n, _p(inv[v], ctypes.c_uint64))
        else:
            inv[v] = raw[v]
    return inv, mf, altmaj


def oracle_split(inv_words, n):
    """(M, stride) packed inverse codes -> hom, r2h planes (M, ceil(n/64)) uint64 + list of vaggs"""
    lib = oracle()
    m = inv_words.shape[0]
    wc = (n + 63) // 64
    gw = (n + 31) // 32
    hom = np.zeros((m, wc), dtype=np.uint64)
    r2h = np.zeros((m, wc), dtype=np.uint64)
    vaggs = (LdoVaggs * m)()
    for v in range(m):
        row = np.zeros(gw + 1, dtype=np.uint64)
        row[:gw] = inv_words[v, :gw]
        lib.ldo_split_hom_ref2het(_p(row, ctypes.c_uint64), n, _p(hom[v], ctypes.c_uint64), _p(r2h[v], ctypes.c_uint64))
        lib.ldo_fill_vaggs(_p(hom[v], ctypes.c_uint64), _p(r2h[v], ctypes.c_uint64), wc, ctypes.byref(vaggs[v]))
    return hom, r2h, vaggs


def oracle_pair_stats(hom, r2h, vaggs, n, first, second):
    lib = oracle()
    st = LdoPairStats()
    lib.ldo_pair_stats(_p(hom[first], ctypes.c_uint64), _p(r2h[first], ctypes.c_uint64), ctypes.byref(vaggs[first]),
                       _p(hom[second], ctypes.c_uint64), _p(r2h[second], ctypes.c_uint64), ctypes.byref(vaggs[second]),
                       n, ctypes.byref(st))
    return st


def oracle_r2(st):
    lib = oracle()
    c, v1, v2 = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    lib.ldo_cov_vars(ctypes.byref(st), ctypes.byref(c), ctypes.byref(v1), ctypes.byref(v2))
    return c.value, v1.value, v2.value


def oracle_indep_pairwise(inv_words, n, chr_idx, bps, maj_freqs, window, step, is_bp, r2, order=2):
    """Returns (removed bool array, pair evaluation count)."""
    lib = oracle()
    m = inv_words.shape[0]
    inv_words = np.ascontiguousarray(inv_words, dtype=np.uint64)
    chr_idx = np.ascontiguousarray(chr_idx, dtype=np.uint32)
    bps = np.ascontiguousarray(bps, dtype=np.uint32)
    maj_freqs = np.ascontiguousarray(maj_freqs, dtype=np.float64)
    removed = np.zeros((m + 63) // 64 + 1, dtype=np.uint64)
    evals = ctypes.c_uint64()
    rc = lib.ldo_indep_pairwise(_p(inv_words, ctypes.c_uint64), inv_words.shape[1], m, n, _p(chr_idx, ctypes.c_uint32),
                                _p(bps, ctypes.c_uint32), _p(maj_freqs, ctypes.c_double), window, step, int(is_bp),
                                r2, int(order == 1), _p(removed, ctypes.c_uint64), ctypes.byref(evals))
    assert rc == 0
    return bitmap_to_bool(removed, m), evals.value


def pack_bits(bits):
    """(M, N) 0/1 array -> (M, ceil(N/64)) uint64, sample s -> bit s%64 of word s//64"""
    bits = np.ascontiguousarray(bits, dtype=np.uint8)
    m, n = bits.shape
    wc = (n + 63) // 64
    padded = np.zeros((m, wc * 64), dtype=np.uint8)
    padded[:, :n] = bits & 1
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view(np.uint64).reshape(m, wc)


def oracle_hapsplit(raw_codes, phasepresent, phaseinfo, haploid=False):
    """REF-based codes (M, N) + per-sample phase bits (0/1 arrays, phaseinfo 1 = ALT on the first haplotype) ->
    (hap_nm rows (M, 2*wc) uint64 in the major-allele-inverse coding the pruner sees, maj_freq, unphased flags, hap_ct).
    Mirrors what the reference's loader hands to IndepPairphaseThread (plink2_ld.cc:2040-2052): PgrGetInv1P
    output through HapsplitMustPhased / HapsplitHaploid."""
    lib = oracle()
    m, n = raw_codes.shape
    inv, mf, altmaj = oracle_prepare(raw_codes)
    hap_ct = n if haploid else 2 * n
    wc = (hap_ct + 63) // 64
    rows = np.zeros((m, 2 * wc), dtype=np.uint64)
    unphased = np.zeros(m, dtype=bool)
    pp = pack_bits(phasepresent)
    gw = (n + 31) // 32
    for v in range(m):
        g = np.zeros(gw + 2, dtype=np.uint64)
        g[:gw] = inv[v, :gw]
        if haploid:
            lib.ldo_hapsplit_haploid(_p(g, ctypes.c_uint64), n, _p(rows[v, :wc], ctypes.c_uint64), _p(rows[v, wc:], ctypes.c_uint64))
            continue
        # inverting the counted allele swaps which haplotype carries it (IMPLPgrGetInv1P, pgenlib_read.cc:7016)
        info = phaseinfo[v:v + 1] ^ 1 if altmaj[v] else phaseinfo[v:v + 1]
        pi = pack_bits(info & phasepresent[v:v + 1])
        hap = np.zeros(gw + 1, dtype=np.uint64)
        nm = np.zeros(gw + 1, dtype=np.uint64)
        ppv = np.zeros(pp.shape[1] + 1, dtype=np.uint64)
        ppv[:pp.shape[1]] = pp[v]
        piv = np.zeros(pp.shape[1] + 1, dtype=np.uint64)
        piv[:pp.shape[1]] = pi[0]
        unphased[v] = bool(lib.ldo_hapsplit_must_phased(_p(g, ctypes.c_uint64), _p(ppv, ctypes.c_uint64), _p(piv, ctypes.c_uint64), n,
                                                        _p(hap, ctypes.c_uint64), _p(nm, ctypes.c_uint64)))
        rows[v, :wc] = hap[:wc]
        rows[v, wc:] = nm[:wc]
    return rows, mf, unphased, hap_ct


def oracle_hap_pair_stats(rows, hap_ct, first, second):
    lib = oracle()
    wc = (hap_ct + 63) // 64
    vh = [LdoVhaggs(), LdoVhaggs()]
    for k, v in enumerate((first, second)):
        lib.ldo_fill_vhaggs(_p(rows[v, :wc], ctypes.c_uint64), _p(rows[v, wc:], ctypes.c_uint64), wc, ctypes.byref(vh[k]))
    st = LdoHapPairStats()
    lib.ldo_hap_pair_stats(_p(rows[first, :wc], ctypes.c_uint64), _p(rows[first, wc:], ctypes.c_uint64), ctypes.byref(vh[0]),
                           _p(rows[second, :wc], ctypes.c_uint64), _p(rows[second, wc:], ctypes.c_uint64), ctypes.byref(vh[1]),
                           hap_ct, ctypes.byref(st))
    return st


def oracle_indep_pairphase(hap_nm_rows, hap_ct, chr_idx, bps, maj_freqs, window, step, is_bp, r2, order=2):
    """Returns (removed bool array, pair evaluation count)."""
    lib = oracle()
    m = hap_nm_rows.shape[0]
    rows = np.ascontiguousarray(hap_nm_rows, dtype=np.uint64)
    chr_idx = np.ascontiguousarray(chr_idx, dtype=np.uint32)
    bps = np.ascontiguousarray(bps, dtype=np.uint32)
    maj_freqs = np.ascontiguousarray(maj_freqs, dtype=np.float64)
    removed = np.zeros((m + 63) // 64 + 1, dtype=np.uint64)
    evals = ctypes.c_uint64()
    rc = lib.ldo_indep_pairphase(_p(rows, ctypes.c_uint64), rows.shape[1], m, hap_ct, _p(chr_idx, ctypes.c_uint32),
                                 _p(bps, ctypes.c_uint32), _p(maj_freqs, ctypes.c_double), window, step, int(is_bp),
                                 r2, int(order == 1), _p(removed, ctypes.c_uint64), ctypes.byref(evals))
    assert rc == 0
    return bitmap_to_bool(removed, m), evals.value


def oracle_subcontig_split(chr_idx, bps, window):
    lib = oracle()
    chr_idx = np.ascontiguousarray(chr_idx, dtype=np.uint32)
    m = len(chr_idx)
    info = np.zeros(2 * max(m, 1), dtype=np.uint32)
    wmax = ctypes.c_uint32()
    bp_ptr = None
    if bps is not None:
        bps = np.ascontiguousarray(bps, dtype=np.uint32)
        bp_ptr = _p(bps, ctypes.c_uint32)
    ct = lib.ldo_subcontig_split(_p(chr_idx, ctypes.c_uint32), bp_ptr, m, window, _p(info, ctypes.c_uint32), ctypes.byref(wmax))
    return [(int(info[2 * k]), int(info[2 * k + 1])) for k in range(ct)], wmax.value


# ---------------------------------------------------------------- synthetic data (numpy; small sizes)
def synth_raw_codes(m, n, seed, missing_rate=0.0, ld_copy_prob=0.5, redraw=0.05, maf_lo=0.01):
    """REF-based codes with planted LD between consecutive variants (same spirit as the reference's
    --dummy generator, plink2_import.cc:16387-16432)."""
    rng = np.random.default_rng(seed)
    out = np.empty((m, n), dtype=np.uint8)
    prev = None
    for v in range(m):
        maf = rng.uniform(maf_lo, 0.5)
        if rng.random() < 0.5:
            maf = 1.0 - maf  # ALT may be the major allele
        fresh = (rng.random(n) < maf).astype(np.uint8) + (rng.random(n) < maf).astype(np.uint8)
        if prev is not None and rng.random() < ld_copy_prob:
            keep = rng.random(n) >= redraw
            cur = np.where(keep, prev, fresh)
        else:
            cur = fresh
        prev = cur.copy()
        if missing_rate > 0:
            cur = np.where(rng.random(n) < missing_rate, 3, cur).astype(np.uint8)
        out[v] = cur
    return out


# ---------------------------------------------------------------- PLINK file writers / reference runner
def write_pgen_fixed(prefix, raw_codes, chroms, bps, ids=None, sexes=None):
    """Fixed-width .pgen (storage mode 0x02: pgenlib_read.cc:881-911) + .pvar + .psam."""
    m, n = raw_codes.shape
    rec = (n + 3) // 4
    packed = pack_2bit(raw_codes).view(np.uint8).reshape(m, -1)[:, :rec]
    with open(prefix + ".pgen", "wb") as f:
        f.write(bytes([0x6C, 0x1B, 0x02]))
        f.write(np.uint32(m).tobytes())
        f.write(np.uint32(n).tobytes())
        f.write(bytes([0x40]))
        f.write(np.ascontiguousarray(packed).tobytes())
    if ids is None:
        ids = ["snp%d" % i for i in range(m)]
    with open(prefix + ".pvar", "w") as f:
        f.write("#CHROM\tPOS\tID\tREF\tALT\n")
        for i in range(m):
            f.write("%s\t%d\t%s\tA\tC\n" % (chroms[i], bps[i], ids[i]))
    with open(prefix + ".psam", "w") as f:
        f.write("#IID\tSEX\n")
        for s in range(n):
            f.write("s%d\t%s\n" % (s, "2" if sexes is None else str(sexes[s])))
    return ids


def phased_pgen_records(raw_codes, phaseinfo):
    """Variable-width .pgen records with the hardcall-phase track (pgen_spec.tex:541-562), every het phased: record =
    raw 2-bit main track (type 0) + aux track 2 = 1 + H bits (bit 0 clear: no explicit phasepresent; then the H
    phaseinfo bits of the het calls in sample order).  Returns (list of record bytes, vrtype array)."""
    m, n = raw_codes.shape
    rec = (n + 3) // 4
    packed = pack_2bit(raw_codes).view(np.uint8).reshape(m, -1)[:, :rec]
    records = []
    vrtypes = np.zeros(m, dtype=np.uint8)
    for v in range(m):
        het = np.flatnonzero(raw_codes[v] == 1)
        body = packed[v].tobytes()
        if len(het):
            bits = np.zeros(1 + len(het), dtype=np.uint8)
            bits[1:] = phaseinfo[v, het] & 1
            body += np.packbits(bits, bitorder="little").tobytes()
            vrtypes[v] = 0x10
        records.append(body)
    return records, vrtypes


def write_pgen_phased(prefix, raw_codes, phaseinfo, chroms, bps, ids=None, sexes=None, parents=None):
    """Standard variable-width .pgen (storage mode 0x10, 8-bit record types, 3-byte record lengths;
    pgen_spec.tex:160-235) whose records carry the hardcall-phase track, + .pvar + .psam."""
    records, vrtypes = phased_pgen_records(raw_codes, phaseinfo)
    return write_pgen_records(prefix, records, vrtypes, raw_codes.shape[1], chroms, bps, ids, sexes, parents)


def write_pgen_records(prefix, records, vrtypes, n, chroms, bps, ids=None, sexes=None, parents=None):
    """... from ready-made record bytes and their 8-bit record types."""
    m = len(records)
    vrtypes = np.asarray(vrtypes, dtype=np.uint8)
    blocks = (m + 65535) // 65536
    header_len = 12 + 8 * blocks + sum(min(65536, m - b * 65536) * 4 for b in range(blocks))
    with open(prefix + ".pgen", "wb") as f:
        f.write(bytes([0x6C, 0x1B, 0x10]))
        f.write(np.uint32(m).tobytes())
        f.write(np.uint32(n).tobytes())
        f.write(bytes([0x40 | 6]))
        off = header_len
        for b in range(blocks):
            f.write(np.uint64(off).tobytes())
            off += sum(len(r) for r in records[b * 65536:(b + 1) * 65536])
        for b in range(blocks):
            lo, hi = b * 65536, min(m, (b + 1) * 65536)
            f.write(vrtypes[lo:hi].tobytes())
            for r in records[lo:hi]:
                f.write(len(r).to_bytes(3, "little"))
        for r in records:
            f.write(r)
    if ids is None:
        ids = ["snp%d" % i for i in range(m)]
    with open(prefix + ".pvar", "w") as f:
        f.write("#CHROM\tPOS\tID\tREF\tALT\n")
        for i in range(m):
            f.write("%s\t%d\t%s\tA\tC\n" % (chroms[i], bps[i], ids[i]))
    with open(prefix + ".psam", "w") as f:
        f.write("#IID\tPAT\tMAT\tSEX\n")
        for s in range(n):
            pat, mat = parents[s] if parents is not None else ("0", "0")
            f.write("s%d\t%s\t%s\t%s\n" % (s, pat, mat, "NA" if (sexes is None or sexes[s] == 0) else str(sexes[s])))
    return ids


def write_bed(prefix, raw_codes, chroms, bps, ids=None):
    """PLINK 1 .bed/.bim/.fam (pgen_spec.tex:425-428: 00 hom-A1(ALT) 01 missing 10 het 11 hom-A2(REF))."""
    m, n = raw_codes.shape
    lut = np.array([3, 2, 0, 1], dtype=np.uint8)  # pgen code -> bed code
    rec = (n + 3) // 4
    packed = pack_2bit(lut[raw_codes]).view(np.uint8).reshape(m, -1)[:, :rec]
    with open(prefix + ".bed", "wb") as f:
        f.write(bytes([0x6C, 0x1B, 0x01]))
        f.write(np.ascontiguousarray(packed).tobytes())
    if ids is None:
        ids = ["snp%d" % i for i in range(m)]
    with open(prefix + ".bim", "w") as f:
        for i in range(m):
            f.write("%s\t%s\t0\t%d\tC\tA\n" % (chroms[i], ids[i], bps[i]))
    with open(prefix + ".fam", "w") as f:
        for s in range(n):
            f.write("s%d s%d 0 0 2 -9\n" % (s, s))
    return ids


def synth_phase(raw_codes, seed, unphased_rate=0.0):
    """Random phase for every het call: (phasepresent, phaseinfo) 0/1 arrays; phaseinfo 1 = "1|0"."""
    rng = np.random.default_rng(seed)
    het = (raw_codes == 1)
    present = het & (rng.random(raw_codes.shape) >= unphased_rate)
    info = present & (rng.random(raw_codes.shape) < 0.5)
    return present.astype(np.uint8), info.astype(np.uint8)


def synth_phased(m, n, seed, missing_rate=0.0, ld_copy_prob=0.5, redraw=0.05, maf_lo=0.01):
    """Phased data with LD planted between consecutive variants on the haplotype level: returns (raw REF-based codes
    (M, N), phasepresent, phaseinfo); every het is phased, phaseinfo 1 = ALT on the first haplotype ("1|0")."""
    rng = np.random.default_rng(seed)
    raw = np.empty((m, n), dtype=np.uint8)
    info = np.zeros((m, n), dtype=np.uint8)
    prev = None
    for v in range(m):
        maf = rng.uniform(maf_lo, 0.5)
        if rng.random() < 0.5:
            maf = 1.0 - maf
        fresh = (rng.random((2, n)) < maf).astype(np.uint8)
        if prev is not None and rng.random() < ld_copy_prob:
            cur = np.where(rng.random((2, n)) >= redraw, prev, fresh)
        else:
            cur = fresh
        prev = cur.copy()
        code = (cur[0] + cur[1]).astype(np.uint8)
        info[v] = ((code == 1) & (cur[0] == 1)).astype(np.uint8)
        if missing_rate > 0:
            code = np.where(rng.random(n) < missing_rate, 3, code).astype(np.uint8)
        raw[v] = code
    present = (raw == 1).astype(np.uint8)
    return raw, present, info & present


def write_vcf(path, raw_codes, chroms, bps, phasepresent=None, phaseinfo=None, ids=None):
    """VCF 4.2 with GT only; phased hets written 0|1 / 1|0, everything else with '/'."""
    m, n = raw_codes.shape
    if ids is None:
        ids = ["snp%d" % i for i in range(m)]
    table = {0: "0/0", 1: "0/1", 2: "1/1", 3: "./."}
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.2\n")
        for c in sorted(set(chroms), key=lambda x: (len(x), x)):
            f.write("##contig=<ID=%s>\n" % c)
        f.write('##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n')
        f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("s%d" % s for s in range(n)) + "\n")
        for v in range(m):
            gts = []
            for s in range(n):
                c = int(raw_codes[v, s])
                if c == 1 and phasepresent is not None and phasepresent[v, s]:
                    gts.append("1|0" if phaseinfo[v, s] else "0|1")
                else:
                    gts.append(table[c])
            f.write("%s\t%d\t%s\tA\tC\t.\t.\t.\tGT\t%s\n" % (chroms[v], bps[v], ids[v], "\t".join(gts)))
    return ids


def synth_multiallelic_haps(m, n, seed, max_alt=3, multi_rate=0.3, missing_rate=0.02, ld_copy_prob=0.5, redraw=0.08):
    """Phased multiallelic data: (first, second) haplotype allele indices (M, N) int arrays (-1 = missing call),
    alt_ct per variant.  LD planted by copying the previous variant's haplotypes (allele indices clipped)."""
    rng = np.random.default_rng(seed)
    first = np.zeros((m, n), dtype=np.int16)
    second = np.zeros((m, n), dtype=np.int16)
    alt_ct = np.where(rng.random(m) < multi_rate, rng.integers(2, max_alt + 1, size=m), 1)
    prev = None
    for v in range(m):
        k = int(alt_ct[v]) + 1
        w = rng.dirichlet(np.ones(k) * rng.uniform(0.3, 2.0))
        fresh = rng.choice(k, size=(2, n), p=w)
        if prev is not None and rng.random() < ld_copy_prob:
            cur = np.where(rng.random((2, n)) >= redraw, np.minimum(prev, k - 1), fresh)
        else:
            cur = fresh
        prev = cur.copy()
        miss = rng.random(n) < missing_rate
        first[v] = np.where(miss, -1, cur[0])
        second[v] = np.where(miss, -1, cur[1])
    return first, second, alt_ct


def write_vcf_haps(path, first, second, alt_ct, chroms, bps, ids=None, unphased=None):
    """VCF with phased GTs a|b from haplotype allele indices (-1 = ./.); unphased (optional bool (M, N)): write a/b"""
    m, n = first.shape
    if ids is None:
        ids = ["snp%d" % i for i in range(m)]
    alts = ["C", "G", "T", "AC", "AG", "AT", "CA", "CC", "CG", "CT"]
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.2\n")
        for c in sorted(set(chroms), key=lambda x: (len(x), x)):
            f.write("##contig=<ID=%s>\n" % c)
        f.write('##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n')
        f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("s%d" % s for s in range(n)) + "\n")
        for v in range(m):
            gts = []
            for s in range(n):
                a, b = int(first[v, s]), int(second[v, s])
                if a < 0:
                    gts.append("./.")
                elif unphased is not None and unphased[v, s]:
                    gts.append("%d/%d" % (min(a, b), max(a, b)))
                else:
                    gts.append("%d|%d" % (a, b))
            f.write("%s\t%d\t%s\tA\t%s\t.\t.\t.\tGT\t%s\n" % (chroms[v], bps[v], ids[v], ",".join(alts[:int(alt_ct[v])]), "\t".join(gts)))
    return ids


def major_allele_multi(cnt):
    """Allele counts of one variant -> (major allele index, its frequency) the way the reference picks them
    (ComputeAlleleFreqs plink2_filter.cc:2113-2153, GetMajIdxMulti plink2_common.cc:1042-1070, GetAlleleFreq
    plink2_common.h:584-593): frequencies of all alleles but the last are count * (1/total)."""
    k = len(cnt)
    tot = int(np.sum(cnt))
    if tot == 0:
        freq = [1.0 / k] * (k - 1)
    else:
        recip = 1.0 / tot
        freq = [float(cnt[a]) * recip for a in range(k - 1)]
    if freq[0] >= 0.5:
        maj = 0
    elif k == 2:
        maj = 1
    elif freq[1] >= 0.5:
        maj = 1
    else:
        maj, mx = 1, freq[1]
        if freq[0] >= freq[1]:
            maj, mx = 0, freq[0]
        tot_nonlast = freq[0] + freq[1]
        for a in range(2, k - 1):
            if freq[a] > mx:
                maj, mx = a, freq[a]
            tot_nonlast += freq[a]
        if mx + tot_nonlast < 1.0 - K_SMALL_EPSILON:
            maj = k - 1
    if maj + 1 < k:
        return maj, freq[maj]
    last = 1.0 - freq[0]
    for a in range(1, k - 1):
        last -= freq[a]
    return maj, max(last, 0.0)


def pairphase_hap_rows_multiallelic(lo, hi, phasepresent, phaseinfo, alt_ct, quirk=True):
    """What PgrGetInv1P -> HapsplitMustPhased hand to the pairphase scan for possibly multiallelic variants, from allele
    pairs (lo <= hi, 255 missing) and the file's phase bits (phaseinfo 1 = the higher allele on the first haplotype):
    (hap_nm rows for oracle_indep_pairphase, maj_freq, unphased flags).  quirk=True reproduces the reference, whose
    Get1MP (pgenlib_read.cc:6962) passes phaseinfo through unchanged, i.e. reads it as "the counted allele is on the
    first haplotype" even when the major allele is the LOWER allele of a multiallelic het."""
    m, n = lo.shape
    codes = np.full((m, 2 * n), 3, dtype=np.uint8)
    mf = np.zeros(m)
    unphased = np.zeros(m, dtype=bool)
    for v in range(m):
        k = int(alt_ct[v]) + 1
        nm = lo[v] != 255
        cnt = [int((lo[v][nm] == a).sum() + (hi[v][nm] == a).sum()) for a in range(k)]
        maj, mf[v] = major_allele_multi(cnt)
        a, b = lo[v].astype(int), hi[v].astype(int)
        sw = phaseinfo[v].astype(bool)
        first = np.where(sw, b, a)
        second = np.where(sw, a, b)
        if quirk and maj >= 1:
            flip = (a == maj) & (b != maj)
            first, second = np.where(flip, second, first), np.where(flip, first, second)
        codes[v, 1::2] = np.where(nm, np.where(first != maj, 2, 0), 3)
        codes[v, 0::2] = np.where(nm, np.where(second != maj, 2, 0), 3)
        unphased[v] = bool((nm & ((a == maj) != (b == maj)) & ~phasepresent[v].astype(bool)).any())
    rows = np.concatenate([pack_bits((codes == 2).astype(np.uint8)), pack_bits((codes != 3).astype(np.uint8))], axis=1)
    return rows, mf, unphased


def _haploid_style_freqs(codes_subset):
    """diploid-style counts over the given samples: (ALT-is-major flags, major allele frequencies), a*(1/t) arithmetic"""
    cnt = np.stack([(codes_subset == k).sum(1) for k in range(3)], 1).astype(np.int64)
    refc = 2 * cnt[:, 0] + cnt[:, 1]
    tot = refc + 2 * cnt[:, 2] + cnt[:, 1]
    ref_freq = np.where(tot > 0, refc * (1.0 / np.maximum(tot, 1)), 0.5)
    altmaj = ~(ref_freq >= 0.5)
    return altmaj, np.where(altmaj, np.maximum(1.0 - ref_freq, 0.0), ref_freq)


def sex_chromosome_rows(raw, founder, sex, kind, phaseinfo=None):
    """What the reference's loaders hand to the scan on chrX / chrY / MT, as 2-bit codes of 'virtual samples' + the major
    allele frequencies (LoadAlleleAndGenoCountsThread, plink2_data.cc:2421-2700):
      kind "Y": non-female founders, hets -> missing;  "MT": every founder, hets -> missing  (haploid);
      kind "X", --indep-pairwise (phaseinfo None): male founders (hets -> missing) followed by the non-male founders
        TWICE (their statistics count double, plink2_ld.cc:890-901,1066-1082);
      kind "X", --indep-pairphase (phaseinfo given): male founders one haplotype each (hets missing), non-male founders
        two haplotypes split by phase (plink2_ld.cc:2060-2097); a haplotype h is the code 2h.
    raw: REF-based codes (M, N); founder: bool (N,); sex: 1 male / 2 female / 0 unknown."""
    founder = np.asarray(founder, dtype=bool)
    sex = np.asarray(sex)
    if kind in ("Y", "MT"):
        smp = np.where(founder & ((sex != 2) if kind == "Y" else True))[0]
        rs = raw[:, smp]
        _, mf = _haploid_style_freqs(rs)
        return np.where(rs == 1, 3, rs).astype(np.uint8), mf
    males = np.where(founder & (sex == 1))[0]
    non = np.where(founder & (sex != 1))[0]
    rm, rn = raw[:, males], raw[:, non]
    g = np.stack([(raw[:, founder] == k).sum(1) for k in range(3)], 1).astype(np.int64)
    mm = np.stack([(rm == k).sum(1) for k in range(3)], 1).astype(np.int64)
    alt = 4 * g[:, 2] + 2 * g[:, 1] - 2 * mm[:, 2] - mm[:, 1]  # plink2_data.cc:2641
    tot = 2 * (2 * g.sum(1) - mm.sum(1))
    ref_freq = np.where(tot > 0, (tot - alt) * (1.0 / np.maximum(tot, 1)), 0.5)
    altmaj = ~(ref_freq >= 0.5)
    mf = np.where(altmaj, np.maximum(1.0 - ref_freq, 0.0), ref_freq)
    hm = np.where(rm == 1, 3, rm)
    if phaseinfo is None:
        return np.concatenate([hm, rn, rn], axis=1).astype(np.uint8), mf
    pin = phaseinfo[:, non]
    ha = np.where(rn == 3, 3, np.where((rn == 2) | ((rn == 1) & (pin == 1)), 2, 0))
    hb = np.where(rn == 3, 3, np.where((rn == 2) | ((rn == 1) & (pin == 0)), 2, 0))
    return np.concatenate([hm, np.stack([ha, hb], 2).reshape(raw.shape[0], -1)], axis=1).astype(np.uint8), mf


def haploid_codes_to_hap_rows(codes):
    """codes in {0, 2, 3} (haplotype h as 2h, 3 missing) -> hap_nm rows for oracle_indep_pairphase"""
    return np.concatenate([pack_bits((codes == 2).astype(np.uint8)), pack_bits((codes != 3).astype(np.uint8))], axis=1)


def ref_import_vcf(vcf_path, prefix, extra=()):
    """reference: --vcf -> variable-width .pgen (with the hardcall-phase track when the VCF has phased hets)"""
    cp = run_ref(["--vcf", os.path.basename(vcf_path), "--make-pgen", "--out", os.path.basename(prefix)] + list(extra), os.path.dirname(prefix))
    if cp.returncode != 0:
        raise RuntimeError("reference plink2 --vcf failed:\n" + cp.stdout)
    return cp.stdout


def ref_pairphase_chrx_is_unreliable(sexes, founder_mask):
    """The reference's --indep-pairphase chrX loader ORs the male remainder word into a word it never initialised
    when 2 x (non-male founders) is a multiple of 64 and the male founder count is not (plink2_ld.cc:2087-2091:
    word_idx is then one past what HapsplitMustPhased wrote) -- its output then depends on stale memory (observed:
    --threads 1..8 vs 64 vs the default give three different prune lists on the same input).  Comparisons against the
    reference have to stay clear of that sample layout."""
    sexes = np.asarray(sexes)
    founder_mask = np.asarray(founder_mask, dtype=bool)
    males = int(((sexes == 1) & founder_mask).sum())
    nonmales = int(founder_mask.sum()) - males
    return (males % 64 != 0) and ((2 * nonmales) % 64 == 0)


def have_ref():
    return os.path.exists(REF_BIN) and os.access(REF_BIN, os.X_OK)


def run_ref(args, cwd, timeout=600):
    """Run the reference binary; returns CompletedProcess (stdout+stderr captured as text)."""
    return subprocess.run([REF_BIN] + list(args), cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                          text=True, timeout=timeout)


def read_id_list(path):
    with open(path) as f:
        return [ln.rstrip("\n") for ln in f if ln.strip()]


def ref_indep_pairwise(prefix, window_args, r2, order=2, threads=2, bad_ld=True, fmt="pfile", extra=(), mode="wise"):
    """Run reference --indep-pairwise (mode="phase": --indep-pairphase) on <prefix>; returns (kept ids, removed ids, log text)."""
    cwd = os.path.dirname(prefix)
    out = prefix + ".ref"
    args = ["--" + fmt, os.path.basename(prefix), "--indep-pair" + mode] + [str(a) for a in window_args] + [repr(float(r2))]
    if order == 1:
        args += ["--indep-order", "1"]
    if bad_ld:
        args += ["--bad-ld"]
    args += ["--threads", str(threads), "--out", os.path.basename(out)] + list(extra)
    cp = run_ref(args, cwd)
    if cp.returncode != 0:
        raise RuntimeError("reference plink2 failed:\n" + cp.stdout)
    return read_id_list(out + ".prune.in"), read_id_list(out + ".prune.out"), cp.stdout


def split_pgen_index(pgen_path, out_pgen, out_pgi):
    """A standard (0x10) .pgen rewritten as an external-index pair (pgen_spec.tex:149-170): the header becomes the .pgen.pgi
    (third byte 0x30, block offsets re-based), the records follow a bare three-byte .pgen header (mode 0x20)."""
    data = open(pgen_path, "rb").read()
    assert data[:3] == bytes([0x6C, 0x1B, 0x10])
    m = int.from_bytes(data[3:7], "little")
    n_blocks = (m + 65535) // 65536
    offs = [int.from_bytes(data[12 + 8 * b:20 + 8 * b], "little") for b in range(n_blocks)]
    header_len = offs[0]
    hdr = bytearray(data[:header_len])
    hdr[2] = 0x30
    for b, o in enumerate(offs):
        hdr[12 + 8 * b:20 + 8 * b] = (o - header_len + 3).to_bytes(8, "little")
    with open(out_pgi, "wb") as f:
        f.write(bytes(hdr))
    with open(out_pgen, "wb") as f:
        f.write(bytes([0x6C, 0x1B, 0x20]) + data[header_len:])


def add_pgen_header_extension(pgen_path, out_path, writer_id=b"ldtools test writer"):
    """A standard (0x10) .pgen rewritten with an ignorable header extension (mode 0x11, pgen_spec.tex:237-270): header flag
    varint 0x2 (writer identifier), no footer extensions, the body's length, the body; block offsets shifted accordingly."""
    data = open(pgen_path, "rb").read()
    assert data[:3] == bytes([0x6C, 0x1B, 0x10]) and len(writer_id) < 128
    m = int.from_bytes(data[3:7], "little")
    n_blocks = (m + 65535) // 65536
    offs = [int.from_bytes(data[12 + 8 * b:20 + 8 * b], "little") for b in range(n_blocks)]
    header_len = offs[0]
    ext = bytes([0x02, 0x00, len(writer_id)]) + writer_id
    hdr = bytearray(data[:header_len])
    hdr[2] = 0x11
    for b, o in enumerate(offs):
        hdr[12 + 8 * b:20 + 8 * b] = (o + len(ext)).to_bytes(8, "little")
    with open(out_path, "wb") as f:
        f.write(bytes(hdr) + ext + data[header_len:])


# ---------------------------------------------------------------- every candidate pair of a band, by plain matrix products
PAIR_FIELDS = ("nm", "sum1", "ssq1", "sum2", "ssq2", "dot")


def band_pairs(lo):
    """(first, second) int64 index arrays of every candidate pair of a band, in the order of ldp_run_with_stats()'s stats
    array: second variant ascending, first variant from lo[second] to second - 1."""
    lo = np.asarray(lo, dtype=np.int64)
    m = len(lo)
    j = np.arange(m, dtype=np.int64)
    cnt = np.maximum(j - lo, 0)
    second = np.repeat(j, cnt)
    off = np.concatenate([[0], np.cumsum(cnt)])
    first = np.arange(int(off[-1]), dtype=np.int64) - np.repeat(off[:-1] - lo, cnt)
    return first, second


def band_pair_stats(raw, lo, block=256, orient=True):
    """The six integers (nm, sum1, ssq1, sum2, ssq2, dot) of EVERY candidate pair (i, j), lo[j] <= i < j, as a (pairs, 6) int64
    array in band order (band_pairs).  raw: REF-based codes (M, N); every variant is oriented on its major allele (REF unless
    ref_ct * (1 / total) < 0.5, the definition of plink2_common.h:559-567; an exact tie goes to REF), x = +1 hom-major, 0 het,
    -1 hom-minor, and the sums run over the samples both variants have a call for.  Plain float64 matrix products of the
    three indicator / valued matrices (call present, homozygous, x): every sum is an integer far below 2^53, so the products
    are exact whatever order BLAS adds in.  Shares no code with oracle/ldoracle.c or with the kernels.
    orient=False: every row keeps the REF orientation (x = +1 hom-REF, -1 hom-ALT; the statistics behind the REF-oriented r of
    --r-unphased, ldp_set_r_signed(2)) -- no major allele is looked at, nothing is flipped afterwards."""
    raw = np.asarray(raw)
    lo = np.asarray(lo, dtype=np.int64)
    m, n = raw.shape
    n_ref = (raw == 0).sum(1).astype(np.int64)
    n_het = (raw == 1).sum(1).astype(np.int64)
    n_alt = (raw == 2).sum(1).astype(np.int64)
    ref_ct = 2 * n_ref + n_het
    tot = ref_ct + 2 * n_alt + n_het
    ref_freq = np.where(tot > 0, ref_ct.astype(np.float64) * (1.0 / np.maximum(tot, 1).astype(np.float64)), 0.5)
    sign = np.where(ref_freq >= 0.5, 1.0, -1.0) if orient else np.ones(m)
    C = (raw != 3).astype(np.float64)
    H = ((raw == 0) | (raw == 2)).astype(np.float64)
    X = ((raw == 0).astype(np.float64) - (raw == 2).astype(np.float64)) * sign[:, None]
    cnt = np.maximum(np.arange(m, dtype=np.int64) - lo, 0)
    off = np.concatenate([[0], np.cumsum(cnt)])
    out = np.zeros((int(off[-1]), 6), dtype=np.int64)
    for j0 in range(0, m, block):
        j1 = min(m, j0 + block)
        if off[j1] == off[j0]:
            continue
        i0 = int(min(lo[j0:j1].min(), j0))
        Ci, Hi, Xi = C[i0:j1], H[i0:j1], X[i0:j1]
        CjT, HjT, XjT = C[j0:j1].T, H[j0:j1].T, X[j0:j1].T
        prods = (Ci @ CjT, Xi @ CjT, Hi @ CjT, Ci @ XjT, Ci @ HjT, Xi @ XjT)   # [i - i0, j - j0]
        for j in range(j0, j1):
            if cnt[j]:
                a, b = int(lo[j]) - i0, j - i0
                for f in range(6):
                    out[off[j]:off[j + 1], f] = np.rint(prods[f][a:b, j - j0]).astype(np.int64)
    return out


def _stats_columns(stats):
    stats = np.asarray(stats)
    if stats.dtype.names:
        return [stats[f].astype(np.int64) for f in PAIR_FIELDS]
    return [stats[:, f].astype(np.int64) for f in range(6)]


def band_cov_vars(stats):
    """(cov12, var1, var2) as float64 arrays: the integer parts in int64 (plink2_ld.cc:1085-1087), then one conversion each."""
    nm, s1, q1, s2, q2, dot = _stats_columns(stats)
    return (dot * nm - s1 * s2).astype(np.float64), (q1 * nm - s1 * s1).astype(np.float64), (q2 * nm - s2 * s2).astype(np.float64)


R2_NAN64 = 0xfff8000000000000   # what the reference's 0.0 / 0.0 leaves on x86; its float32 cast is R2_NAN32
R2_NAN32 = 0xffc00000


def band_r2(stats, signed=0):
    """r^2 of every pair as ComputeR2 forms it (plink2_ld.cc:6654-6682), float64, from the six integers: both variances and the
    covariance in int64 with ONE conversion each, variance_prod = var0 * var1, NaN (R2_NAN64) when nm == 0 or variance_prod == 0.0,
    otherwise (cov * cov) / variance_prod -- separate numpy operations, each rounded on its own, nothing fused.
    signed=1: r = +-sqrt(r^2) with the sign of the int64 covariance (--r-unphased); a zero covariance gives +0.0, NaN stays NaN.
    The orientation is the statistics': band_pair_stats(..., orient=False) gives the REF-oriented r."""
    nm, s1, q1, s2, q2, dot = _stats_columns(stats)
    var0 = (q1 * nm - s1 * s1).astype(np.float64)
    var1 = (q2 * nm - s2 * s2).astype(np.float64)
    cov_int = dot * nm - s1 * s2
    cov = cov_int.astype(np.float64)
    variance_prod = var0 * var1
    undefined = (nm == 0) | (variance_prod == 0.0)
    num = cov * cov
    out = num / np.where(undefined, 1.0, variance_prod)
    if signed:
        out = np.sqrt(out)
        neg = cov_int < 0
        out[neg] = -out[neg]
    out.view(np.uint64)[undefined] = R2_NAN64
    return out


def r2_to_float32(values):
    """the float32 form of the r^2 outputs: the IEEE cast of the double, NaN as R2_NAN32"""
    values = np.asarray(values, dtype=np.float64)
    nan = np.isnan(values)
    out = np.where(nan, 0.0, values).astype(np.float32)
    out.view(np.uint32)[nan] = R2_NAN32
    return out


def self_r2(raw):
    """the diagonal of the r^2 matrix: r^2(v, v) through the same formula = 1.0, or NaN for a variant without variance"""
    raw = np.asarray(raw)
    nm = (raw != 3).sum(1).astype(np.int64)
    s = (raw == 0).sum(1).astype(np.int64) - (raw == 2).sum(1).astype(np.int64)
    q = ((raw == 0) | (raw == 2)).sum(1).astype(np.int64)
    st = np.stack([nm, s, q, s, q, q], 1)
    return band_r2(st)


def band_to_dense(values, lo, row_first, row_ct, col_first, col_ct, diag=None):
    """Band-order values (band_pairs(lo) order; (pairs,) or (pairs, k)) scattered into the dense layout the engine returns for rows
    [row_first, +row_ct) x columns [col_first, +col_ct): element [j - row_first, i - col_first] for the pairs i < j of the band inside
    the block, `diag[j]` at i == j where given, zero bits everywhere else."""
    values = np.asarray(values)
    first, second = band_pairs(lo)
    out = np.zeros((row_ct, col_ct) + values.shape[1:], dtype=values.dtype)
    sel = (second >= row_first) & (second < row_first + row_ct) & (first >= col_first) & (first < col_first + col_ct)
    out[second[sel] - row_first, first[sel] - col_first] = values[sel]
    if diag is not None:
        j = np.arange(max(row_first, col_first), min(row_first + row_ct, col_first + col_ct), dtype=np.int64)
        out[j - row_first, j - col_first] = np.asarray(diag)[j]
    return out


def bits_of(a):
    """the bit patterns of a float32 / float64 array (comparisons of r^2 outputs are on these: NaN payloads and signed zeros count)"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def band_decisions(stats, r2):
    """The prune predicate of every pair: cov * cov > (thr * var1) * var2 with thr = ldo_prune_thresh(r2), three float64
    multiplications in exactly that order, var1 the FIRST variant's (plink2_ld.cc:1085-1090; numpy's elementwise products are
    separate roundings, nothing is contracted).  stats: (pairs, 6) integers or a structured array with PAIR_FIELDS."""
    thr = float(oracle().ldo_prune_thresh(float(r2)))
    cov, v1, v2 = band_cov_vars(stats)
    return (cov * cov) > ((thr * v1) * v2)


def compare_decisions(got, want, lo, stats, r2, counters=None, limit=10):
    """Per-pair comparison of two decision arrays in band order: (number of differing pairs, message).  The message names the
    first `limit` differing pairs (i, j) with their six integers, cov^2 / (thr var1 var2) and, when given, the route counters
    of the run, so that a failure says whether it is a bound, an ownership error or arithmetic."""
    got = np.asarray(got, dtype=bool)
    want = np.asarray(want, dtype=bool)
    if got.shape != want.shape:
        return max(len(got), len(want)), "decision arrays differ in length: %d vs %d" % (len(got), len(want))
    bad = np.flatnonzero(got != want)
    if not len(bad):
        return 0, "all %d pairs agree" % len(got)
    first, second = band_pairs(lo)
    thr = float(oracle().ldo_prune_thresh(float(r2)))
    cols = _stats_columns(stats)
    cov, v1, v2 = band_cov_vars(stats)
    lines = ["%d of %d pairs differ (got %d true, want %d true)" % (len(bad), len(got), int(got.sum()), int(want.sum()))]
    for k in bad[:limit]:
        den = (thr * v1[k]) * v2[k]
        ratio = (cov[k] * cov[k]) / den if den != 0 else float("nan")
        lines.append("  pair (i=%d, j=%d): got %d want %d; nm,sum1,ssq1,sum2,ssq2,dot = %s; cov^2/(thr var1 var2) = %.17g"
                     % (first[k], second[k], int(got[k]), int(want[k]), tuple(int(c[k]) for c in cols), ratio))
    if counters is not None:
        keys = ("pair_kernel_launches", "route_complete_launches", "route_sparse_launches", "route_general_launches", "sparse_tile_launches",
                "four_tile_launches", "wide_tiles", "mfma_skipped_product_stages", "sparse_exact_pairs", "pred_true")
        lines.append("  counters: " + ", ".join("%s=%s" % (k, counters[k]) for k in keys if k in counters))
    return len(bad), "\n".join(lines)


# ---------------------------------------------------------------- the engine's columns for rows that are re-laid out on the way in
def hap_raw_codes(raw, phaseinfo):
    """LDP_GENO_PHASED rows as the engine's image holds them: (M, S) REF-based codes + (M, S) phaseinfo bits -> (M, 2S) codes of
    the haplotype "samples", 2 = the haplotype carries ALT, 0 = it does not, 3 on both = a missing call.  Sample s owns columns
    2s and 2s + 1, and a het call's ALT allele goes to column 2s + 1 when its phaseinfo bit is set ("1|0", oracle_hapsplit),
    to column 2s otherwise: the bit order of HapsplitMustPhased's output (pgenlib_misc.cc:1917: het + phaseinfo -> binary 10),
    which the count pass keeps (hap_codes_of_16 in ldp_codes.hip) and tests/test_input_forms_reference.py compares with the
    oracle's rows bit by bit.
    The prune decision cov^2 > thr var1 var2 does not depend on which allele a row is oriented on (a flipped row changes the
    sign of its sum and of the dot product, hence of cov, and nothing else), so band_pair_stats / band_decisions over these
    codes -- or over mapped_raw_codes, or over REF-coded rows of any other input form -- is the one reference for every form
    in which rows reach the image; the statistics themselves are 4 x the reference's haplotype ones
    (test_pairphase.py::test_haplotype_statistics_are_a_quarter_of_the_genotype_coded_ones), the decisions the same bits."""
    raw = np.asarray(raw)
    info = np.asarray(phaseinfo).astype(bool)
    m, s = raw.shape
    het = raw == 1
    out = np.empty((m, 2 * s), dtype=np.uint8)
    out[:, 0::2] = np.where(raw == 3, 3, np.where((raw == 2) | (het & ~info), 2, 0))
    out[:, 1::2] = np.where(raw == 3, 3, np.where((raw == 2) | (het & info), 2, 0))
    return out


def mapped_raw_codes(raw, src, het_to_missing):
    """LDP_GENO_MAPPED rows as the engine's image holds them: column f = sample src[f] of the file's REF-based row, a het call
    turned into a missing one where het_to_missing[f] is set (ldp_set_sample_map).  The statistics of every pair are those of
    these columns (band_pair_stats); only the major allele -- which no decision depends on, see hap_raw_codes -- is counted
    before the substitution (host_rows)."""
    cols = np.asarray(raw)[:, np.asarray(src, dtype=np.int64)].copy()
    cols[(cols == 1) & (np.asarray(het_to_missing)[None, :] != 0)] = 3
    return cols


def host_rows(raw, src, het_missing):
    """numpy restatement of the host builder of sample-mapped rows: (inverse-coded rows, maj_freq, ALT-is-major flags)"""
    cols = raw[:, src]                                   # raw REF codes of the engine's columns
    ref_ct = 2 * (cols == 0).sum(1) + (cols == 1).sum(1)
    alt_ct = 2 * (cols == 2).sum(1) + (cols == 1).sum(1)
    tot = ref_ct + alt_ct
    ref_freq = np.full(raw.shape[0], 0.5)
    nz = tot > 0
    ref_freq[nz] = ref_ct[nz].astype(np.float64) * (1.0 / tot[nz].astype(np.float64))
    alt_major = ~(ref_freq >= 0.5)
    mf = np.where(alt_major, np.maximum(1.0 - ref_freq, 0.0), ref_freq)
    out = cols.copy()
    out[(cols == 1) & (het_missing[None, :] != 0)] = 3
    inv = np.array([2, 1, 0, 3], dtype=out.dtype)
    out[alt_major] = inv[out[alt_major]]
    return out, mf, alt_major


def major_oriented_planes(codes, alt_major=None):
    """what LdPruneEngine.planes() returns for a row whose image holds `codes` ((N,) REF-based codes): the hom and ref2het bit
    planes of the row oriented on its major allele (uint32 words, sample s -> bit s % 32 of word s // 32; padding clear).
    alt_major: the major allele where the codes alone do not decide it (sample-mapped rows: host_rows)"""
    codes = np.asarray(codes)
    if alt_major is None:
        ref_ct = 2 * int((codes == 0).sum()) + int((codes == 1).sum())
        tot = ref_ct + 2 * int((codes == 2).sum()) + int((codes == 1).sum())
        alt_major = not ((ref_ct * (1.0 / tot) if tot else 0.5) >= 0.5)
    major = 2 if alt_major else 0
    hom = pack_bits(((codes == 0) | (codes == 2))[None, :].astype(np.uint8)).view(np.uint32)[0]
    r2h = pack_bits(((codes == major) | (codes == 1))[None, :].astype(np.uint8)).view(np.uint32)[0]
    w = (len(codes) + 31) // 32
    return hom[:w], r2h[:w]


# ---------------------------------------------------------------- the count pass's checkpoint statistics, from the image row's codes
CP_CHECKPOINTS, CP_GEN_FIRST, CP_GEN_CHECKPOINTS = 5, 2, 2   # csrc/ldp_device.h: kCheckpoints, kGenCheckpointFirst, kGenCheckpoints
CP_CHUNK_SAMPLES = 512
CP_STEPS = (0.012, 0.04, 0.08, 0.16, 0.36)
CP_UNUSED = 0xffffffff


def checkpoint_chunks(n, r2):
    """The k-chunks (512 samples) at which a prune engine over n samples places its checkpoints, the rule of csrc/ldp_engine.cpp
    restated: none below four chunks; otherwise the fractions 1 - sqrt(r2) + CP_STEPS that stay below 0.93, each times the chunk
    count and rounded up, kept when strictly above the previous one and below the chunk count."""
    chunks = (n + CP_CHUNK_SAMPLES - 1) // CP_CHUNK_SAMPLES
    out = []
    if chunks >= 4:
        f0 = 1.0 - float(np.sqrt(np.float64(r2)))
        for step in CP_STEPS:
            f = f0 + step
            if f < 0.93:
                c = int(np.ceil(chunks * f))
                if c and c < chunks and (not out or c > out[-1]):
                    out.append(c)
    return out


def cp_tv_scale(r2):
    return float(np.sqrt(np.sqrt(np.float64(r2) * (1 + K_SMALL_EPSILON)) * (1.0 - 1e-6)))


def cp_reference(image_codes, n, chunks_list, r2):
    """What the count pass stores per variant (csrc/ldp_device.h: cp_slot, cp_gen_slot), from the codes of the FINAL image rows:
    image_codes (M, n), 0 / 1 / 2 / 3 as the image holds them (the raw codes with 0 <-> 2 swapped where the engine stores the row
    inverted).  x = +1 / 0 / -1 and z = 0 / 1 / 2 for codes 0 / 1 / 2.  chunks_list: the checkpoints in use (checkpoint_chunks); the
    others give zeros.  Returns a dict of int64 (M, 5) arrays over the samples >= 512 * chunk -- hom_r (codes 0 and 2), s_r (sum x),
    calls_r, zs_r (sum z), zq_r (sum z^2) --, the whole-row int64 (M,) arrays hom, S, calls, zs, zq, and the float64 (M, 6) arrays a, b:
        slot k < 5: a = s_r sqrt(n / n_r), b = sqrt(n (hom_r - s_r^2 / n_r)), n_r = n - 512 chunk
        slot 5:     a = S,                 b = sqrt(n hom - S^2) cp_tv_scale(r2)
    every operation a separate float64 rounding, in the order written."""
    codes = np.asarray(image_codes)
    m = codes.shape[0]
    assert codes.shape[1] == n and len(chunks_list) <= CP_CHECKPOINTS
    n_chunks = (n + CP_CHUNK_SAMPLES - 1) // CP_CHUNK_SAMPLES
    per = np.zeros((3, m, n_chunks + 1), dtype=np.int64)    # per code and chunk; a zero behind the last chunk
    for c in range(3):
        hit = np.zeros((m, n_chunks * CP_CHUNK_SAMPLES), dtype=np.uint8)
        hit[:, :n] = codes == c
        per[c, :, :n_chunks] = hit.reshape(m, n_chunks, CP_CHUNK_SAMPLES).sum(2, dtype=np.int64)
    suffix = np.cumsum(per[:, :, ::-1], axis=2)[:, :, ::-1]   # [c, v, k]: code-c calls in chunks >= k
    out = {}
    out["hom"] = suffix[0, :, 0] + suffix[2, :, 0]
    out["S"] = suffix[0, :, 0] - suffix[2, :, 0]
    out["calls"] = out["hom"] + suffix[1, :, 0]
    out["zs"] = suffix[1, :, 0] + 2 * suffix[2, :, 0]
    out["zq"] = suffix[1, :, 0] + 4 * suffix[2, :, 0]
    for name in ("hom_r", "s_r", "calls_r", "zs_r", "zq_r"):
        out[name] = np.zeros((m, CP_CHECKPOINTS), dtype=np.int64)
    a = np.zeros((m, CP_CHECKPOINTS + 1), dtype=np.float64)
    b = np.zeros((m, CP_CHECKPOINTS + 1), dtype=np.float64)
    nn = np.float64(n)
    for k, chunk in enumerate(chunks_list):
        assert 0 < chunk < n_chunks
        c0, c1, c2 = (suffix[c, :, chunk] for c in range(3))
        out["hom_r"][:, k] = c0 + c2
        out["s_r"][:, k] = c0 - c2
        out["calls_r"][:, k] = c0 + c1 + c2
        out["zs_r"][:, k] = c1 + 2 * c2
        out["zq_r"][:, k] = c1 + 4 * c2
        n_r = np.float64(n - CP_CHUNK_SAMPLES * chunk)
        s_r = (c0 - c2).astype(np.float64)
        v_r = np.maximum((c0 + c2).astype(np.float64) - (s_r * s_r) / n_r, 0.0)
        a[:, k] = s_r * np.sqrt(nn / n_r)
        b[:, k] = np.sqrt(nn * v_r)
    S = out["S"].astype(np.float64)
    a[:, CP_CHECKPOINTS] = S
    b[:, CP_CHECKPOINTS] = np.sqrt(np.maximum(nn * out["hom"].astype(np.float64) - S * S, 0.0)) * cp_tv_scale(r2)
    out["a"], out["b"] = a, b
    return out


def cp_recover(a, b, n, chunks_list):
    """the integers back from the remainder slots, the way a checkpoint takes them: s_r = rint(a sqrt(n_r / n)),
    hom_r = rint(b^2 / n + s_r^2 / n_r); (s_r, hom_r, largest |value - integer| met) over the checkpoints in use"""
    a, b = np.asarray(a), np.asarray(b)
    s_r = np.zeros(a.shape[:1] + (CP_CHECKPOINTS,), dtype=np.int64)
    hom_r = np.zeros_like(s_r)
    worst = 0.0
    nn = np.float64(n)
    for k, chunk in enumerate(chunks_list):
        n_r = np.float64(n - CP_CHUNK_SAMPLES * chunk)
        sv = a[:, k] * np.sqrt(n_r / nn)
        s = np.rint(sv)
        hv = (b[:, k] * b[:, k]) / nn + (s * s) / n_r
        h = np.rint(hv)
        worst = max(worst, float(np.abs(sv - s).max(initial=0.0)), float(np.abs(hv - h).max(initial=0.0)))
        s_r[:, k], hom_r[:, k] = s.astype(np.int64), h.astype(np.int64)
    return s_r, hom_r, worst


CP_ROW_KINDS = ("random complete", "random 3% missing", "all missing", "all het", "monomorphic REF", "monomorphic ALT", "ALT-major with hets",
                "exact tie", "complete but the last sample", "missing behind the last checkpoint", "missing before the first checkpoint",
                "hom calls in one chunk before the first checkpoint", "hom calls in the last chunk", "60% missing", "random complete 2",
                "random 3% missing ALT-major")


def cp_test_rows(n, r2, count=16, seed=0):
    """The rows tests/test_count_pass_slots.py feeds every count-pass form: (count, n) raw REF-based codes, one per CP_ROW_KINDS (the
    first `count` of them), placed relative to checkpoint_chunks(n, r2)."""
    rng = np.random.default_rng(1000003 * seed + n)
    cps = checkpoint_chunks(n, r2)
    n_chunks = (n + CP_CHUNK_SAMPLES - 1) // CP_CHUNK_SAMPLES
    first = (cps[0] if cps else max(n_chunks - 1, 1)) * CP_CHUNK_SAMPLES     # samples in front of the first checkpoint
    last = (cps[-1] if cps else max(n_chunks - 1, 1)) * CP_CHUNK_SAMPLES     # ... and of the last one
    first, last = min(first, n - 1), min(last, n - 1)

    def draw(maf):
        return ((rng.random(n) < maf).astype(np.uint8) + (rng.random(n) < maf).astype(np.uint8)).astype(np.uint8)

    rows = np.empty((len(CP_ROW_KINDS), n), dtype=np.uint8)
    rows[0] = draw(0.3)
    rows[1] = np.where(rng.random(n) < 0.03, 3, draw(0.2))
    rows[2] = 3
    rows[3] = 1
    rows[4] = 0
    rows[5] = 2
    rows[6] = draw(0.8)
    tie = np.ones(n, dtype=np.uint8)                 # as many REF as ALT alleles: ref_freq = 0.5 exactly, REF stays major
    q = n // 4
    tie[:q] = 0
    tie[q:2 * q] = 2
    rows[7] = rng.permutation(tie)
    rows[8] = draw(0.4)
    rows[8, n - 1] = 3
    rows[9] = draw(0.7)
    rows[9, last:] = np.where(rng.random(n - last) < 0.2, 3, rows[9, last:])
    rows[9, n - 1] = 3
    rows[10] = draw(0.35)
    rows[10, :first] = np.where(rng.random(first) < 0.2, 3, rows[10, :first])
    rows[10, 0] = 3
    one = (first // CP_CHUNK_SAMPLES - 1) * CP_CHUNK_SAMPLES   # the chunk in front of the first checkpoint
    rows[11] = 1
    rows[11, one:one + CP_CHUNK_SAMPLES] = np.where(rng.random(CP_CHUNK_SAMPLES) < 0.7, 2, 0)[:n - one]
    tail0 = (n_chunks - 1) * CP_CHUNK_SAMPLES
    rows[12] = 1
    rows[12, tail0:] = np.where(rng.random(n - tail0) < 0.3, 2, 0)
    rows[13] = np.where(rng.random(n) < 0.6, 3, draw(0.25))
    rows[14] = draw(0.05)
    rows[15] = np.where(rng.random(n) < 0.03, 3, draw(0.9))
    return np.ascontiguousarray(rows[:count])
