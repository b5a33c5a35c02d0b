"""Every candidate pair's prune decision for each way rows reach the image.

tests/test_pair_decisions.py loads every engine one way (aligned REF rows from host memory).  The count pass codes_kernel
(ldp_codes.hip) has many more entry forms, and each of them produces the records, the image orientation and the checkpoint statistics
(cp_stats) that the pair kernels' early termination trusts -- statistics without an accessor: a wrong slot shows only as a pair dropped at
a checkpoint.  Each case here brings the SAME kind of rows into an engine through one input form, runs it with the production settings
and checks (a)-(e) of test_pair_decisions.decide() -- every decision against ldtools.band_pair_stats / band_decisions, which do not
depend on the allele a row is oriented on and therefore serve every form (tests/test_input_forms_reference.py) -- at a size where the
checkpoints retire products: N = 20,003 samples (39 k-chunks of 512 + a 35-sample tail unit, three samples in the last byte), S = 10,001
phased samples (20,002 haplotypes, 2,501 code bytes, phase bits at offset 2,504).  Every form runs on complete rows and on rows with 5 %
missing calls in every third row; every fourth row has its alleles swapped, so both image orientations occur.  The baseline -- the
image's columns as REF rows from host memory, the path of test_pair_decisions.py -- must give identical decisions and route counters,
and on complete rows it must retire product stages (asserted on the baseline itself: N was not tuned against a form under test)."""
import copy
import os

import numpy as np
import pytest

import ldtools as T
from test_host_logic import make_positions
from test_pair_decisions import Reference, decide, run_and_compare

pytestmark = pytest.mark.gpu

N = 20003            # samples of the unphased forms
S = 10001            # samples of the phased forms
# The sample-mapped forms: 7,000 columns whose het calls become missing + samples that appear twice.  With 6,501 of the latter (20,002 columns)
# every row misses 11.4 % of its calls and the baseline's launch -- on the general route, whose checkpoint bound pays for every call that may
# drop out -- retires none of 32,640 product stages; so the columns were raised by k-chunks, the 7,000 kept, by the baseline alone: at
# 20,002 + 20 * 512 = 30,242 columns (8.3 % missing) it retires 13,104 of 48,960.  The file has the 1,499 unused samples it had at 15,000.
MAP_ONES, MAP_TWICE = 7000, 11621
N_MAPPED = MAP_ONES + 2 * MAP_TWICE   # 30,242 = 59 * 512 + 34
N_RAW = MAP_ONES + MAP_TWICE + 1499   # 20,120 samples in the file the rows are gathered from
SWAP = np.array([2, 1, 0, 3], dtype=np.uint8)
BED = np.array([3, 2, 0, 1], dtype=np.uint8)   # .pgen code -> .bed code
VARIANTS = ("complete", "missing")

# m, window, engine options, rows the restricted engine is loaded with
PLANS = {"narrow": (700, 150, {"wide_min_reach": 1e9}, 900),
         "tiles": (1500, 600, {"wide_min_reach": 12}, 1900)}
R2, STEP, ORDER = 0.5, 1, 2

TOTALS = {"compared": 0, "candidate_pairs": 0, "engines": 0}
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---------------------------------------------------------------- rows
def _late_ld(m, n_cols, seed):
    """test_complete_rows_on_the_tiles_with_checkpoints' rows: (v, column permutation of the first 60 %) for the rows that become correlated
    with the row 37 back only in the last 40 % of the columns"""
    rng = np.random.default_rng(seed)
    cut = int(0.6 * n_cols)
    return cut, [(v, rng.permutation(cut)) for v in range(40, m, 11)]


def unphased_rows(plan, variant, seed, n=N):
    def make():
        m = PLANS[plan][0]
        raw = T.synth_raw_codes(m, n, seed, 0.0, ld_copy_prob=0.6, redraw=0.1)
        if plan == "tiles":
            cut, rows = _late_ld(m, n, n + m + seed)
            for v, perm in rows:
                raw[v, :cut] = raw[v, perm]
                raw[v, cut:] = raw[v - 37, cut:]
        if variant == "missing":
            rng = np.random.default_rng(seed + 17)
            part = raw[0::3]
            part[rng.random(part.shape) < 0.05] = 3
            raw[0::3] = part
        raw[1::4] = SWAP[raw[1::4]]
        raw.setflags(write=False)
        return raw
    return cached(("rows", plan, variant, seed, n), make)


def phased_rows(plan, variant, seed):
    def make():
        m = PLANS[plan][0]
        raw, _, info = T.synth_phased(m, S, seed, 0.0, ld_copy_prob=0.6, redraw=0.1)
        if plan == "tiles":
            cut, rows = _late_ld(m, S, S + m + seed)
            for v, perm in rows:
                raw[v, :cut], info[v, :cut] = raw[v, perm], info[v, perm]
                raw[v, cut:], info[v, cut:] = raw[v - 37, cut:], info[v - 37, cut:]
        if variant == "missing":
            rng = np.random.default_rng(seed + 17)
            part = raw[0::3]
            part[rng.random(part.shape) < 0.05] = 3
            raw[0::3] = part
        # the alleles swapped: 0 <-> 2, and a het's ALT allele is now the one that was REF, on the other haplotype
        raw[1::4] = SWAP[raw[1::4]]
        info[1::4] ^= 1
        info &= (raw == 1).astype(np.uint8)
        raw.setflags(write=False)
        info.setflags(write=False)
        return raw, info
    return cached(("phased rows", plan, variant, seed), make)


def positions(plan):
    m = PLANS[plan][0]
    if plan == "narrow":
        return make_positions(m, 2, 5)
    return np.repeat(np.arange(2, dtype=np.uint32), m // 2), None


def row_bytes_of(codes):
    """(M, n) 2-bit codes -> (M, ceil(n / 4)) bytes: rows as a .pgen / .bed file holds them, no padding"""
    m, n = codes.shape
    return np.ascontiguousarray(T.pack_2bit(codes).view(np.uint8).reshape(m, -1)[:, :(n + 3) // 4])


# ---------------------------------------------------------------- references and baselines
def new_reference(pkg, plan, raw, **kw):
    m, window, _, _ = PLANS[plan]
    chr_idx, bps = positions(plan)
    return Reference(pkg, raw, chr_idx, bps, window, STEP, False, R2, ORDER, **kw)


def plain_reference(pkg, plan, variant):
    return cached(("plain", plan, variant), lambda: new_reference(pkg, plan, unphased_rows(plan, variant, 41)))


def second_reference(pkg, plan, variant):
    """the rows of plain_reference with every third row replaced by a row of a second seed"""
    def make():
        raw = unphased_rows(plan, variant, 41).copy()
        raw[0::3] = unphased_rows(plan, variant, 1041)[0::3]
        return new_reference(pkg, plan, raw)
    return cached(("second", plan, variant), make)


def phased_reference(pkg, plan, variant):
    def make():
        raw, info = phased_rows(plan, variant, 43)
        m, window, _, _ = PLANS[plan]
        chr_idx, bps = positions(plan)
        hrows, mf, unphased, hap_ct = T.oracle_hapsplit(raw, (raw == 1).astype(np.uint8), info)
        assert hap_ct == 2 * S and not unphased.any()
        removed, _ = T.oracle_indep_pairphase(hrows, hap_ct, chr_idx, bps if bps is not None else np.arange(m, dtype=np.uint32), mf, window, STEP, False, R2, ORDER)
        ref = new_reference(pkg, plan, raw, raw_for_stats=T.hap_raw_codes(raw, info), removed=removed)
        ref.info = info
        return ref
    return cached(("phased", plan, variant), make)


def mapped_reference(pkg, variant):
    def make():
        plan = "narrow"
        raw = unphased_rows(plan, variant, 47, n=N_RAW)
        perm = np.random.default_rng(N_RAW).permutation(N_RAW)
        part1, part2 = np.sort(perm[:MAP_ONES]), np.sort(perm[MAP_ONES:MAP_ONES + MAP_TWICE])
        src = np.concatenate([part1, part2, part2]).astype(np.uint32)
        het = np.concatenate([np.ones(MAP_ONES, np.uint8), np.zeros(2 * MAP_TWICE, np.uint8)])
        m, window, _, _ = PLANS[plan]
        chr_idx, bps = positions(plan)
        rows, mf, alt_major = T.host_rows(raw, src, het)
        removed, _ = T.oracle_indep_pairwise(T.pack_2bit(rows), len(src), chr_idx, bps, mf, window, STEP, False, R2, ORDER)
        ref = new_reference(pkg, plan, raw, raw_for_stats=T.mapped_raw_codes(raw, src, het), removed=removed)
        assert ref.n == N_MAPPED == 30242 and N_MAPPED % 512 == (2 * S) % 512
        ref.src, ref.het, ref.mf, ref.alt_major = src, het, mf, alt_major
        return ref
    return cached(("mapped", variant), make)


ROUTE_KEYS = ("route_complete_launches", "route_sparse_launches", "route_general_launches", "sparse_tile_launches", "four_tile_launches", "wide_tiles")


def owned_mask(eng):
    owned = np.zeros(eng.variant_ct, dtype=bool)
    for length, first in eng.subcontigs():
        owned[first:first + length] = True
    return owned


def baseline(pkg, key, ref, plan, variant, options=None):
    """ref's image columns as REF rows from host memory -- the unchanged path: its decisions, counters and records.  That it retires product
    stages on complete rows is asserted by retires_stages(), after everything else of a case."""
    def make():
        base = ref
        if ref.raw is not ref.raw_for_stats:
            base = copy.copy(ref)
            base.raw = ref.raw_for_stats
            base.packed = T.pack_2bit(base.raw)
            if key[0] == "mapped":   # (REF rows decide the major allele from the calls they have: the tie-break frequencies differ)
                inv, mf, _ = T.oracle_prepare(base.raw)
                base.removed, _ = T.oracle_indep_pairwise(inv, base.n, base.chr_idx, base.bps if base.bps is not None else np.arange(base.m, dtype=np.uint32), mf,
                                                          base.window, STEP, False, R2, ORDER)
        got = {}

        def inspect(eng, c):
            got["pred"] = eng.last_pred()
            got["recs"] = eng.variant_recs().copy()
            got["c"] = c
        opts = PLANS[plan][2] if options is None else options
        decide(pkg, base, opts, label="baseline %s %s %s" % (key[0], plan, variant), inspect=inspect, totals=TOTALS)
        if plan == "tiles":
            assert got["c"]["wide_tiles"] > 0
        return got
    return cached(("baseline",) + key + (plan, variant), make)


SAME_AS_BASELINE = ("pred_true", "mfma_skipped_product_stages") + ROUTE_KEYS


def same_as_baseline(c, base, label):
    """The same image columns under the same plan: the same checkpoint statistics up to the rows' orientation -- which changes the sign of a
    row's slots and of its partial dot products together, exactly --, hence the same products retired at the same checkpoints.  (A count pass
    that leaves the remainders of major-allele-oriented rows empty makes the bound weaker, not wrong: no decision changes, this count does.)"""
    for k in SAME_AS_BASELINE:
        assert c[k] == base["c"][k], (label, k, c[k], base["c"][k])


def retires_stages(variant, base, c, label):
    """the last assertion of a case on complete rows: the baseline retires product stages at this size (otherwise raise N in steps of
    512 k + 35 -- by the baseline, never by a form under test), and so does the form"""
    if variant == "complete":
        assert base["c"]["mfma_skipped_product_stages"] > 0, (label, "the baseline retires no product stage at this size")
        assert c["mfma_skipped_product_stages"] > 0, label


def check_form(pkg, ref, base, plan, variant, load, label, oriented=True, inspect=None):
    """(a)-(e) for one input form, the counters against the baseline's, both image orientations"""
    def expect(c):
        if plan == "tiles":
            assert c["wide_tiles"] > 0
        else:
            assert c["wide_tiles"] == 0
        same_as_baseline(c, base, label)

    def look(eng, c):
        assert np.array_equal(eng.last_pred(), base["pred"]), label
        recs = eng.variant_recs()
        owned = owned_mask(eng)
        stored_inverted = ((recs["flags"] >> 3) & 1).astype(bool)[owned]
        if oriented:
            assert 0 < int(stored_inverted.sum()) < int(owned.sum()), label
        else:
            assert not stored_inverted.any(), label
        # the records are those of the baseline's rows, whatever the row came in as
        for f in ("nm_ct", "ssq"):
            assert np.array_equal(recs[f][owned], base["recs"][f][owned]), (label, f)
        assert np.array_equal(np.abs(recs["sum"][owned]), np.abs(base["recs"]["sum"][owned])), label
        assert np.array_equal(recs["flags"][owned] & 6, base["recs"]["flags"][owned] & 6), label
        if inspect is not None:
            inspect(eng, c, recs)
    c = decide(pkg, ref, PLANS[plan][2], expect, label="%s/%s/%s" % (label, plan, variant), load=load, inspect=look, totals=TOTALS)
    retires_stages(variant, base, c, label)
    return c


def planes_match(eng, ref, alt_major=None):
    """a few image rows, column by column, against the reference's columns (major-allele-oriented planes)"""
    for v in (0, 1, 2, 3, ref.m // 2, ref.m - 1):
        hom, r2h = eng.planes(v)
        want_hom, want_r2h = T.major_oriented_planes(ref.raw_for_stats[v], None if alt_major is None else bool(alt_major[v]))
        assert np.array_equal(hom, want_hom) and np.array_equal(r2h, want_r2h), v


def odd_stride(row_bytes):
    """the smallest odd stride that leaves at least one byte between rows: consecutive rows start at every alignment within a dword"""
    return row_bytes + (2 if row_bytes % 2 else 1)


def device_buffer(rows, stride, lead, garbage_bits):
    """rows (M, row_bytes) uint8 in a device buffer at base + lead with `stride` bytes between them, 0xA5 wherever no row byte lies and
    `garbage_bits` ORed into every row's last byte (bits of samples the row does not have): (tensor, address of row 0)"""
    import torch
    m, rb = rows.shape
    buf = np.full(lead + m * stride + 16, 0xA5, dtype=np.uint8)
    view = buf[lead:lead + m * stride].reshape(m, stride)
    view[:, :rb] = rows
    view[:, rb - 1] |= garbage_bits
    dev = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    assert dev.data_ptr() % 4 == 0
    return dev, dev.data_ptr() + lead


def tail_garbage(n):
    """the bits of the last row byte behind sample n - 1"""
    return (0xff << (2 * (n % 4))) & 0xff if n % 4 else 0


# ---------------------------------------------------------------- plain rows through the other doors
def _plain(pkg, plan, variant):
    ref = plain_reference(pkg, plan, variant)
    return ref, baseline(pkg, ("plain",), ref, plan, variant)


@pytest.mark.parametrize("variant", VARIANTS)
def test_bed_rows_from_host_memory(gpu_pkg, variant):
    """LDP_GENO_BED, rows ceil(N / 4) = 5,001 bytes apart: three of four rows start off a dword in the caller's buffer"""
    pkg = gpu_pkg
    ref, base = _plain(pkg, "narrow", variant)
    rows = row_bytes_of(BED[ref.raw])
    assert rows.shape[1] % 4 != 0

    def load(pkg, eng, ref):
        eng.load_genotypes_host(0, rows, pkg.LDP_GENO_BED)
    check_form(pkg, ref, base, "narrow", variant, load, "bed_host")


@pytest.mark.parametrize("variant", VARIANTS)
def test_inverse_rows_with_caller_frequencies(gpu_pkg, variant):
    """LDP_GENO_INVERSE + ldp_set_maj_freqs: nothing to orient, no allele counts in the records"""
    pkg = gpu_pkg
    ref, base = _plain(pkg, "narrow", variant)
    inv, mf, altmaj = T.oracle_prepare(ref.raw)
    assert 0 < int(altmaj.sum()) < ref.m

    def load(pkg, eng, ref):
        eng.load_genotypes_host(0, inv, pkg.LDP_GENO_INVERSE)
        eng.set_maj_freqs(0, mf)

    def inspect(eng, c, recs):
        assert not recs["n_homref"].any() and not recs["n_het"].any() and not recs["n_homalt"].any()
        assert not (recs["flags"] & 1).any()
    check_form(pkg, ref, base, "narrow", variant, load, "inverse_host", oriented=False, inspect=inspect)


@pytest.mark.parametrize("variant", VARIANTS)
def test_rows_from_a_file_descriptor(gpu_pkg, variant, tmp_path):
    """ldp_load_genotypes_fd: rows behind a three-byte header, ceil(N / 4) bytes apart, in two calls"""
    pkg = gpu_pkg
    ref, base = _plain(pkg, "narrow", variant)
    rows = row_bytes_of(ref.raw)
    path = str(tmp_path / "rows.bin")
    with open(path, "wb") as f:
        f.write(bytes([0x6C, 0x1B, 0x02]))
        f.write(rows.tobytes())
    stride = rows.shape[1]

    def load(pkg, eng, ref):
        fd = os.open(path, os.O_RDONLY)
        try:
            eng.load_genotypes_fd(0, 333, fd, 3, stride, pkg.LDP_GENO_REF)
            eng.load_genotypes_fd(333, ref.m - 333, fd, 3 + 333 * stride, stride, pkg.LDP_GENO_REF)
        finally:
            os.close(fd)
    check_form(pkg, ref, base, "narrow", variant, load, "fd")


@pytest.mark.parametrize("enc", ["ref", "bed"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_device_rows_off_the_dword(gpu_pkg, variant, enc):
    """Rows resident in device memory at base + 1 and an odd stride (ceil(N / 4) + 1 = 5,002 is even, so 5,003): three of four rows are
    not 4-byte aligned and go through codes_kernel's byte loads -- every unit in the rolled loop --, the fourth through the vector loads, in one
    launch.  Garbage between the rows and in the last byte's unused bits."""
    pkg = gpu_pkg
    ref, base = _plain(pkg, "narrow", variant)
    rows = row_bytes_of(ref.raw if enc == "ref" else BED[ref.raw])
    stride = odd_stride(rows.shape[1])
    assert stride % 2 == 1
    keep = []

    def load(pkg, eng, ref):
        dev, ptr = device_buffer(rows, stride, 1, tail_garbage(N))
        keep.append(dev)
        assert sorted({(ptr + k * stride) % 4 for k in range(8)}) == [0, 1, 2, 3]
        eng.load_genotypes_device(0, ref.m, ptr, stride, pkg.LDP_GENO_REF if enc == "ref" else pkg.LDP_GENO_BED)
    check_form(pkg, ref, base, "narrow", variant, load, "device_unaligned" + ("_bed" if enc == "bed" else ""))
    del keep[:]


# ---------------------------------------------------------------- phased rows
def _phased(pkg, plan, variant):
    ref = phased_reference(pkg, plan, variant)
    return ref, baseline(pkg, ("phased",), ref, plan, variant)


def _phased_host_load(pkg, eng, ref):
    rows = pkg.pack_phased_rows(T.pack_2bit(ref.raw).view(np.uint8).reshape(ref.m, -1), ref.info, S)
    assert rows.shape[1] == pkg.phased_row_bytes(2 * S) == 2504 + 1251
    for a, b in [(0, 123), (123, 124), (124, ref.m)]:
        eng.load_genotypes_host(a, rows[a:b], pkg.LDP_GENO_REF | pkg.LDP_GENO_PHASED)


def _phased_inspect(eng, c, recs):
    assert eng.founder_ct == 2 * S and int(recs["nm_ct"].max()) == 2 * S and not recs["n_het"].any()


@pytest.mark.parametrize("variant", VARIANTS)
def test_phased_rows_from_host_memory(gpu_pkg, variant):
    """LDP_GENO_REF | LDP_GENO_PHASED in three uneven pieces: hap_codes_of_16, every unit through the rolled loop; the image's columns are
    ldtools.hap_raw_codes', haplotype by haplotype"""
    pkg = gpu_pkg
    ref, base = _phased(pkg, "narrow", variant)

    def inspect(eng, c, recs):
        _phased_inspect(eng, c, recs)
        planes_match(eng, ref)
    check_form(pkg, ref, base, "narrow", variant, _phased_host_load, "phased_host", inspect=inspect)


@pytest.mark.parametrize("variant", VARIANTS)
def test_phased_inverse_rows_on_the_device(gpu_pkg, variant):
    """LDP_GENO_INVERSE | LDP_GENO_PHASED: major-allele-inverse codes, phaseinfo re-oriented with them (PgrGetInv1P), caller frequencies, rows
    resident in device memory at an odd stride"""
    pkg = gpu_pkg
    ref, base = _phased(pkg, "narrow", variant)
    inv, mf, altmaj = T.oracle_prepare(ref.raw)
    info_inv = np.where(altmaj[:, None].astype(bool), ref.info ^ 1, ref.info) & (ref.raw == 1)
    rows = pkg.pack_phased_rows(inv.view(np.uint8).reshape(ref.m, -1), info_inv, S)
    stride = odd_stride(rows.shape[1])
    keep = []

    def load(pkg, eng, ref):
        dev, ptr = device_buffer(rows, stride, 0, 0)
        keep.append(dev)
        eng.load_genotypes_device(0, ref.m, ptr, stride, pkg.LDP_GENO_INVERSE | pkg.LDP_GENO_PHASED)
        eng.set_maj_freqs(0, mf)
    check_form(pkg, ref, base, "narrow", variant, load, "phased_device_inverse", oriented=False)
    del keep[:]


# ---------------------------------------------------------------- sample-mapped rows
@pytest.mark.parametrize("enc", ["ref", "bed"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_sample_mapped_rows(gpu_pkg, variant, enc):
    """LDP_GENO_MAPPED: file rows of 20,120 samples, 7,000 columns whose het calls become missing + 11,621 samples twice (gather_rows_kernel,
    then the count pass with extra_het): 30,242 columns.  Het -> missing leaves missing calls in EVERY row, whatever the file's rows have, so
    also the [complete] cases take the general route; the size is the one at which their baseline retires product stages there (N_MAPPED)."""
    pkg = gpu_pkg
    ref = mapped_reference(pkg, variant)
    base = baseline(pkg, ("mapped",), ref, "narrow", variant)
    rows = row_bytes_of(ref.raw if enc == "ref" else BED[ref.raw])

    def load(pkg, eng, ref):
        eng.set_sample_map(N_RAW, ref.src, ref.het)
        eng.load_genotypes_host(0, rows, (pkg.LDP_GENO_REF if enc == "ref" else pkg.LDP_GENO_BED) | pkg.LDP_GENO_MAPPED)

    def inspect(eng, c, recs):
        assert np.array_equal(eng.maj_freqs(), ref.mf)     # exact doubles: the alleles are counted before het -> missing
        assert np.array_equal((recs["flags"] & 1).astype(bool), ref.alt_major)
        planes_match(eng, ref, ref.alt_major)
    check_form(pkg, ref, base, "narrow", variant, load, "mapped_" + enc, inspect=inspect)


# ---------------------------------------------------------------- rows counted where they lie
def _fill_mapped_rows(pkg, eng, raw, verify=None, rewrite=None):
    """ldp_map_rows per owned run; last_pred() refuses the engine from here until the load.  verify: the rows the image must hold now, in the
    input's orientation (the engine's own padding behind them); rewrite: (M,) bool, the rows to overwrite with raw's -- all when None.  Returns
    the mapped runs."""
    import torch
    runs = []
    rb = (N + 3) // 4
    for length, first in eng.subcontigs():
        ptr, stride = eng.map_rows(first, length)
        assert stride % 64 == 0 and stride >= rb
        with pytest.raises(pkg.LdpError) as ei:
            eng.last_pred()
        assert ei.value.code == pkg.LDP_ERR_STATE
        new = np.full((length, stride), 0xA5, dtype=np.uint8)        # garbage in the padding: the engine's to fill
        new[:, :rb] = row_bytes_of(raw[first:first + length])
        new[:, rb - 1] |= tail_garbage(N)                              # ... and in the bits behind the last sample
        if verify is not None:
            dev = torch.empty(length * stride, dtype=torch.uint8, device="cuda")
            assert pkg.hip_memcpy_dtod(dev.data_ptr(), ptr, length * stride) == 0
            now = dev.cpu().numpy().reshape(length, stride)
            assert np.array_equal(T.unpack_2bit(now[:, :rb], N), verify[first:first + length]), "mapped rows are not in the input's orientation"
            sel = rewrite[first:first + length]
            now[sel] = new[sel]
            new = now
        dev = torch.from_numpy(np.ascontiguousarray(new)).cuda()
        torch.cuda.synchronize()
        assert pkg.hip_memcpy_dtod(ptr, dev.data_ptr(), length * stride) == 0
        runs.append((first, length, ptr, stride))
    return runs


def _in_place(pkg, plan, variant):
    ref, base = _plain(pkg, plan, variant)
    ref2 = second_reference(pkg, plan, variant)
    base2 = baseline(pkg, ("second",), ref2, plan, variant)
    options = PLANS[plan][2]

    def load(pkg, eng, ref):
        for first, length, ptr, stride in _fill_mapped_rows(pkg, eng, ref.raw):
            eng.load_genotypes_device(first, length, ptr, stride, pkg.LDP_GENO_REF)

    def again(eng, c, recs):
        assert recs.tobytes() == base["recs"].tobytes()
        rewrite = np.zeros(ref.m, dtype=bool)
        rewrite[0::3] = True
        runs = _fill_mapped_rows(pkg, eng, ref2.raw, verify=ref.raw, rewrite=rewrite)
        with pytest.raises(pkg.LdpError) as ei:
            eng.run()                                                 # rows mapped again count as not loaded
        assert ei.value.code == pkg.LDP_ERR_STATE
        for first, length, ptr, stride in runs:
            eng.load_genotypes_device(first, length, ptr, stride, pkg.LDP_GENO_REF)

        c2 = run_and_compare(pkg, eng, ref2, options, lambda c2: same_as_baseline(c2, base2, "in_place/rewritten"), "in_place/rewritten/%s/%s" % (plan, variant), TOTALS)
        retires_stages(variant, base2, c2, "in_place/rewritten")
        assert np.array_equal(eng.last_pred(), base2["pred"])
        assert eng.variant_recs().tobytes() == base2["recs"].tobytes()
    check_form(pkg, ref, base, plan, variant, load, "in_place", inspect=again)


@pytest.mark.parametrize("variant", VARIANTS)
def test_rows_counted_in_place_and_again_after_a_rewrite(gpu_pkg, variant):
    """ldp_map_rows: REF rows written into the image (garbage in the padding and behind the last sample), counted in place, run; mapped
    again -- back in the input's orientation, checked --, every third row overwritten with a row of a second seed, counted again (the rows
    that stayed are read as they lie), run: both runs against their rows and their baselines, records included"""
    _in_place(gpu_pkg, "narrow", variant)


def _restricted(pkg, plan, variant, options=None, label="restricted"):
    """ldp_set_variants_matrix over more rows than are kept, ldp_restrict_variants to a random subset that IS the plain reference's rows
    (compacted in batches of 16), whose count pass reads the image in place with rows stored inverted (inv_in)"""
    ref = plain_reference(pkg, plan, variant)
    opts = PLANS[plan][2] if options is None else options
    base = baseline(pkg, ("plain",) + tuple(sorted(opts.items())) if options is not None else ("plain",), ref, plan, variant, opts)
    m, _, _, m_all = PLANS[plan]
    keep = np.zeros(m_all, dtype=bool)
    keep[np.random.default_rng(m_all).choice(m_all, size=m, replace=False)] = True
    rows = np.empty((m_all, N), dtype=np.uint8)
    rows[keep] = ref.raw
    rows[~keep] = unphased_rows(plan, variant, 1041)[:m_all - m]
    moved = {}

    def load(pkg, eng, ref):
        eng.set_variants_matrix(m_all)
        eng.load_genotypes_host(0, T.pack_2bit(rows), pkg.LDP_GENO_REF)
        eng.set_option("compact_batch_rows", 16)
        eng.restrict_variants(keep, ref.chr_idx, ref.bps)
        assert eng.variant_ct == m
        moved.update(eng.compact_stats())
        assert moved["rows_direct"] > 0 and moved["rows_bounced"] > 0 and moved["rows_direct"] + moved["rows_bounced"] == moved["rows_compacted"], moved

    def inspect(eng, c):
        # a fresh engine over the kept rows (the baseline): byte-equal records, the same decisions, the same retired stages
        recs = eng.variant_recs()
        assert recs.tobytes() == base["recs"].tobytes()
        if opts.get("pair_mfma", 1):
            assert 0 < int(((recs["flags"] >> 3) & 1).sum()) < m         # rows of both orientations were counted where they lay
        assert np.array_equal(eng.last_pred(), base["pred"])
        same_as_baseline(c, base, label)
        assert c["mfma_block_products"] == base["c"]["mfma_block_products"]
        print("%s: early_exit_unit_chunks %d of %d tile_unit_chunks" % (label, c["early_exit_unit_chunks"], c["tile_unit_chunks"]))

    def expect(c):
        if opts.get("pair_mfma", 1):
            assert (c["wide_tiles"] > 0) == (plan == "tiles")
        else:
            assert c["mfma_block_products"] == 0 and c["tile_unit_chunks"] > 0
    c = decide(pkg, ref, opts, expect, label="%s/%s/%s" % (label, plan, variant), load=load, inspect=inspect, totals=TOTALS)
    if opts.get("pair_mfma", 1):
        retires_stages(variant, base, c, label)
    return c


@pytest.mark.parametrize("variant", VARIANTS)
def test_rows_counted_again_by_restrict_variants(gpu_pkg, variant):
    _restricted(gpu_pkg, "narrow", variant)


@pytest.mark.parametrize("variant", VARIANTS)
def test_restrict_variants_on_the_bit_plane_engine(gpu_pkg, variant):
    """"pair_mfma" 0: the checkpoint slots travel with the rows and the checkpoint chunks are frozen from the matrix-mode plan the rows were
    loaded under.  The decisions are asserted.  early_exit_unit_chunks is printed, not asserted: observed 0 of 13,840 tile_unit_chunks on both
    variants, as expected of checkpoint chunks frozen from a matrix-mode plan, which has none."""
    _restricted(gpu_pkg, "narrow", variant, options={"pair_mfma": 0, "wide_min_reach": 1e9}, label="restricted/bit-planes")


# ---------------------------------------------------------------- the same on the tiles
def test_phased_rows_on_the_tiles(gpu_pkg):
    """m = 1,500, window 600, late LD 37 rows back: hap images hold no het code -- an operand mix the diagonal and corner bodies of
    pair_mfma_wide_kernel have not been fed by any other test"""
    pkg = gpu_pkg
    ref, base = _phased(pkg, "tiles", "complete")
    assert not (ref.raw_for_stats == 1).any()
    check_form(pkg, ref, base, "tiles", "complete", _phased_host_load, "phased_host", inspect=_phased_inspect)


def test_rows_counted_in_place_on_the_tiles(gpu_pkg):
    _in_place(gpu_pkg, "tiles", "complete")


def test_restricted_rows_on_the_tiles(gpu_pkg):
    _restricted(gpu_pkg, "tiles", "complete")


def test_zz_nothing_was_skipped_here_either():
    """as test_pair_decisions.test_zz_nothing_was_skipped: over this file, baselines included"""
    print("pairs compared in this file: %d over %d engine runs (sum of their candidate_pairs: %d)" % (TOTALS["compared"], TOTALS["engines"], TOTALS["candidate_pairs"]))
    assert TOTALS["compared"] == TOTALS["candidate_pairs"] > 0
