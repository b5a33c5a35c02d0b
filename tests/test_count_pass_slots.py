"""Every checkpoint slot of every count-pass form against numpy.

The pair kernels retire products at checkpoints on the strength of per-variant numbers the count pass wrote: codes_kernel
(ldp_codes.hip) on the code image, prepare_kernel + cp_gen_fix_kernel (ldp_kernels.hip) on bit-planes.  Each of the two launchers
picks one of nine instantiations by row length.  Until now a slot could only show as a pair dropped at a checkpoint, and only in
the 128 x 4 / 128 x 7 band; here LdPruneEngine.cp_stats() (ldp_debug_get_cp_stats) brings the raw records back and every slot of
every form is compared with ldtools.cp_reference -- numpy over the codes of the final image row (tests/test_cp_reference.py checks
that reference without a GPU) -- for 16 rows per case that are chosen for the edges of the pass (ldtools.CP_ROW_KINDS), at row
lengths one sample into a band (a 1-sample tail unit followed by seven padding units) and exactly at a band's end, through every
way rows reach the image.  Which form ran is asserted from ldp_debug_get_count_pass, the thresholds restated here; the last test
asserts that all 9 + 9 were seen.

Per variant: the integer slots bit for bit (gen on the code image, cp_gen on bit-planes: that array's complete rows come from
prepare_kernel, the others from cp_gen_fix_kernel); the integers a checkpoint recovers from a and b; S exactly; the doubles within
what csrc/ldp_pair_device.h ("FP64 error budget") grants the stored slots -- 2e-9 absolute on the remainder slots at N <= 4e6 --
and 1e-9 relative on the whole-row b, three orders inside cp_tv_scale's 1e-6 margin; the flag of the whole-row gen slot; the
records against the oracle's major allele; four rows of the image as bit-planes.  The largest distance in ulp between a stored
double and the reference's is printed per kernel by the last test.

What cannot be reached: map_rows() hands rows back in the input's orientation and clears their flags (unflip_rows_kernel), so a row
counted in place after a rewrite is read with inv_in = 0 whatever it was before; rows that ARE read inverted in place (inv_in) are
those of restrict_variants(), whose major allele cannot change.  Both are run here; inv_in together with flip_now has no caller.
Rows inside the image and the orient_rows option exist on the code image only."""
import ctypes

import numpy as np
import pytest

import ldtools as T
from test_pair_decisions_inputs import BED, SWAP, device_buffer, odd_stride, row_bytes_of, tail_garbage

pytestmark = pytest.mark.gpu

R2 = 0.5
WINDOW = 100
ABS_REMAINDER = 2e-9    # ldp_pair_device.h: "a few ulp of relative error at a magnitude <= N, i.e. <= 2e-9 each"
REL_WHOLE_B = 1e-9

CODES_N = (1537, 2048, 2049, 16384, 16385, 32769, 57344, 57345, 65537, 131073, 262145, 524288, 524289, 1048577, 4000000)
PREPARE_N = tuple(sorted(CODES_N + (49152, 49153)))
EXTRA_N = (1537, 65537, 1048577)
FEWER_CHECKPOINTS = ((1537, 0.1, 1), (2049, 0.2, 2), (65537, 0.1, 4))
CODES_FORMS = ((128, 2), (128, 4), (128, 7), (128, 8), (128, 16), (256, 16), (512, 16), (1024, 16), (1024, 0))
PREPARE_FORMS = ((128, 2), (128, 4), (128, 6), (128, 8), (128, 16), (256, 16), (512, 16), (1024, 16), (1024, 0))

SEEN = {"codes": set(), "prepare": set()}
ULP = {"codes": 0, "prepare": 0}
SLOTS = {"codes": 0, "prepare": 0}
_ROWS = {}


def expected_form(kernel, n):
    """launch_codes / launch_prepare restated: 16-byte units of the image row = pairs of plane dwords = 8 per 512-sample chunk"""
    units = 8 * ((n + 511) // 512)
    for threads, iters in (CODES_FORMS if kernel == "codes" else PREPARE_FORMS)[:-1]:
        if units <= threads * iters:
            return threads, iters
    return 1024, 0


def rows_of(n, r2=R2):
    """the case's raw rows, cached per row length (and checkpoint placement); the two largest lengths take the 14 named kinds only"""
    key = (n, r2)
    if key not in _ROWS:
        raw = T.cp_test_rows(n, r2, count=16 if n < 1000000 else 14)
        raw.setflags(write=False)
        _ROWS[key] = raw
    return _ROWS[key]


def phased_rows_of(n):
    """(raw codes (M, S), phaseinfo, haplotype columns (M, 2 S)) with 2 S = n + 1 haplotypes: one haplotype pair into the band's first chunk"""
    key = ("phased", n)
    if key not in _ROWS:
        s = (n + 1) // 2
        raw = rows_of(n)[:, :s]
        info = ((np.random.default_rng(n).random(raw.shape) < 0.5) & (raw == 1)).astype(np.uint8)
        cols = T.hap_raw_codes(raw, info)
        cols.setflags(write=False)
        _ROWS[key] = (raw, info, cols)
    return _ROWS[key]


def oriented_of(cols, n):
    """(the oracle's ALT-is-major flags, the rows oriented on their major allele) of a case's columns, computed once per array"""
    key = ("oriented", id(cols))
    if key not in _ROWS:
        inv, _, altmaj = T.oracle_prepare(cols)
        altmaj = altmaj.astype(bool)
        major = np.where(altmaj[:, None], SWAP[cols], cols)
        assert np.array_equal(T.unpack_2bit(inv, n), major)
        _ROWS[key] = (cols, altmaj, major)      # (cols is kept alive with its id)
    return _ROWS[key][1:]


def reference_of(cols, n, r2, inverted):
    """ldtools.cp_reference over the image rows -- cols with 0 <-> 2 swapped where `inverted` --, computed once and left unchanged"""
    inverted = np.asarray(inverted, dtype=bool)
    key = ("reference", id(cols), r2, inverted.tobytes())
    if key not in _ROWS:
        altmaj, major = oriented_of(cols, n)
        image = major if np.array_equal(inverted, altmaj) else np.where(inverted[:, None], SWAP[cols], cols)
        ref = T.cp_reference(image, n, T.checkpoint_chunks(n, r2), r2)
        for v in ref.values():
            v.setflags(write=False)
        _ROWS[key] = (cols, ref)
    return _ROWS[key][1]


def new_engine(pkg, n, m, r2, options):
    eng = pkg.LdPruneEngine(n, WINDOW, 1, False, r2, order=2, device=0)
    for k, v in options.items():
        eng.set_option(k, v)
    eng.set_variants(np.zeros(m, dtype=np.uint32), None)
    return eng


def ordered(x):
    """float64 -> int64 that orders like the doubles (the distance of two of them = their distance in ulp)"""
    i = np.ascontiguousarray(x, dtype=np.float64).view(np.int64)
    return np.where(i < 0, -(i & np.int64(0x7fffffffffffffff)), i)


def check_slots(pkg, eng, cols, n, r2, kernel, orient, label):
    """every slot of the engine's rows against the reference over `cols`, the image's columns in the input's orientation"""
    m = cols.shape[0]
    chunks = T.checkpoint_chunks(n, r2)
    altmaj, major = oriented_of(cols, n)

    # ---- which form ran
    is_codes, threads, iters = eng.count_pass()
    assert is_codes == (kernel == "codes"), label
    assert (threads, iters) == expected_form(kernel, n), (label, threads, iters)
    SEEN[kernel].add((threads, iters))

    st = eng.cp_stats()
    assert st["n_checkpoints"] == len(chunks) and st["chunks"][:len(chunks)].tolist() == chunks, (label, st["chunks"], chunks)
    assert (st["chunks"][len(chunks):] == T.CP_UNUSED).all(), label

    # ---- the records: the oracle's major allele, the counts of the major-allele-oriented row
    recs = eng.variant_recs()
    plus, minus, calls = (major == 0).sum(1), (major == 2).sum(1), (major != 3).sum(1)
    assert np.array_equal(recs["flags"] & 1, altmaj.astype(np.uint32)), label
    assert np.array_equal(recs["nm_ct"], calls) and np.array_equal(recs["sum"], plus - minus) and np.array_equal(recs["ssq"], plus + minus), label
    mono = ((plus == 0) & (minus == 0)) | (plus == calls) | (minus == calls)
    assert np.array_equal((recs["flags"] >> 1) & 1, mono.astype(np.uint32)) and np.array_equal((recs["flags"] >> 2) & 1, (calls != n).astype(np.uint32)), label
    stored_inverted = ((recs["flags"] >> 3) & 1).astype(bool)
    # the image's orientation: the code image stores ALT-major rows inverted iff the engine orients; bit-planes are major-allele-oriented
    assert np.array_equal(stored_inverted, altmaj & bool(orient) if kernel == "codes" else np.zeros(m, dtype=bool)), label
    ref = reference_of(cols, n, r2, stored_inverted if kernel == "codes" else altmaj)

    # ---- integer slots, bit for bit
    if kernel == "codes":
        gen = st["gen"]
        for f, whole, rest in (("nm_r", "calls", "calls_r"), ("zs_r", "zs", "zs_r"), ("zq_r", "zq", "zq_r")):
            assert np.array_equal(gen[f][:, 0], ref[whole]), (label, f, "whole row", gen[f][:, 0], ref[whole])
            for k in range(T.CP_GEN_CHECKPOINTS):
                want = ref[rest][:, T.CP_GEN_FIRST + k]
                assert np.array_equal(gen[f][:, 1 + k], want), (label, f, "remainder", k, gen[f][:, 1 + k], want)
        assert np.array_equal(gen["pad"][:, 0], (altmaj ^ stored_inverted).astype(np.uint32)), (label, "flag")
        assert not gen["pad"][:, 1:].any(), label
    else:
        cg = st["cp_gen"]
        for f, rest in (("nm_r", "calls_r"), ("zs_r", "zs_r"), ("zq_r", "zq_r")):
            assert np.array_equal(cg[f], ref[rest]), (label, "cp_gen", f, cg[f], ref[rest])
        assert not cg["pad"].any(), label

    # ---- the doubles
    a, b = st["cp"]["a"], st["cp"]["b"]
    assert np.array_equal(a[:, 5], ref["S"].astype(np.float64)), (label, "S", a[:, 5], ref["S"])
    s_r, hom_r, _ = T.cp_recover(a[:, :5], b[:, :5], n, chunks)
    assert np.array_equal(s_r, ref["s_r"]), (label, "s_r recovered", s_r, ref["s_r"])
    assert np.array_equal(hom_r, ref["hom_r"]), (label, "hom_r recovered", hom_r, ref["hom_r"])
    assert np.array_equal(np.sign(a[:, :5]), np.sign(ref["s_r"])), label
    assert (b >= 0).all(), label
    worst = int(max(np.abs(ordered(a) - ordered(ref["a"])).max(), np.abs(ordered(b) - ordered(ref["b"])).max()))
    err_a, err_b = np.abs(a[:, :5] - ref["a"][:, :5]).max(), np.abs(b[:, :5] - ref["b"][:, :5]).max()
    rel = np.abs(b[:, 5] - ref["b"][:, 5]) / np.maximum(ref["b"][:, 5], 1e-300)
    print("%s: <%d, %d> %d checkpoints; largest error a %.3g b %.3g, whole-row b relative %.3g; %d ulp" % (label, threads, iters, len(chunks), err_a, err_b, rel.max(), worst))
    ULP[kernel] = max(ULP[kernel], worst)
    SLOTS[kernel] += 12 * m
    assert err_a <= ABS_REMAINDER and err_b <= ABS_REMAINDER, (label, err_a, err_b)
    assert (rel <= REL_WHOLE_B).all(), (label, rel)
    assert not a[:, len(chunks):5].any() and not b[:, len(chunks):5].any(), (label, "unused slots")

    # ---- four rows of the image
    for v in (0, 1, 6, m - 1):
        hom, r2h = eng.planes(v)
        want_hom, want_r2h = T.major_oriented_planes(cols[v], bool(altmaj[v]))
        assert np.array_equal(hom, want_hom) and np.array_equal(r2h, want_r2h), (label, v)


def options_of(kernel, **more):
    opts = {"pair_mfma": 0} if kernel == "prepare" else {}
    opts.update(more)
    return opts


def run_host_case(pkg, kernel, n, enc, r2=R2, options=None, label=None):
    cols = rows_of(n, r2)
    opts = options_of(kernel) if options is None else options
    eng = new_engine(pkg, n, cols.shape[0], r2, opts)
    if enc == "ref":
        eng.load_genotypes_host(0, T.pack_2bit(cols), pkg.LDP_GENO_REF)
    else:
        eng.load_genotypes_host(0, row_bytes_of(BED[cols]), pkg.LDP_GENO_BED)
    check_slots(pkg, eng, cols, n, r2, kernel, opts.get("orient_rows", 1), label or "%s/%s_host/%d" % (kernel, enc, n))
    eng.close()


# ---------------------------------------------------------------- REF and BED rows from host memory, every row length
@pytest.mark.parametrize("enc", ["ref", "bed"])
@pytest.mark.parametrize("n", CODES_N)
def test_codes_kernel_slots(gpu_pkg, n, enc):
    run_host_case(gpu_pkg, "codes", n, enc)


@pytest.mark.parametrize("enc", ["ref", "bed"])
@pytest.mark.parametrize("n", PREPARE_N)
def test_prepare_kernel_slots(gpu_pkg, n, enc):
    """"pair_mfma" 0: bit-planes, prepare_kernel's own third boundary (128 x 6: 49,152 | 49,153)"""
    run_host_case(gpu_pkg, "prepare", n, enc)


@pytest.mark.parametrize("enc", ["ref", "bed"])
def test_bit_plane_fallback_above_the_matrix_pipe(gpu_pkg, enc):
    """4,000,001 founders with default options: one more than the matrix pipe accepts, the engine falls back to bit-planes by itself"""
    assert gpu_pkg.lib().ldp_matrix_pipe_max_founders() == 4000000
    run_host_case(gpu_pkg, "prepare", 4000001, enc, options={}, label="fallback/%s_host/4000001" % enc)


# ---------------------------------------------------------------- fewer than five checkpoints
@pytest.mark.parametrize("kernel", ["codes", "prepare"])
@pytest.mark.parametrize("n,r2,want", FEWER_CHECKPOINTS)
def test_fewer_checkpoints(gpu_pkg, kernel, n, r2, want):
    """unused slots (checkpoint_chunk = 0xffffffff); with one or two checkpoints the six-product kernel's remainders (checkpoints 2, 3) are unused too"""
    assert len(T.checkpoint_chunks(n, r2)) == want
    run_host_case(gpu_pkg, kernel, n, "ref", r2=r2, label="%s/%d checkpoints/%d" % (kernel, want, n))


# ---------------------------------------------------------------- the other ways in, at three lengths
@pytest.mark.parametrize("kernel", ["codes", "prepare"])
@pytest.mark.parametrize("n", EXTRA_N)
def test_unaligned_device_rows(gpu_pkg, kernel, n):
    """rows in device memory at base + 1 and an odd stride: byte loads, every unit through the rolled loop; garbage between the rows and behind the last sample"""
    pkg = gpu_pkg
    cols = rows_of(n)
    rows = row_bytes_of(cols)
    stride = odd_stride(rows.shape[1])
    assert stride % 2 == 1
    eng = new_engine(pkg, n, cols.shape[0], R2, options_of(kernel))
    dev, ptr = device_buffer(rows, stride, 1, tail_garbage(n))
    eng.load_genotypes_device(0, cols.shape[0], ptr, stride, pkg.LDP_GENO_REF)
    check_slots(pkg, eng, cols, n, R2, kernel, 1, "%s/device_unaligned/%d" % (kernel, n))
    eng.close()
    del dev


@pytest.mark.parametrize("kernel", ["codes", "prepare"])
@pytest.mark.parametrize("n", EXTRA_N)
def test_phased_rows(gpu_pkg, kernel, n):
    """LDP_GENO_REF | LDP_GENO_PHASED: n + 1 haplotypes, the image's columns are ldtools.hap_raw_codes'"""
    pkg = gpu_pkg
    raw, info, cols = phased_rows_of(n)
    s = raw.shape[1]
    eng = new_engine(pkg, 2 * s, raw.shape[0], R2, options_of(kernel))
    rows = pkg.pack_phased_rows(T.pack_2bit(raw).view(np.uint8).reshape(raw.shape[0], -1), info, s)
    eng.load_genotypes_host(0, rows, pkg.LDP_GENO_REF | pkg.LDP_GENO_PHASED)
    check_slots(pkg, eng, cols, 2 * s, R2, kernel, 1, "%s/phased/%d" % (kernel, 2 * s))
    eng.close()


@pytest.mark.parametrize("n", EXTRA_N)
def test_rows_kept_as_the_input_had_them(gpu_pkg, n):
    """"orient_rows" 0: nothing is stored inverted, the whole-row flag says which rows count the minor allele"""
    run_host_case(gpu_pkg, "codes", n, "ref", options={"orient_rows": 0}, label="codes/orient_rows 0/%d" % n)


def _write_in_place(pkg, eng, cols, n):
    import torch
    rb = (n + 3) // 4
    for length, first in eng.subcontigs():
        ptr, stride = eng.map_rows(first, length)
        assert stride % 64 == 0 and stride >= rb
        with pytest.raises(pkg.LdpError) as ei:
            eng.cp_stats(first, length)                                # mapped rows count as not loaded
        assert ei.value.code == pkg.LDP_ERR_STATE
        new = np.full((length, stride), 0xA5, dtype=np.uint8)          # garbage in the padding: the engine's to fill
        new[:, :rb] = row_bytes_of(cols[first:first + length])
        new[:, rb - 1] |= tail_garbage(n)
        dev = torch.from_numpy(new).cuda()
        torch.cuda.synchronize()
        assert pkg.hip_memcpy_dtod(ptr, dev.data_ptr(), length * stride) == 0
        torch.cuda.synchronize()     # (a device-to-device hipMemcpy returns before it is done, and the engine's stream does not wait for the null stream)
        eng.load_genotypes_device(first, length, ptr, stride, pkg.LDP_GENO_REF)


@pytest.mark.parametrize("n", EXTRA_N)
def test_rows_counted_in_place_and_again_with_the_other_allele_major(gpu_pkg, n):
    """map_rows: rows written into the image and counted where they lie (ALT-major rows are inverted in place: flip_now); mapped again
    and every row rewritten with its alleles swapped, so that every row that was stored inverted no longer is and the others now are"""
    pkg = gpu_pkg
    cols = rows_of(n)
    eng = new_engine(pkg, n, cols.shape[0], R2, {})
    _write_in_place(pkg, eng, cols, n)
    check_slots(pkg, eng, cols, n, R2, "codes", 1, "codes/in_place/%d" % n)
    before = (eng.variant_recs()["flags"] >> 3) & 1
    swapped = SWAP[cols]
    _write_in_place(pkg, eng, swapped, n)
    check_slots(pkg, eng, swapped, n, R2, "codes", 1, "codes/in_place_rewritten/%d" % n)
    after = (eng.variant_recs()["flags"] >> 3) & 1
    changed = before != after
    assert changed.sum() >= cols.shape[0] - 3 and (before[changed] == 1).any() and (after[changed] == 1).any()   # (all but the tie, the all-het and the all-missing row)
    eng.close()


@pytest.mark.parametrize("n", EXTRA_N)
def test_rows_counted_again_where_they_lie_inverted(gpu_pkg, n):
    """restrict_variants: the kept rows are compacted and counted again in place, the ALT-major ones as they are stored -- inverted (inv_in)"""
    pkg = gpu_pkg
    cols = rows_of(n)
    m = cols.shape[0]
    keep = np.ones(m + m // 2, dtype=bool)
    keep[1::3] = False
    assert int(keep.sum()) == m
    rows = np.empty((len(keep), n), dtype=np.uint8)
    rows[keep] = cols
    rows[~keep] = SWAP[cols[:int((~keep).sum())]]
    eng = pkg.LdPruneEngine(n, WINDOW, 1, False, R2, order=2, device=0)
    eng.set_variants_matrix(len(keep))
    eng.load_genotypes_host(0, T.pack_2bit(rows), pkg.LDP_GENO_REF)
    eng.restrict_variants(keep, np.zeros(m, dtype=np.uint32), None)
    check_slots(pkg, eng, cols, n, R2, "codes", 1, "codes/restricted/%d" % n)
    eng.close()


# ---------------------------------------------------------------- the accessor's refusals
def test_accessor_states(gpu_pkg):
    pkg = gpu_pkg
    n = 1537
    cols = rows_of(n)
    m = cols.shape[0]
    eng = new_engine(pkg, n, m, R2, {})
    for call in (eng.cp_stats, eng.count_pass):
        with pytest.raises(pkg.LdpError) as ei:
            call()                                                      # nothing on the device yet
        assert ei.value.code == pkg.LDP_ERR_STATE
    eng.load_genotypes_host(0, T.pack_2bit(cols[:5]), pkg.LDP_GENO_REF)
    assert eng.cp_stats(0, 5)["cp"].shape == (5, 6) and eng.cp_stats(2, 3)["cp_gen"].shape == (3, 5)
    whole = eng.cp_stats(0, 5)
    part = eng.cp_stats(2, 3)
    assert whole["cp"][2:].tobytes() == part["cp"].tobytes() and whole["gen"][2:].tobytes() == part["gen"].tobytes()
    with pytest.raises(pkg.LdpError) as ei:
        eng.cp_stats(0, 6)                                              # row 5 is not loaded
    assert ei.value.code == pkg.LDP_ERR_STATE
    with pytest.raises(pkg.LdpError) as ei:
        eng.cp_stats(0, m + 1)
    assert ei.value.code == pkg.LDP_ERR_INVALID
    # NULL outputs
    n_cp = np.zeros(1, dtype=np.uint32)
    assert pkg.lib().ldp_debug_get_cp_stats(eng._h, 0, 5, None, None, None, n_cp.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))) == 0
    assert int(n_cp[0]) == len(T.checkpoint_chunks(n, R2))
    eng.close()
    # a sharded engine
    eng = pkg.LdPruneEngine(n, WINDOW, 1, False, R2, order=2, device=0)
    eng.set_variants(np.repeat(np.arange(2, dtype=np.uint32), m // 2), None)
    eng.set_shard(0, 2)
    eng.load_genotypes_host(0, T.pack_2bit(cols), pkg.LDP_GENO_REF)
    with pytest.raises(pkg.LdpError) as ei:
        eng.cp_stats(0, 1)
    assert ei.value.code == pkg.LDP_ERR_UNSUPPORTED
    eng.close()


def test_zz_every_form_was_seen():
    """all nine instantiations of each launcher ran in this file; the largest distance between a stored double and the reference's"""
    for kernel in ("codes", "prepare"):
        print("%s: forms seen %s; %d slots compared, largest distance %d ulp%s" % (kernel, sorted(SEEN[kernel]), SLOTS[kernel], ULP[kernel], " (bit-equal)" if ULP[kernel] == 0 else ""))
    assert SEEN["codes"] == set(CODES_FORMS)
    assert SEEN["prepare"] == set(PREPARE_FORMS)
