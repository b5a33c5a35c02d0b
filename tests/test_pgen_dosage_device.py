"""The allele dosage sums of ldp_load_pgen_records (pgen_dosage_kernel, ldp_pgen_decode.hip; ldp_get_dosage_sums): what the host's
ldp_pgen_dosage_sums computes from a second read of the file, computed on the device where the record's bytes and its decoded row lie
side by side.  All integers, compared exactly: against numpy's restatement (test_pgen_dosage.expected_sums) and against the host reader,
for records written by the test (every dosage kind, phase tracks in front, sample counts at which the kernel changes behaviour) and for a
file the reference wrote.

Sample counts: 2 (fewer samples than one code dword; ldp_create refuses fewer than two founders -- the reference's own rule,
plink2_ld.cc:2537 -- so a file of ONE sample cannot reach any load that computes sums, and 2 is the smallest count that can), the
32-sample word edge (31, 32, 33), 37, 300 (2-byte sample ids), 4097 (more code dwords than threads), 70001 (3-byte sample ids)."""
import os

import numpy as np
import pytest

import ldtools as T
from test_pgen_dosage import dosage_records, expected_sums, make_case

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pgen")
SAMPLE_CTS = [2, 31, 32, 33, 37, 300, 4097, 70001]

_cases = {}


def handmade(n, first_index, seed):
    """Six variants appended behind make_case's draw, so that every sample count has the edges the kernel can trip over whatever the
    draw gave.  dosage_records() puts a phase track in front of variant v when it has a het call and v % 3 != 2 -- implicit
    phasepresent for v % 3 == 0, explicit for v % 3 == 1 --, hence first_index % 3 == 0."""
    assert first_index % 3 == 0
    rng = np.random.default_rng(seed)

    def row(het_ct):
        r = rng.choice(np.array([0, 2], dtype=np.uint8), size=n)
        r[0] = 3                                   # a sample without a hardcall
        if n > 1:
            hets = 1 + rng.choice(n - 1, size=min(het_ct, n - 1), replace=False)
            r[hets] = 1
        return r

    raw = np.stack([row(7), row(8), row(3), row(8), row(7), row(5)])
    dos = np.full((6, n), -1, dtype=np.int64)
    kinds = np.array([3, 1, 1, 2, 3, 0])             # (the last one: no dosage track)
    value = lambda size: rng.integers(0, 32769, size=size)
    dos[0] = value(n)                              # bit array, all set: sample 0 has a dosage and no hardcall
    # (variant 1: a list with zero entries)
    ids = np.sort(rng.choice(n, size=min(n, 150), replace=False))
    ids[0] = 0
    dos[2, ids] = value(len(ids))                  # a list of more than 64 entries where the file has the samples for one
    dos[3] = np.where(raw[3] != 3, value(n), -1)   # one value per sample: every called sample has one ...
    dos[3, 0] = 7000                               # ... and one without a call
    some = rng.random(n) < 0.2
    dos[4] = np.where(some, value(n), -1)          # a sparse bit array
    return raw, dos, kinds


def build_case(n):
    """(raw, dos, kinds, records, vrtypes) of one sample count, built once"""
    if n not in _cases:
        m = 60 if n < 1000 else 12
        raw, dos, kinds, _ = make_case(m, n, n)
        hraw, hdos, hkinds = handmade(n, m, 1000 + n)
        raw, dos, kinds = np.concatenate([raw, hraw]), np.concatenate([dos, hdos]), np.concatenate([kinds, hkinds])
        _, info = T.synth_phase(raw, n + 1)
        records, vrtypes = dosage_records(raw, dos, kinds, info)
        for a in (raw, dos, kinds, vrtypes):
            a.setflags(write=False)
        _cases[n] = (raw, dos, kinds, records, vrtypes)
    return _cases[n]


def header_len(m):
    blocks = (m + 65535) // 65536
    return 12 + 8 * blocks + 4 * m     # (ldtools.write_pgen_records: one type byte and a 3-byte length per record)


def check_inputs(n):
    """The edges are in the inputs -- seen by numpy alone, no product code involved."""
    raw, dos, kinds, records, vrtypes = build_case(n)
    m = len(records)
    assert {0, 1, 2, 3} <= set(kinds.tolist())
    starts = header_len(m) + np.concatenate([[0], np.cumsum([len(r) for r in records])[:-1]])
    value_ct = np.where(kinds == 2, n, (dos >= 0).sum(axis=1))
    in_file, in_record = set(), set()
    for v in range(m):
        if kinds[v] and value_ct[v]:
            in_record.add((len(records[v]) - 2 * int(value_ct[v])) & 1)   # (the values are the last thing in a record)
            in_file.add((int(starts[v]) + len(records[v]) - 2 * int(value_ct[v])) & 1)
    assert in_file == {0, 1} and in_record == {0, 1}, (in_file, in_record)
    het_ct = (raw == 1).sum(axis=1)
    phased = (vrtypes & 0x10) != 0
    implicit = phased & (np.arange(m) % 3 == 0)
    explicit = phased & (np.arange(m) % 3 == 1)
    assert implicit.any() and explicit.any()
    if n >= 9:
        for want in (0, 1):
            hit = (kinds > 0) & ((1 + het_ct) % 8 == want)
            assert (hit & implicit).any() and (hit & explicit).any(), want
    lists = kinds == 1
    entries = (dos >= 0).sum(axis=1)
    assert (lists & (entries == 0)).any()
    if n >= 65:
        assert (lists & (entries > 64)).any()
    assert ((kinds == 3) & (entries == n)).any()
    for k in (1, 2, 3):
        assert ((kinds == k)[:, None] & (dos >= 0) & (raw == 3)).any(), k   # a dosage without a hardcall, in every kind
    return raw, dos, kinds, records, vrtypes


@pytest.mark.parametrize("n", SAMPLE_CTS)
def test_the_handwritten_inputs_hold_the_edges(n):
    check_inputs(n)


def write_case(tmp_path, n, name="d"):
    raw, dos, kinds, records, vrtypes = check_inputs(n)
    prefix = str(tmp_path / name)
    m = len(records)
    T.write_pgen_records(prefix, records, vrtypes, n, ["1"] * m, np.arange(m) + 1)
    return prefix, raw, dos, kinds


def engine(pkg, founders, m):
    eng = pkg.LdPruneEngine(founders, 40, 1, False, 0.3, order=2, device=0)
    eng.set_variants(np.zeros(m, dtype=np.uint32), (np.arange(m, dtype=np.uint32) + 1) * 1000)
    return eng


def host_sums(f, m, mask=None):
    return [f.dosage_sums(v, mask) for v in range(m)]


def assert_sums(eng, want, kinds, what=""):
    ref, alt, has = eng.dosage_sums()
    assert np.array_equal(has, (kinds > 0).astype(np.uint8)), what
    for v in range(len(kinds)):
        if kinds[v]:
            assert (int(ref[v]), int(alt[v])) == want[v], (what, v, int(kinds[v]))
        else:
            assert (int(ref[v]), int(alt[v])) == (0, 0), (what, v)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SAMPLE_CTS)
def test_device_sums_of_handwritten_records(gpu_pkg, tmp_path, n):
    pkg = gpu_pkg
    prefix, raw, dos, kinds = write_case(tmp_path, n)
    m = len(kinds)
    f = pkg.PgenFile(prefix + ".pgen")
    everybody = np.ones(n, dtype=bool)
    want = [expected_sums(raw[v], dos[v], everybody) for v in range(m)]
    assert host_sums(f, m) == want
    # ---- every sample of the file
    eng = engine(pkg, n, m)
    eng.load_pgen_records(0, f)
    assert_sums(eng, want, kinds, "whole file")
    rows = f.read()
    hard = engine(pkg, n, m)
    hard.load_genotypes_host(0, rows, pkg.LDP_GENO_REF)
    recs_a, recs_b = eng.variant_recs(), hard.variant_recs()
    for name in ("nm_ct", "n_homref", "n_het", "n_homalt"):
        assert np.array_equal(recs_a[name], recs_b[name]), name      # (the rows stay the hardcalls)
    # ---- launches cut every 7 rows; rows assembled in global memory
    for option in ("decode_rows", "decode_no_lds"):
        e2 = engine(pkg, n, m)
        e2.set_option(option, 7 if option == "decode_rows" else 1)
        e2.load_pgen_records(0, f)
        assert_sums(e2, want, kinds, option)
        e2.close()
    # ---- the file's bytes already in device memory
    import torch
    ptr, nbytes = f.file_bytes()
    buf = torch.from_numpy(np.ctypeslib.as_array((pkg.ctypes.c_uint8 * nbytes).from_address(ptr)).copy()).cuda()
    e3 = engine(pkg, n, m)
    e3.load_pgen_records(0, f, location=pkg.LDP_MEM_DEVICE, device_bytes=buf.data_ptr())
    assert_sums(e3, want, kinds, "device-resident bytes")
    e3.close()
    # ---- a subset of the file's samples (founders among non-founders)
    sub = np.random.default_rng(n).random(n) < 0.7
    sub[:2] = True                                   # (an engine has at least two founders)
    keep = np.flatnonzero(sub).astype(np.uint32)
    want_sub = [expected_sums(raw[v], dos[v], sub) for v in range(m)]
    assert host_sums(f, m, sub) == want_sub
    e4 = engine(pkg, len(keep), m)
    e4.set_sample_map(n, keep)
    e4.load_pgen_records(0, f)
    assert_sums(e4, want_sub, kinds, "subset map")
    e4.release_device()                              # (the device's mask is rebuilt from the host's map; the sums went with the rows)
    assert not e4.dosage_sums()[2].any()
    e4.set_option("decode_rows", 7)
    e4.load_pgen_records(0, f)
    assert_sums(e4, want_sub, kinds, "subset map, after release_device")
    for e in (eng, hard, e4):
        e.close()
    f.close()


@pytest.mark.gpu
def test_device_sums_of_a_reference_written_file(gpu_pkg):
    """tests/golden/pgen/dosage_small.pgen: the reference's --dummy wrote it -- mixed main-track record types, LD-compressed ones
    included, dosage lists and bit arrays."""
    pkg = gpu_pkg
    f = pkg.PgenFile(os.path.join(GOLD, "dosage_small.pgen"))
    m, n = f.variant_ct, f.sample_ct
    assert m == 200
    recs, _ = f.record_index()
    vrtypes = np.array([int(recs[v].vrtype) for v in range(m)])
    assert ((vrtypes & 6) == 2).any() and {0x20, 0x60} <= set((vrtypes & 0x60).tolist())
    kinds = (vrtypes & 0x60) >> 5
    want = host_sums(f, m)
    for decode_rows in (0, 7):
        eng = engine(pkg, n, m)
        eng.set_option("decode_rows", decode_rows)
        eng.load_pgen_records(0, f)
        assert_sums(eng, want, kinds, decode_rows)
        eng.close()
    sub = np.random.default_rng(5).random(n) < 0.6
    eng = engine(pkg, int(sub.sum()), m)
    eng.set_sample_map(n, np.flatnonzero(sub).astype(np.uint32))
    eng.load_pgen_records(0, f)
    assert_sums(eng, host_sums(f, m, sub), kinds, "subset")
    eng.close()
    f.close()


@pytest.mark.gpu
def test_sums_follow_their_rows(gpu_pkg, tmp_path):
    """ldp_restrict_variants carries the entries to the new indices, a reload replaces them, ldp_set_variants clears them; loads that
    compute none report has == 0."""
    pkg = gpu_pkg
    n = 300
    prefix, raw, dos, kinds = write_case(tmp_path, n)
    m = len(kinds)
    everybody = np.ones(n, dtype=bool)
    want = [expected_sums(raw[v], dos[v], everybody) for v in range(m)]
    f = pkg.PgenFile(prefix + ".pgen")
    eng = pkg.LdPruneEngine(n, 40, 1, False, 0.3, order=2, device=0)
    with pytest.raises(pkg.LdpError):
        eng.dosage_sums(0, 1)                        # (no plan yet)
    eng.set_variants_matrix(m)
    assert not eng.dosage_sums()[2].any()
    eng.load_pgen_records(0, f)
    assert_sums(eng, want, kinds, "before")
    with pytest.raises(pkg.LdpError) as ei:
        eng.dosage_sums(m - 1, 2)
    assert ei.value.code == pkg.LDP_ERR_INVALID
    keep = np.random.default_rng(1).random(m) < 0.6
    kept = np.flatnonzero(keep)
    eng.restrict_variants(keep, np.zeros(len(kept), dtype=np.uint32), (kept.astype(np.uint32) + 1) * 1000)
    assert_sums(eng, [want[v] for v in kept], kinds[kept], "restricted")
    # a reload replaces: another file's records into the same rows, then plain rows
    raw2, dos2, kinds2, _ = make_case(len(kept), n, 77)
    records2, vrtypes2 = dosage_records(raw2, dos2, kinds2, None)
    T.write_pgen_records(str(tmp_path / "e"), records2, vrtypes2, n, ["1"] * len(kept), np.arange(len(kept)) + 1)
    f2 = pkg.PgenFile(str(tmp_path / "e.pgen"))
    eng.load_pgen_records(0, f2)
    assert_sums(eng, [expected_sums(raw2[v], dos2[v], everybody) for v in range(len(kept))], kinds2, "reloaded")
    with_track = int(np.flatnonzero(kinds2 > 0)[0])
    eng.load_genotypes_host(with_track, f2.read(with_track, 1), pkg.LDP_GENO_REF)
    has = eng.dosage_sums()[2]
    assert has[with_track] == 0 and int(has.sum()) == int((kinds2 > 0).sum()) - 1
    eng.set_variants_matrix(len(kept))
    assert not eng.dosage_sums()[2].any()
    eng.close()
    # several ALT alleles (the reference has no sums for such a record either), a map that is no plain subset
    multi = np.flatnonzero(kinds > 0)[[1, 4]]
    allele_cts = np.full(m, 2)
    allele_cts[multi] = 3
    e2 = engine(pkg, n, m)
    e2.load_pgen_records(0, f, allele_cts=allele_cts)
    ref, alt, has = e2.dosage_sums()
    only = (kinds > 0)
    only[multi] = False
    assert np.array_equal(has, only.astype(np.uint8))
    assert all((int(ref[v]), int(alt[v])) == want[v] for v in np.flatnonzero(only))
    e2.close()
    e3 = engine(pkg, n + 1, m)
    e3.set_sample_map(n, np.concatenate([np.arange(n), [0]]).astype(np.uint32))   # a sample twice
    e3.load_pgen_records(0, f)
    assert not e3.dosage_sums()[2].any()
    e3.close()
    f.close()
    f2.close()


@pytest.mark.gpu
def test_a_truncated_value_array_is_refused(gpu_pkg, tmp_path):
    """One deterministic case per dosage kind: the `length` of a middle record ends its value array three bytes early, while the bytes
    behind it -- the next records -- remain inside the uploaded span.  LDP_ERR_INVALID names the variant; the engine stays usable."""
    pkg = gpu_pkg
    n = 300
    prefix, raw, dos, kinds = write_case(tmp_path, n)
    m = len(kinds)
    f = pkg.PgenFile(prefix + ".pgen")
    recs, _ = f.record_index()
    ptr, nbytes = f.file_bytes()
    everybody = np.ones(n, dtype=bool)
    want = [expected_sums(raw[v], dos[v], everybody) for v in range(m)]
    eng = engine(pkg, n, m)
    for kind in (1, 2, 3):
        q = int([v for v in range(5, m - 5) if kinds[v] == kind and (dos[v] >= 0).sum() >= 2][0])
        cut = (pkg.ldp_pgen_rec * m)()
        for k in range(m):
            cut[k].offset, cut[k].length, cut[k].vrtype, cut[k].allele_ct = recs[k].offset, recs[k].length, recs[k].vrtype, 2
        cut[q].length = recs[q].length - 3
        rc = eng._L.ldp_load_pgen_records(eng._h, 0, m, pkg.ctypes.c_void_p(ptr), nbytes, pkg.LDP_MEM_HOST, cut, None, n, None)
        assert rc == pkg.LDP_ERR_INVALID, (kind, q)
        assert ("variant %d)" % q) in eng._L.ldp_last_error(eng._h).decode(), (kind, q)
        eng.load_pgen_records(0, f)
        assert_sums(eng, want, kinds, kind)
    eng.close()
    f.close()
