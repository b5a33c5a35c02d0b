"""The refusals the post-load passes share (resident_runs()): code and text of every call that is wrong in one way, for
ldp_sample_missing_counts, ldp_sample_het_counts, ldp_king_counts_block, ldp_king_block_hits and ldp_hwe_ln_pvals.  No GPU: planning is host
work, and every refusal up to "nothing is loaded" comes before the first HIP call.  (The refusals of loaded engines -- rows loaded as
LDP_GENO_PHASED, partly loaded ranges, LDP_GENO_INVERSE rows under HWE -- are in the GPU tests of the five calls.)"""
import ctypes

import numpy as np
import pytest

N = 40                                   # founders
CHR = [0] * 5 + [1] + [2] * 6            # variant 5 is alone on its chromosome: no subcontig, no row
M = len(CHR)

# public name in the messages, the call on (engine, first, n), reads the 2-bit image
ENTRIES = {
    "sample_missing": ("ldp_sample_missing_counts()", lambda e, first, n: e.sample_missing_counts(first, n), True),
    "sample_het": ("ldp_sample_het_counts()", lambda e, first, n: e.sample_het_counts(first, n), True),
    "king_dense": ("ldp_king_counts_block()", lambda e, first, n: e.king_counts_block(0, N, 0, N, first, n), True),
    "king_hits": ("ldp_king_block_hits()", lambda e, first, n: e.king_block_hits(0.1, 0, N, 0, N, first, n, capacity=16), True),
    "hwe": ("ldp_hwe_ln_pvals()", lambda e, first, n: e.hwe_ln_pvals(first, n), False),
}


def new_engine(pkg, options=None, plan=True):
    eng = pkg.LdPruneEngine(N, 50, 5, False, 0.2, order=2, device=0)
    for name, value in (options or {}).items():
        eng.set_option(name, value)
    if plan:
        eng.set_variants(np.array(CHR, dtype=np.uint32), np.arange(M, dtype=np.uint32) * 1000 + 1)
    return eng


def refused(pkg, eng, call, first, n, code, text):
    with pytest.raises(pkg.LdpError) as err:
        call(eng, first, n)
    assert err.value.code == code, str(err.value)
    assert text in str(err.value), str(err.value)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_every_refusal_before_the_first_load(pkg, entry):
    who, call, reads_image = ENTRIES[entry]
    eng = new_engine(pkg, plan=False)
    refused(pkg, eng, call, 0, 1, pkg.LDP_ERR_STATE, "ldp_set_variants*() and the loads first")
    eng.close()
    eng = new_engine(pkg)
    refused(pkg, eng, call, 11, 2, pkg.LDP_ERR_INVALID, "variant range out of bounds")
    refused(pkg, eng, call, 0, M, pkg.LDP_ERR_STATE, "a variant of the range has no row in this engine (its plan did not own it)")
    refused(pkg, eng, call, 0, 5, pkg.LDP_ERR_STATE, "nothing is loaded")
    eng.set_shard(0, 2)
    refused(pkg, eng, call, 0, 5, pkg.LDP_ERR_UNSUPPORTED, who + " on a sharded engine (ldp_set_shard with world > 1)")
    eng.close()
    eng = new_engine(pkg, {"pair_mfma": 0})
    if reads_image:
        refused(pkg, eng, call, 0, 5, pkg.LDP_ERR_UNSUPPORTED, who + " on an engine that keeps bit-planes (no 2-bit code image)")
    else:
        # the records are read, not the image: bit-plane engines are served
        refused(pkg, eng, call, 0, 5, pkg.LDP_ERR_STATE, "nothing is loaded")
    eng.close()


def test_an_empty_range_zeroes_the_outputs(pkg):
    L = pkg.lib()
    eng = new_engine(pkg)
    u32, u64 = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
    for first in (0, 5, M):
        out = np.full(N, 7, dtype=np.uint32)
        got = eng.sample_missing_counts(first, 0, out=out)
        assert len(got) == N and not out.any()
        het, mis, mw = np.full(N, 7, dtype=np.uint32), np.full(N, 7, dtype=np.uint32), np.full(N, 7, dtype=np.uint64)
        weight = np.zeros(1, dtype=np.uint64)
        assert L.ldp_sample_het_counts(eng._h, first, 0, None, weight.ctypes.data_as(u64), het.ctypes.data_as(u32), mis.ctypes.data_as(u32), mw.ctypes.data_as(u64)) == pkg.LDP_OK
        assert not het.any() and not mis.any() and not mw.any()
        h, m, w = eng.sample_het_counts(first, 0)
        assert len(h) == N and len(m) == N and w is None and not h.any() and not m.any()
        # a 3 x 5 block in rows of 6 elements: the block is zeroed, the sixth element of a row is not the call's
        dense = np.full((3, 6, 5), 7, dtype=np.uint32)
        assert pkg.KING_COUNTS_DTYPE.itemsize == 20
        assert L.ldp_king_counts_block(eng._h, first, 0, None, 10, 3, 2, 5, dense.ctypes.data_as(ctypes.c_void_p), 6) == pkg.LDP_OK
        assert not dense[:, :5].any() and (dense[:, 5] == 7).all()
        block = eng.king_counts_block(10, 3, 2, 5, first, 0)
        assert block.shape == (3, 5) and not any(block[f].any() for f in block.dtype.names)
        # (the hit form of a block with pairs launches its hit kernel over the zero counts; a block without a pair ends before the device)
        hits, found = eng.king_block_hits(0.1, 0, 1, 0, N, first, 0, capacity=16)
        assert len(hits) == 0 and found == 0
        ln_p, flags = eng.hwe_ln_pvals(first, 0)
        assert len(ln_p) == 0 and len(flags) == 0
    eng.close()
