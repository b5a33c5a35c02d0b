"""What an engine computes must not depend on how often its device memory was released and built again: one engine goes through every path
that frees or moves device memory -- ldp_release_device(), a new plan on a loaded engine, ldp_restrict_variants(), ldp_destroy() -- and its
prune sets are compared with the CPU oracle's and a fresh engine's; the decode scratch of ldp_load_pgen_records() grows between two loads
of one engine; and the free device memory (hipMemGetInfo) after ten plan / load / run / release cycles is what it was after the first.

ldp_restrict_variants() takes an engine whose rows are resident and on which no pair work was queued, and a load into a windowed plan
queues pair work: so run 3 is reached through ldp_set_variants_matrix() + load on the same engine (one more new plan over the old one's
device memory), not straight from run 2."""
import functools
import os

import numpy as np
import pytest

import ldtools as T
from test_pgen_device_decode import assert_same_rows, engine
from test_pgen_reader import GOLD

pytestmark = pytest.mark.gpu

N_RAW, M, WINDOW, STEP, R2 = 256, 600, 50, 5, 0.2
CHR_IDX = (np.arange(M) >= 330).astype(np.uint32)
BPS = (1000 + 100 * np.arange(M)).astype(np.uint32)   # (count windows: the oracle's interface wants positions, nothing reads them)
KEEP = (np.arange(M) % 2) == 0


@functools.lru_cache(maxsize=None)
def raw_codes():
    raw = T.synth_raw_codes(M, N_RAW, seed=23, missing_rate=0.02)
    raw.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def oracle_removed(subset_key, restricted):
    """the CPU oracle's prune set over the engine's columns (all samples, or the sample map's subset) and rows (all, or the kept ones)"""
    cols = raw_codes() if subset_key is None else raw_codes()[:, np.array(subset_key)]
    rows = cols[KEEP] if restricted else cols
    chr_idx, bps = (CHR_IDX[KEEP], BPS[KEEP]) if restricted else (CHR_IDX, BPS)
    inv, mf, _ = T.oracle_prepare(rows)
    removed, _ = T.oracle_indep_pairwise(inv, rows.shape[1], chr_idx, bps, mf, WINDOW, STEP, False, R2, order=2)
    return removed


class Lifecycle:
    def __init__(self, pkg, options, subset):
        self.pkg, self.options, self.subset = pkg, options, subset
        self.founders = N_RAW if subset is None else len(subset)

    def new_engine(self):
        eng = self.pkg.LdPruneEngine(self.founders, WINDOW, STEP, False, R2, order=2, device=0)
        for name, value in self.options.items():
            eng.set_option(name, value)
        if self.subset is not None:
            eng.set_sample_map(N_RAW, self.subset, None)
        return eng

    def load(self, eng, rows):
        if self.subset is None:
            eng.load_genotypes_host(0, T.pack_2bit(rows), self.pkg.LDP_GENO_REF)
        else:
            packed = np.ascontiguousarray(T.pack_2bit(rows).view(np.uint8).reshape(rows.shape[0], -1)[:, :(N_RAW + 3) // 4])
            eng.load_genotypes_host(0, packed, self.pkg.LDP_GENO_REF | self.pkg.LDP_GENO_MAPPED)


@pytest.mark.parametrize("case", ["codes", "planes", "sample_map"])
def test_results_through_every_release_path(gpu_pkg, case):
    subset = np.sort(np.random.default_rng(3).permutation(N_RAW)[:200]).astype(np.uint32) if case == "sample_map" else None
    life = Lifecycle(gpu_pkg, {"pair_mfma": 0} if case == "planes" else {}, subset)
    key = None if subset is None else tuple(int(s) for s in subset)
    want, want_kept = oracle_removed(key, False), oracle_removed(key, True)
    assert 0 < int(want.sum()) < M and 0 < int(want_kept.sum()) < int(KEEP.sum())
    raw = raw_codes()

    eng = life.new_engine()
    eng.set_variants(CHR_IDX, BPS)
    life.load(eng, raw)
    run1 = eng.run()
    eng.release_device()
    life.load(eng, raw)
    run2 = eng.run()
    eng.set_variants_matrix(M)          # (rows resident, no pair work queued: what restrict_variants() starts from)
    life.load(eng, raw)
    eng.restrict_variants(KEEP, CHR_IDX[KEEP], BPS[KEEP])
    run3 = eng.run()
    eng.set_variants(CHR_IDX, BPS)
    life.load(eng, raw)
    run4 = eng.run()
    eng.close()

    fresh = life.new_engine()
    fresh.set_variants(CHR_IDX[KEEP], BPS[KEEP])
    life.load(fresh, raw[KEEP])
    run3_fresh = fresh.run()
    fresh.close()

    for name, got in (("run 1", run1), ("run 2 (after release_device)", run2), ("run 4 (full table planned again)", run4)):
        assert np.array_equal(got, want), name
    assert np.array_equal(run3, run3_fresh), "run 3 (restricted) against a fresh engine"
    assert np.array_equal(run3, want_kept), "run 3 (restricted) against the oracle"


def test_decode_scratch_that_grows(gpu_pkg):
    """launches of 7 rows, then the whole file in one launch, on the same engine: the scratch of the second load is larger than the first's"""
    pkg = gpu_pkg
    f = pkg.PgenFile(os.path.join(GOLD, "varwidth_small.pgen"))
    m, n = f.variant_ct, f.sample_ct
    host = engine(pkg, n, m)
    host.load_genotypes_host(0, f.read(), pkg.LDP_GENO_REF)
    dev = engine(pkg, n, m)
    for rows_per_launch in (7, 0):
        dev.set_option("decode_rows", rows_per_launch)
        dev.load_pgen_records(0, f)
        assert_same_rows(host, dev, m)
    assert np.array_equal(host.run(), dev.run())
    host.close()
    dev.close()
    f.close()


LEAK_FOUNDERS, LEAK_VARIANTS, LEAK_WINDOW = 4096, 8192, 200
IMAGE_BYTES = LEAK_VARIANTS * LEAK_FOUNDERS // 4   # 8 MiB


def lifecycle_cycles(pkg, rows, chr_idx, cycles):
    for _ in range(cycles):
        eng = pkg.LdPruneEngine(LEAK_FOUNDERS, LEAK_WINDOW, 1, False, 0.2, order=2, device=0)
        for second in (False, True):
            eng.set_variants(chr_idx, None)
            eng.load_genotypes_host(0, rows, pkg.LDP_GENO_REF)
            eng.run()
            if not second:
                eng.release_device()
        eng.close()


def free_device_bytes():
    import torch
    torch.cuda.synchronize()
    return int(torch.cuda.mem_get_info()[0])


def test_no_device_memory_left_behind(gpu_pkg):
    """plan, load, run, release_device(), plan again, load, run, close(): after ten such cycles the device has not lost as much free memory
    as one image takes (a leak of the image or of the plan-sized arrays would show ten times over).  profiles/device_lifecycle.md has the
    drift of this reading on its own."""
    pkg = gpu_pkg
    rows = pkg.synth_genotypes_host(5, 0, LEAK_VARIANTS, LEAK_FOUNDERS, 0.01)
    chr_idx = np.zeros(LEAK_VARIANTS, dtype=np.uint32)
    lifecycle_cycles(pkg, rows, chr_idx, 1)
    before = free_device_bytes()
    lifecycle_cycles(pkg, rows, chr_idx, 10)
    after = free_device_bytes()
    print("free device memory: %d -> %d bytes (drop %d, bound %d)" % (before, after, before - after, IMAGE_BYTES))
    assert before - after < IMAGE_BYTES
