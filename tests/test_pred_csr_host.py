"""The host replay over the COMPACTED predicate rows, without a GPU.

A production run never copies its dense predicate rows back: pred_compact_kernel (csrc/ldp_pred_csr.hip) returns every row as its non-zero
words -- meta[j] = (first entry, entries), an entry = (word index inside the row, bits), ascending -- and replay_subcontig / pred_word
(csrc/ldp_engine_run.cpp) walk those entries through PredView's CSR branch.  The debug option "replay_csr" makes ldp_debug_replay_pairs()
build that form from its dense rows with a plain host loop (1: the 64-row blocks' runs ascend, 2: they descend -- the kernel's blocks land in
the order of their atomic adds) and replay through the same branch.  Compared here, as equalities of sets and integers:
  the removed set, and counters()["replay_pairs"] -- the pairs the scan visited, which sees a walk over other pairs even where the set
  comes out equal --, for dense / CSR ascending / CSR descending x replay_steps 0, 2, 7, 1000.
Tier 1, realisable decisions (band_decisions of synthetic rows): all three views and ldtools.oracle_indep_pairwise agree.  Tier 2, arbitrary
decision sets (none, every candidate pair, random bits at 0.1 % and 30 %, 200 single flips of the tier-1 set): both CSR views equal the
dense view, which tier 1 pins to the oracle on the same shapes (and tests/test_host_logic.py on its own)."""
import numpy as np
import pytest

import ldtools as T
from test_host_logic import make_positions, recs_from_vaggs

VIEWS = (0, 1, 2)            # option "replay_csr": dense, CSR with ascending block runs, CSR with descending block runs
STEPS = (0, 2, 7, 1000)      # option "replay_steps"
N_FLIPS = 100                # single flips per direction (true dropped / false set)


class Plan:
    """rows, positions, the band, the realisable decisions and the oracle's prune set of one case (computed once per case)"""

    def __init__(self, pkg, m, n, seed, window, step, is_bp, r2, order, nchr=3, big_gap_prob=0.01, ld_copy_prob=0.5):
        self.m, self.n, self.window, self.step, self.is_bp, self.r2, self.order = m, n, window, step, is_bp, r2, order
        self.raw = T.synth_raw_codes(m, n, seed, missing_rate=0.02, ld_copy_prob=ld_copy_prob)
        if is_bp:
            self.chr_idx, self.bps = make_positions(m, nchr, seed + 100, big_gap_prob=big_gap_prob)
        else:
            per = (m + nchr - 1) // nchr
            self.chr_idx, self.bps = (np.arange(m) // per).astype(np.uint32), np.arange(m, dtype=np.uint32)
        inv, self.mf, _ = T.oracle_prepare(self.raw)
        self.want, _ = T.oracle_indep_pairwise(inv, n, self.chr_idx, self.bps, self.mf, window, step, is_bp, r2, order)
        _, _, vaggs = T.oracle_split(inv, n)
        self.recs = recs_from_vaggs(pkg, vaggs, n, m)
        eng = self.engine(pkg)
        self.lo, self.cand = eng.band()
        self.subs = eng.subcontigs()
        eng.close()
        self.lo = self.lo.astype(np.int64)
        # band_decisions(band_pair_stats(raw, lo), r2), slab by slab of second variants (a slab's statistics are a few MB at any band width)
        dec = []
        for j0 in range(0, m, 512):
            part = np.arange(m, dtype=np.int64)
            part[j0:j0 + 512] = self.lo[j0:j0 + 512]
            dec.append(T.band_decisions(T.band_pair_stats(self.raw, part), r2))
        self.dec = np.concatenate(dec) if dec else np.zeros(0, dtype=bool)
        assert len(self.dec) == self.cand
        self.first, self.second = (a.astype(np.uint32) for a in T.band_pairs(self.lo))

    def engine(self, pkg, shard=None):
        eng = pkg.LdPruneEngine(self.n, self.window, self.step, self.is_bp, self.r2, order=self.order, device=-1)
        eng.set_variants(self.chr_idx, self.bps if self.is_bp else None)
        if shard is not None:
            eng.set_shard(*shard)
        eng.debug_set_variant_recs(self.recs)
        eng.set_maj_freqs(0, self.mf)
        return eng

    def pairs(self, dec):
        return self.first[dec], self.second[dec]


def replay_all_views(eng, first, second, what):
    """every view x every instalment count: the CSR views give the dense view's removed set and visit the dense view's pairs; the dense
    view's removed set does not depend on the instalments.  Returns the removed set."""
    base = None
    for steps in STEPS:
        eng.set_option("replay_steps", steps)
        dense = None
        for view in VIEWS:
            eng.set_option("replay_csr", view)
            got = eng.debug_replay_pairs(first, second)
            visited = eng.counters()["replay_pairs"]
            if view == 0:
                dense = (got, visited)
            else:
                assert np.array_equal(got, dense[0]), (what, "replay_csr", view, "replay_steps", steps, int(got.sum()), int(dense[0].sum()))
                assert visited == dense[1], (what, "replay_csr", view, "replay_steps", steps, "replay_pairs", visited, dense[1])
        if base is None:
            base = dense
        else:
            assert np.array_equal(dense[0], base[0]) and dense[1] == base[1], (what, "replay_steps", steps)
    eng.set_option("replay_steps", 0)
    eng.set_option("replay_csr", 0)
    return base[0]


def decision_sets(plan, seed, flips=N_FLIPS):
    """tier 2: (label, decisions) -- none, every candidate pair, independent random bits, single flips of the realisable set"""
    rng = np.random.default_rng(seed)
    cand = plan.cand
    yield "none", np.zeros(cand, dtype=bool)
    yield "every pair", np.ones(cand, dtype=bool)
    yield "random 0.1 %", rng.random(cand) < 0.001
    yield "random 30 %", rng.random(cand) < 0.3
    true, false = np.flatnonzero(plan.dec), np.flatnonzero(~plan.dec)
    for k in rng.choice(true, size=min(flips, len(true)), replace=False):
        dec = plan.dec.copy()
        dec[k] = False
        yield "true pair %d dropped" % k, dec
    for k in rng.choice(false, size=min(flips, len(false)), replace=False):
        dec = plan.dec.copy()
        dec[k] = True
        yield "false pair %d set" % k, dec


def check_plan(pkg, plan, seed, flips=N_FLIPS):
    eng = plan.engine(pkg)
    try:
        got = replay_all_views(eng, *plan.pairs(plan.dec), "tier 1")
        assert np.array_equal(got, plan.want), ("tier 1 against the oracle", int(got.sum()), int(plan.want.sum()))
        for label, dec in decision_sets(plan, seed, flips):
            replay_all_views(eng, *plan.pairs(dec), label)
    finally:
        eng.close()


# m, n, seed, window, step, is_bp, r2
COUNT_CASES = [
    (400, 65, 1, 50, 1, False, 0.2),
    (400, 65, 2, 50, 5, False, 0.2),
    (400, 33, 3, 40, 40, False, 0.1),
]


@pytest.mark.parametrize("order", [2, 1])
@pytest.mark.parametrize("case", COUNT_CASES)
def test_count_windows(pkg, case, order):
    """count windows with step 1, 5 and step = window; 400 rows are seven 64-row blocks with a ragged last one"""
    plan = Plan(pkg, *case, order)
    assert 50 < plan.dec.sum() < plan.cand // 2
    check_plan(pkg, plan, case[2])


@pytest.mark.parametrize("order", [2, 1])
def test_kb_windows_over_three_chromosomes_with_gaps(pkg, order):
    """kb windows; gaps far wider than the window cut the chromosomes into subcontigs of every length, 2 among them, and leave variants alone
    in their stretch (a subcontig of length 1 holds no pair: the plan lists none, the variant is in no subcontig)"""
    plan = Plan(pkg, 600, 65, 11, 15000, 1, True, 0.2, order, big_gap_prob=0.08)
    lens = [ln for ln, _ in plan.subs]
    covered = np.zeros(plan.m, dtype=bool)
    for ln, f0 in plan.subs:
        covered[f0:f0 + ln] = True
    assert 2 in lens and (1 in lens or not covered.all()) and max(lens) > 32, sorted(set(lens))
    assert plan.dec.sum() > 50
    check_plan(pkg, plan, 11)


@pytest.mark.parametrize("order", [2, 1])
def test_rows_of_132_words(pkg, order):
    """a count window of 4,200 variants over 6,000: rows reach 132 words (133 where the 4,199 firsts straddle one more), and at 33 samples and r^2 > 0.1 chance alone sets bits in all of
    them -- entries lie past index 64, rows hold more than 128 entries.  (Fewer flips: a replay here reads 790,000 words.)"""
    plan = Plan(pkg, 6000, 33, 21, 4200, 1, False, 0.1, order, nchr=1)
    nw = (np.arange(plan.m) - 1) // 32 - plan.lo // 32 + 1
    assert nw.max() in (132, 133)
    word = plan.first[plan.dec].astype(np.int64) // 32 - plan.lo[plan.second[plan.dec]] // 32
    per_row = np.bincount(plan.second[plan.dec], minlength=plan.m)
    assert word.max() >= 131 and (word > 64).sum() > 1000 and per_row.max() > 128
    check_plan(pkg, plan, 21, flips=5)


@pytest.mark.parametrize("order", [2, 1])
@pytest.mark.parametrize("m", [1, 2, 33, 64, 65])
def test_small_plans(pkg, m, order):
    """no pair, one pair, fewer rows than a block, exactly one block, one block and a remainder"""
    plan = Plan(pkg, m, 33, 30 + m, 50, 5, False, 0.1, order, nchr=1)
    assert plan.cand == (m * (m - 1) // 2 if m <= 50 else plan.cand)
    check_plan(pkg, plan, m)


@pytest.mark.parametrize("order", [2, 1])
def test_every_rank_of_three(pkg, order):
    """ldp_set_shard(rank, 3): a rank's rows are its own subcontigs' (shard-local indices, its own 64-row blocks); every rank's CSR views
    equal its dense view, and the union of the ranks' sets is the unsharded set = the oracle's"""
    plan = Plan(pkg, 600, 65, 13, 15000, 1, True, 0.2, order, big_gap_prob=0.03)
    assert len(plan.subs) >= 6
    union = np.zeros(plan.m, dtype=bool)
    for rank in range(3):
        eng = plan.engine(pkg, shard=(rank, 3))
        try:
            assert eng.counters()["owned_subcontig_ct"] > 0
            got = replay_all_views(eng, *plan.pairs(plan.dec), "rank %d, tier 1" % rank)
            assert not (got & union).any()
            union |= got
            for label, dec in decision_sets(plan, 13 + rank, flips=10):
                replay_all_views(eng, *plan.pairs(dec), "rank %d, %s" % (rank, label))
        finally:
            eng.close()
    assert np.array_equal(union, plan.want)


def test_the_option_takes_0_1_2_only(pkg):
    eng = pkg.LdPruneEngine(33, 50, 5, False, 0.2, device=-1)
    for value in (3, -1, 0.5):
        with pytest.raises(pkg.LdpError) as ei:
            eng.set_option("replay_csr", value)
        assert ei.value.code == pkg.LDP_ERR_INVALID
    for value in (1, 2, 0):
        eng.set_option("replay_csr", value)
    eng.close()
