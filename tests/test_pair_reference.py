"""CPU tests of the per-pair reference the GPU tests compare the production kernels' decisions with (ldtools.band_pair_stats,
band_decisions, compare_decisions): plain float64 matrix products and three float64 multiplications, checked here against
the oracle's word-by-word popcount arithmetic (oracle/ldoracle.c) for EVERY candidate pair of small bands that hold the rows
kernels go wrong on, and for every pair of the rows with missing calls that tests/test_r2_missing.py runs the r^2 kernels on
(r2_tools.missing_rows, whose input conditions are checked here too).  Also the measurement of how much of a single wrong decision the prune set shows."""
import ctypes

import numpy as np
import pytest

import ldtools as T
import r2_tools as R
from test_host_logic import make_positions, recs_from_vaggs


def edge_rows(m, n, seed):
    """complete rows, rows at 0.1 % / 5 % / 70 % missing, the four monomorphic kinds, an exact REF = ALT tie, ALT-major rows"""
    rng = np.random.default_rng(seed)
    raw = T.synth_raw_codes(m, n, seed, missing_rate=0.0, ld_copy_prob=0.6, redraw=0.1)
    for v in range(m):
        rate = (0.0, 0.001, 0.05, 0.7)[v % 4]
        if rate:
            raw[v, rng.random(n) < rate] = 3
    raw[3] = 0                      # monomorphic hom-REF
    raw[9] = 2                      # monomorphic hom-ALT
    raw[14] = 1                     # all het
    raw[20] = 3                     # all missing
    raw[26] = 0
    raw[26, : n // 2] = 2           # ref_ct == alt_ct when n is even: the tie goes to REF
    for v in (5, 11, 12, 30):       # ALT is the major allele
        raw[v] = np.where(rng.random(n) < 0.8, 2, rng.integers(0, 2, size=n))
        raw[v, rng.random(n) < 0.02] = 3
    return raw


def oracle_all_pairs(raw, lo, r2):
    m, n = raw.shape
    inv, mf, altmaj = T.oracle_prepare(raw)
    hom, r2h, vaggs = T.oracle_split(inv, n)
    lib = T.oracle()
    thr = lib.ldo_prune_thresh(r2)
    stats, dec = [], []
    for j in range(m):
        for i in range(int(lo[j]), j):
            st = T.oracle_pair_stats(hom, r2h, vaggs, n, i, j)
            stats.append(st.astuple())
            dec.append(bool(lib.ldo_exceeds(ctypes.byref(st), thr)))
    return np.array(stats, dtype=np.int64).reshape(-1, 6), np.array(dec, dtype=bool), altmaj


@pytest.mark.parametrize("n", [2, 63, 64, 65, 1025])
@pytest.mark.parametrize("is_bp,window", [(False, 25), (True, 6000)])
def test_every_pair_of_a_band_equals_the_oracle(pkg, n, is_bp, window):
    m = 64
    raw = edge_rows(m, n, seed=100 + n)
    chr_idx, bps = make_positions(m, 2, n + 3)
    eng = pkg.LdPruneEngine(n, window, 1, is_bp, 0.2)
    eng.set_variants(chr_idx, bps)
    lo, cand = eng.band()
    eng.close()
    first, second = T.band_pairs(lo)
    assert len(first) == cand > 300
    k = 0
    for j in range(m):                               # band_pairs is the order of ldp_run_with_stats()
        for i in range(int(lo[j]), j):
            assert (first[k], second[k]) == (i, j)
            k += 1
    stats = T.band_pair_stats(raw, lo, block=7)      # (a block size that cuts the band everywhere)
    assert np.array_equal(stats, T.band_pair_stats(raw, lo))
    for r2 in (0.02, 0.2, 0.5, 0.95):
        want_stats, want_dec, altmaj = oracle_all_pairs(raw, lo, r2)
        assert np.array_equal(stats, want_stats), np.flatnonzero((stats != want_stats).any(1))[:5]
        got = T.band_decisions(stats, r2)
        nd, msg = T.compare_decisions(got, want_dec, lo, stats, r2)
        assert nd == 0, msg
    assert altmaj[[5, 11, 12, 30]].all() or n == 2
    assert not altmaj[26]
    print("pairs compared: %d x 4 thresholds" % cand)


@pytest.mark.parametrize("n", [2, 63, 64, 65, 1025])
def test_every_r2_of_all_pairs_equals_the_oracle(n):
    """ldtools.band_r2 / r2_to_float32 / the REF-oriented r (what tests/test_r2_complete.py compares the r^2 outputs with), all pairs of
    the edge rows: bit for bit the oracle's integers through ComputeR2's operations, the IEEE float32 cast, and the REF orientation --
    obtained from REF-oriented products -- against sign(cov) x (one of the two variants is ALT-major) from the oracle's major alleles."""
    m = 64
    raw = edge_rows(m, n, seed=100 + n)
    lo = np.zeros(m, dtype=np.int64)
    first, second = T.band_pairs(lo)
    assert len(first) == m * (m - 1) // 2
    stats = T.band_pair_stats(raw, lo)
    r2 = T.band_r2(stats)
    r_major = T.band_r2(stats, signed=1)
    r_ref = T.band_r2(T.band_pair_stats(raw, lo, orient=False), signed=1)
    inv, mf, altmaj = T.oracle_prepare(raw)
    hom, r2h, vaggs = T.oracle_split(inv, n)
    want = np.zeros(len(first), dtype=np.float64)
    want_major = np.zeros(len(first), dtype=np.float64)
    want_ref = np.zeros(len(first), dtype=np.float64)
    nan = np.array([T.R2_NAN64], dtype=np.uint64).view(np.float64)[0]
    for k in range(len(first)):
        i, j = int(first[k]), int(second[k])
        st = T.oracle_pair_stats(hom, r2h, vaggs, n, i, j)
        cov, v1, v2 = T.oracle_r2(st)
        prod = v1 * v2
        if st.nm == 0 or prod == 0.0:
            want[k] = want_major[k] = want_ref[k] = nan
            continue
        want[k] = cov * cov / prod
        r = float(np.sqrt(np.float64(want[k])))
        sign = (cov > 0) - (cov < 0)
        want_major[k] = -r if sign < 0 else r
        sign_ref = sign * (-1 if (altmaj[i] ^ altmaj[j]) else 1)
        want_ref[k] = -r if sign_ref < 0 else r
    assert np.array_equal(T.bits_of(r2), T.bits_of(want)), np.flatnonzero(T.bits_of(r2) != T.bits_of(want))[:5]
    assert np.array_equal(T.bits_of(r_major), T.bits_of(want_major))
    assert np.array_equal(T.bits_of(r_ref), T.bits_of(want_ref)), np.flatnonzero(T.bits_of(r_ref) != T.bits_of(want_ref))[:5]
    isn = np.isnan(want)
    assert isn.sum() >= 4 * (m - 1) - 6 and (T.bits_of(r2)[isn] == T.R2_NAN64).all()     # the four monomorphic rows against everything
    for vals in (r2, r_major, r_ref):
        f32 = T.r2_to_float32(vals)
        assert f32.dtype == np.float32
        assert (T.bits_of(f32)[isn] == T.R2_NAN32).all()
        assert np.array_equal(T.bits_of(f32)[~isn], T.bits_of(np.float32(vals[~isn])))
    # +0.0 at a zero covariance in either orientation; both signs and both orientations occur
    zero = ~isn & (want == 0.0)
    assert not T.bits_of(r_major)[zero].any() and not T.bits_of(r_ref)[zero].any()
    if n > 2:
        assert (want_major[~isn] < 0).any() and (want_major[~isn] > 0).any() and (np.signbit(r_ref) != np.signbit(r_major)).any()
    # the diagonal and the dense layout
    d = T.self_r2(raw)
    for v in range(m):
        st = T.oracle_pair_stats(hom, r2h, vaggs, n, v, v)
        cov, v1, v2 = T.oracle_r2(st)
        w = nan if (st.nm == 0 or v1 * v2 == 0.0) else cov * cov / (v1 * v2)
        assert T.bits_of(np.float64(d[v]))[()] == T.bits_of(np.float64(w))[()], v
    dense = T.band_to_dense(r2, lo, 10, 30, 5, 20, diag=d)
    for j in range(10, 40):
        for i in range(5, 25):
            k = j * (j - 1) // 2 + i
            w = r2[k] if i < j else (d[j] if i == j else 0.0)
            assert T.bits_of(np.float64(dense[j - 10, i - 5]))[()] == T.bits_of(np.float64(w))[()], (i, j)
    print("pairs compared: %d (r^2, r major-oriented, r REF-oriented, float32 casts)" % len(first))


@pytest.mark.parametrize("n", [3, 90, 512, 513, 1100])
def test_rows_with_missing_calls_meet_their_input_conditions(n):
    """r2_tools.missing_rows (the fixture of tests/test_r2_missing.py): the placed rows at every n, the counts and shares from n = 90 on --
    MissingReference.input_conditions, from the reference alone; the smaller matrices of the planner test as well"""
    ref = R.reference_missing(600, n)
    ref.input_conditions()
    places = R.missing_places(600)
    assert places == {"all_missing": [17, 300, 597], "complementary": [(50, 290), (258, 259), (31, 32)], "shared_variance": [(70, 330), (513, 515)],
                      "edges": [100, 257, 599], "singletons": [110, 521]}
    assert R.missing_places(200) == {"all_missing": [17, 197], "complementary": [(31, 32)], "shared_variance": [], "edges": [100, 199], "singletons": [110]}
    assert np.array_equal(ref.raw, R.missing_rows(600, n)) and not ref.raw.flags.writeable      # one seeded generator: the same rows every time
    kept = ref.raw != 3
    unplaced = np.ones(600, dtype=bool)
    unplaced[[26, 70, 513, 110, 521]] = False                                                             # (rows rewritten as a whole)
    assert np.array_equal(ref.raw[unplaced][kept[unplaced]], R.complete_rows(600, n)[unplaced][kept[unplaced]])   # every call left is complete_rows' call
    if n >= 90:
        c = ref.counts
        assert c["nm0"] >= 1500 and c["nan_own_variance"] >= 20 and c["strong"] >= 500 and 0.25 <= c["negative"] <= 0.75
        assert c["complete_rows"] >= 150 and 2 * c["partial"] >= 179700
    if n == 90:
        for m in (384, 385, 200):
            R.reference_missing(m, n).input_conditions()


@pytest.mark.parametrize("n", [90, 513])
def test_reference_of_the_rows_with_missing_calls_equals_the_oracle(n):
    """band_pair_stats / band_r2 (r^2, r in both orientations) on missing_rows(600, n): EVERY pair's six integers equal the oracle's word-by-word
    popcounts, every value its cov, var1, var2 through ComputeR2's operations bit for bit -- all-missing rows, pairs without a shared sample,
    variance that vanishes on the shared samples, major alleles decided by the calls a row has"""
    m = 600
    ref = R.reference_missing(m, n)
    inv, mf, altmaj = T.oracle_prepare(ref.raw)
    assert np.array_equal(altmaj.astype(bool), R.alt_major(ref.raw))
    hom, r2h, vaggs = T.oracle_split(inv, n)
    pairs = len(ref.first)
    assert pairs == m * (m - 1) // 2
    want_stats = np.zeros((pairs, 6), dtype=np.int64)
    cvv = np.zeros((pairs, 3), dtype=np.float64)
    for k in range(pairs):
        st = T.oracle_pair_stats(hom, r2h, vaggs, n, int(ref.first[k]), int(ref.second[k]))
        want_stats[k] = st.astuple()
        cvv[k] = T.oracle_r2(st)
    bad = np.flatnonzero((ref.stats != want_stats).any(1))
    assert not len(bad), [(int(ref.first[k]), int(ref.second[k]), ref.stats[k].tolist(), want_stats[k].tolist()) for k in bad[:5]]
    cov, prod = cvv[:, 0], cvv[:, 1] * cvv[:, 2]
    undefined = (want_stats[:, 0] == 0) | (prod == 0.0)
    want = (cov * cov) / np.where(undefined, 1.0, prod)
    want_major = np.sqrt(want)
    want_major[cov < 0] = -want_major[cov < 0]
    flip = (altmaj[ref.first] ^ altmaj[ref.second]).astype(bool)
    want_ref = np.where(flip & (want_major != 0.0), -want_major, want_major)
    for w in (want, want_major, want_ref):
        T.bits_of(w)[undefined] = T.R2_NAN64
    for mode, w in ((0, want), (1, want_major), (2, want_ref)):
        bad = np.flatnonzero(T.bits_of(ref.band[mode]) != T.bits_of(w))
        assert not len(bad), (mode, [(int(ref.first[k]), int(ref.second[k]), ref.band[mode][k], w[k], want_stats[k].tolist()) for k in bad[:5]])
    d = ref.diag
    for v in range(m):
        st = T.oracle_pair_stats(hom, r2h, vaggs, n, v, v)
        c, v1, v2 = T.oracle_r2(st)
        w = np.float64(c * c / (v1 * v2)) if (st.nm and v1 * v2 != 0.0) else np.array([T.R2_NAN64], dtype=np.uint64).view(np.float64)[0]
        assert T.bits_of(np.float64(d[v]))[()] == T.bits_of(np.float64(w))[()], v
    assert undefined.sum() >= 1500 and (want_stats[:, 0] == 0).sum() >= 1500 and (undefined & (want_stats[:, 0] > 0)).sum() >= 20
    print("pairs compared: %d (six integers, r^2, r major-oriented, r REF-oriented), %d undefined" % (pairs, int(undefined.sum())))


def test_decisions_from_a_structured_stats_array(pkg):
    """band_decisions takes the device's own tuples (ldp_pair_stats_t) as well"""
    raw = edge_rows(40, 130, seed=5)
    lo = np.maximum(np.arange(40) - 12, 0)
    stats = T.band_pair_stats(raw, lo)
    rec = np.zeros(len(stats), dtype=pkg.PAIR_STATS_DTYPE)
    for f, name in enumerate(T.PAIR_FIELDS):
        rec[name] = stats[:, f]
    assert np.array_equal(T.band_decisions(rec, 0.3), T.band_decisions(stats, 0.3))
    assert 0 < T.band_decisions(stats, 0.3).sum() < len(stats)


def test_a_planted_one_bit_difference_is_named():
    m, n = 50, 200
    raw = T.synth_raw_codes(m, n, 9, missing_rate=0.02, ld_copy_prob=0.7, redraw=0.1)
    lo = np.maximum(np.arange(m) - 9, 0)
    stats = T.band_pair_stats(raw, lo)
    want = T.band_decisions(stats, 0.2)
    assert T.compare_decisions(want, want, lo, stats, 0.2)[0] == 0
    first, second = T.band_pairs(lo)
    k = int(np.flatnonzero((first == 30) & (second == 37))[0])
    got = want.copy()
    got[k] = not got[k]
    nd, msg = T.compare_decisions(got, want, lo, stats, 0.2, counters={"pred_true": 7, "route_sparse_launches": 1})
    assert nd == 1
    assert "pair (i=30, j=37)" in msg and "got %d want %d" % (int(got[k]), int(want[k])) in msg
    assert str(tuple(int(x) for x in stats[k])) in msg and "route_sparse_launches=1" in msg
    # a second one: both are listed, in band order
    got[0] = not got[0]
    nd, msg = T.compare_decisions(got, want, lo, stats, 0.2)
    assert nd == 2 and msg.index("pair (i=0, j=1)") < msg.index("pair (i=30, j=37)")
    assert T.compare_decisions(got[:-1], want, lo, stats, 0.2)[0] > 0


SENSITIVITY_SHAPES = [
    # m, n, window (variants), r2, missing
    (1500, 3000, 600, 0.2, 0.001),
    (700, 2000, 150, 0.5, 0.05),
]


@pytest.mark.parametrize("shape", SENSITIVITY_SHAPES)
def test_how_much_of_one_wrong_decision_the_prune_set_shows(pkg, shape):
    """A measurement kept reproducible, not a bound: the reference's decisions of every candidate pair go through the greedy scan
    (ldp_debug_replay_pairs) with ONE decision changed at a time, 400 times a true one dropped and 400 times a false one set, and
    the number of trials in which the prune set changes is printed (DESIGN 5a has the table).  The scan ignores a pair as soon as
    one of its variants is gone, so most single errors leave the set as it was: that is why the GPU tests compare the
    predicate rows themselves (tests/test_pair_decisions.py)."""
    m, n, window, r2, miss = shape
    trials = 400
    raw = T.synth_raw_codes(m, n, seed=m + n, missing_rate=miss, ld_copy_prob=0.5, redraw=0.05)
    chr_idx = np.zeros(m, dtype=np.uint32)
    inv, mf, _ = T.oracle_prepare(raw)
    _, _, vaggs = T.oracle_split(inv, n)
    eng = pkg.LdPruneEngine(n, window, 1, False, r2)
    eng.set_variants(chr_idx, None)
    lo, cand = eng.band()
    eng.debug_set_variant_recs(recs_from_vaggs(pkg, vaggs, n, m))
    eng.set_maj_freqs(0, mf)
    dec = T.band_decisions(T.band_pair_stats(raw, lo), r2)
    first, second = T.band_pairs(lo)
    first, second = first.astype(np.uint32), second.astype(np.uint32)
    base = eng.debug_replay_pairs(first[dec], second[dec])
    want, _ = T.oracle_indep_pairwise(inv, n, chr_idx, np.arange(m, dtype=np.uint32), mf, window, 1, False, r2, 2)
    assert np.array_equal(base, want)
    rng = np.random.default_rng(7)
    true_idx, false_idx = np.flatnonzero(dec), np.flatnonzero(~dec)
    changed = {}
    for name, pool in (("one TRUE decision dropped", true_idx), ("one FALSE decision set", false_idx)):
        changed[name] = 0
        for k in rng.choice(pool, size=trials, replace=False):
            d = dec.copy()
            d[k] = not d[k]
            changed[name] += int(not np.array_equal(eng.debug_replay_pairs(first[d], second[d]), base))
    eng.close()
    print("sensitivity m=%d n=%d window=%d r2=%g missing=%g: %d true of %d candidates; %s"
          % (m, n, window, r2, miss, len(true_idx), cand, "; ".join("%s: set changed in %d of %d" % (k, v, trials) for k, v in changed.items())))
    for v in changed.values():
        assert v < trials
