"""The reference of tests/test_count_pass_slots.py, checked without a GPU.

ldtools.cp_reference restates, with numpy on the codes of an image row, what the count pass (codes_kernel, prepare_kernel +
cp_gen_fix_kernel) stores per variant for the pair kernels' checkpoints.  Here it is compared with a loop over the samples that
shares no arithmetic with it, the checkpoint rule is compared with the cases the slot test relies on, and the integers a checkpoint
takes back out of the stored doubles (csrc/ldp_pair_device.h, "FP64 error budget": s_R by rint from a sqrt(n_R / N)) are shown to
come back exactly from the reference's doubles at every row length and for every kind of row of the slot test."""
import math

import numpy as np
import pytest

import ldtools as T

# the row lengths of tests/test_count_pass_slots.py (both kernels' lists)
LENGTHS = (1537, 2048, 2049, 16384, 16385, 32769, 49152, 49153, 57344, 57345, 65537, 131073, 262145, 524288, 524289, 1048577, 4000000, 4000001)


def brute_force(codes, n, chunks_list, r2):
    """cp_reference's numbers by one pass over the samples of every row, in Python integers and math.sqrt"""
    m = codes.shape[0]
    out = {k: np.zeros((m, 5), dtype=np.int64) for k in ("hom_r", "s_r", "calls_r", "zs_r", "zq_r")}
    for k in ("hom", "S", "calls", "zs", "zq"):
        out[k] = np.zeros(m, dtype=np.int64)
    out["a"] = np.zeros((m, 6))
    out["b"] = np.zeros((m, 6))
    scale = math.sqrt(math.sqrt(r2 * (1 + 2.0 ** -44)) * (1.0 - 1e-6))
    for v in range(m):
        row = [int(c) for c in codes[v]]
        for k in range(-1, len(chunks_list)):
            start = 0 if k < 0 else 512 * chunks_list[k]
            hom = s = calls = zs = zq = 0
            for c in row[start:]:
                if c == 3:
                    continue
                calls += 1
                z = c
                x = 1 - c
                hom += x * x
                s += x
                zs += z
                zq += z * z
            if k < 0:
                out["hom"][v], out["S"][v], out["calls"][v], out["zs"][v], out["zq"][v] = hom, s, calls, zs, zq
                out["a"][v, 5] = float(s)
                out["b"][v, 5] = math.sqrt(max(float(n) * float(hom) - float(s) * float(s), 0.0)) * scale
            else:
                out["hom_r"][v, k], out["s_r"][v, k], out["calls_r"][v, k], out["zs_r"][v, k], out["zq_r"][v, k] = hom, s, calls, zs, zq
                n_r = float(n - start)
                out["a"][v, k] = float(s) * math.sqrt(float(n) / n_r)
                out["b"][v, k] = math.sqrt(float(n) * max(float(hom) - float(s) * float(s) / n_r, 0.0))
    return out


@pytest.mark.parametrize("n,r2", [(1537, 0.5), (1537, 0.1), (2049, 0.2), (2600, 0.5), (3583, 0.05)])
def test_reference_against_a_loop_over_the_samples(n, r2):
    chunks = T.checkpoint_chunks(n, r2)
    raw = T.cp_test_rows(n, r2)
    assert raw.shape == (16, n) and len(T.CP_ROW_KINDS) == 16
    for codes in (raw, np.array([2, 1, 0, 3], dtype=np.uint8)[raw]):   # both orientations of every row
        got = T.cp_reference(codes, n, chunks, r2)
        want = brute_force(codes, n, chunks, r2)
        for k in want:
            if k in ("a", "b"):
                assert np.array_equal(T.bits_of(got[k]), T.bits_of(want[k])), k   # (numpy's and libm's sqrt are both correctly rounded)
            else:
                assert np.array_equal(got[k], want[k]), k
        # unused checkpoints: zeros
        for k in range(len(chunks), 5):
            assert not got["a"][:, k].any() and not got["b"][:, k].any() and not got["hom_r"][:, k].any() and not got["calls_r"][:, k].any()


def test_checkpoint_rule():
    """the rule of csrc/ldp_engine.cpp at the sizes the slot test names"""
    assert T.checkpoint_chunks(1536, 0.5) == []                    # three chunks: no checkpoint
    assert T.checkpoint_chunks(1537, 0.5) == [2, 3]
    assert T.checkpoint_chunks(1537, 0.1) == [3]                   # one
    assert len(T.checkpoint_chunks(2049, 0.2)) == 2                # two
    assert len(T.checkpoint_chunks(65537, 0.1)) == 4               # 0.6838 + 0.36 is beyond 0.93
    assert len(T.checkpoint_chunks(65537, 0.5)) == 5
    assert T.checkpoint_chunks(20003, 0.5) == [13, 14, 15, 19, 27]  # 40 chunks x (0.2929 + steps), rounded up
    for n in LENGTHS:
        for r2 in (0.05, 0.1, 0.2, 0.5, 0.8, 0.99):
            c = T.checkpoint_chunks(n, r2)
            assert c == sorted(set(c)) and all(0 < x < (n + 511) // 512 for x in c) and len(c) <= 5


def test_row_kinds_are_what_their_names_say():
    n, r2 = 16385, 0.5
    raw = T.cp_test_rows(n, r2)
    cps = T.checkpoint_chunks(n, r2)
    kinds = {k: raw[i] for i, k in enumerate(T.CP_ROW_KINDS)}
    _, _, altmaj = T.oracle_prepare(raw)
    assert not (kinds["random complete"] == 3).any() and (kinds["all missing"] == 3).all() and (kinds["all het"] == 1).all()
    assert (kinds["monomorphic REF"] == 0).all() and (kinds["monomorphic ALT"] == 2).all()
    assert altmaj[T.CP_ROW_KINDS.index("ALT-major with hets")] == 1 and (kinds["ALT-major with hets"] == 1).any()
    tie = kinds["exact tie"]
    assert (tie == 0).sum() == (tie == 2).sum() > 0 and altmaj[T.CP_ROW_KINDS.index("exact tie")] == 0
    assert kinds["complete but the last sample"][-1] == 3 and not (kinds["complete but the last sample"][:-1] == 3).any()
    late = kinds["missing behind the last checkpoint"]
    assert not (late[:512 * cps[-1]] == 3).any() and (late[512 * cps[-1]:] == 3).sum() > 1
    early = kinds["missing before the first checkpoint"]
    assert not (early[512 * cps[0]:] == 3).any() and (early[:512 * cps[0]] == 3).sum() > 1
    one = np.flatnonzero(kinds["hom calls in one chunk before the first checkpoint"] != 1)
    assert len(one) == 512 and one[0] // 512 == one[-1] // 512 == cps[0] - 1
    last = np.flatnonzero(kinds["hom calls in the last chunk"] != 1)
    assert len(last) == n - 512 * ((n - 1) // 512) and last[0] // 512 == (n - 1) // 512
    assert 0.55 < (kinds["60% missing"] == 3).mean() < 0.65
    assert 0 < int(altmaj.sum()) < len(altmaj)


@pytest.mark.parametrize("n", LENGTHS)
def test_integers_come_back_from_the_doubles(n):
    """s_r = rint(a sqrt(n_R / N)) and hom_r = rint(b^2 / N + s_r^2 / n_R) are exact for every kind of row, in both orientations, at every
    row length of the slot test (worst distance from an integer met over all of them: 4.7e-10, at N = 4,000,000 and 4,000,001,
    doubling with N from 2.8e-14 at 1,537; 0.5 would be needed to lose one)."""
    r2 = 0.5
    chunks = T.checkpoint_chunks(n, r2)
    raw = T.cp_test_rows(n, r2, count=16 if n < 1000000 else 14)
    worst = 0.0
    for codes in (raw, np.array([2, 1, 0, 3], dtype=np.uint8)[raw]):
        ref = T.cp_reference(codes, n, chunks, r2)
        s_r, hom_r, w = T.cp_recover(ref["a"], ref["b"], n, chunks)
        assert np.array_equal(s_r, ref["s_r"]) and np.array_equal(hom_r, ref["hom_r"])
        worst = max(worst, w)
    print("N = %d: %d checkpoints, worst distance from an integer %.3g" % (n, len(chunks), worst))
    # the budget of csrc/ldp_pair_device.h: s_r is off by <= 4e6 x 5e-16 = 2e-9; hom_r's two terms carry three roundings each at a
    # magnitude <= N: 6 x 2^-53 x 4e6 = 2.7e-9
    assert worst < 1e-8
