"""CPU tests of the choice of thresholds by pseudo-expected accuracy: the restatement of
tests/auto_ref.py on random matrices and on hand-made cases whose choice is written out, and the library's new symbols.
No device: these pin the contract the GPU tests compare the library with."""
import ctypes as C
import os

import numpy as np
import pytest

import auto_ref as ref
import levels_ref as lref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, FREE = ref.NONE, ref.FREE


def _random_matrix(rs, L, quarters):
    p = np.triu(rs.rand(L, L).astype(np.float32), 1) if L else np.zeros((0, 0), np.float32)
    p[rs.rand(L, L) < 0.55] = 0
    if quarters:
        p = (np.round(p * 4) / 4).astype(np.float32)
    return p


@pytest.fixture(scope="module")
def random_cases(oracle):
    """(p, candidates, K, restatement) for L = 0 .. 33, a third of them rounded to quarters so that T ties occur; built once"""
    rs = np.random.RandomState(27)
    lists = (ref.GAMMAS, (1, 3), (2,), tuple(range(1, 17)))
    cases = []
    for L in range(34):
        p = _random_matrix(rs, L, quarters=(L % 3 == 1))
        cand = ref.candidates(lists[L % 4])
        K = 1 + (L // 2) % 4
        cases.append((p, cand, K, ref.decode(oracle, p, cand, K)))
    return cases


def test_q_is_an_exact_integer():
    p = np.array([0.0, 1.0, 0.5, 0.9, 2.0, -1.0, 2.0 ** -31, 1 - 2.0 ** -24], np.float32)
    assert ref.q(p).tolist() == [0, 2 ** 30, 2 ** 29, int(np.float32(0.9) * np.float32(2 ** 30)), 2 ** 30, 0, 0, 2 ** 30 - 64]
    assert float(np.float32(0.9) * np.float32(2 ** 30)) == float(np.float32(0.9)) * 2 ** 30  # the product is exact: a power of two


def test_the_choice_is_the_list_order_argmax(random_cases):
    """by brute force over all C: nothing beats the chosen one, and nothing before it equals it"""
    ties = kept = 0
    for p, cand, K, r in random_cases:
        base = (0, 0)
        for k in range(r.launched):
            vals = [(base[0] + t, base[1] + n) for t, n in zip(r.cand_tp[k], r.cand_pairs[k])]
            if r.chosen[k] == NONE:
                assert not any(ref.beats(v, base, r.sum_p) for v in vals)
                continue
            b = r.chosen[k]
            assert not any(ref.beats(v, vals[b], r.sum_p) for v in vals)
            assert all(ref.beats(vals[b], v, r.sum_p) for v in vals[:b])  # an earlier one that equalled it would have won
            ties += sum(1 for v in vals[b + 1:] if not ref.beats(vals[b], v, r.sum_p))
            assert ref.beats(vals[b], base, r.sum_p)  # a kept level strictly raises F
            assert ref.f_of(*vals[b], r.sum_p) > ref.f_of(*base, r.sum_p) or base == (0, 0)
            assert (r.tp[k], r.npairs[k]) == (r.cand_tp[k][b], r.cand_pairs[k][b]) == ref.value(p, r.per_level[k])
            base = vals[b]
            kept += 1
    assert ties > 10 and kept > 30


def test_levels_above_an_empty_level_are_empty(random_cases):
    seen = 0
    for p, cand, K, r in random_cases:
        first_empty = r.chosen.index(NONE) if NONE in r.chosen else K
        assert all(c == NONE for c in r.chosen[first_empty:]) and r.launched == min(K, first_empty + 1) * (p.shape[0] > 0)
        for k in range(first_empty, K):
            assert r.scores[k] == 0 and r.tp[k] == 0 and r.npairs[k] == 0 and not np.any(r.level == k)
        for k in range(r.launched, K):
            assert not any(r.cand_tp[k]) and not any(r.cand_pairs[k])
        seen += first_empty < K
    assert seen > 5


def test_the_result_is_the_fixed_decode_at_the_chosen_thresholds(random_cases, oracle):
    knots = 0
    for p, cand, K, r in random_cases:
        m = len(r.kept)
        if not m:
            assert np.all(r.ss == NONE) and np.all(r.level == FREE) and np.all(r.scores == 0)
            continue
        scores, merged, level, per_level = lref.decode(oracle, p, [cand[c] for c in r.kept])
        assert merged.tobytes() == r.ss.tobytes() and level.tobytes() == r.level.tobytes()
        assert scores.tobytes() == r.scores[:m].tobytes() and np.all(r.scores[m:] == 0)
        knots += m > 1
        if K == 1:
            s, ss = oracle.nussinov(p, None, float(cand[r.kept[0]]))
            assert ss.tobytes() == r.ss.tobytes() and np.float32(s).tobytes() == r.scores[0].tobytes()
    assert knots > 5


def test_sum_p_counts_the_upper_triangle_once(random_cases):
    for p, cand, K, r in random_cases:
        L = p.shape[0]
        assert r.sum_p == sum(int(ref.q(p[i, j])) for i in range(L) for j in range(i + 1, L))


@pytest.mark.parametrize("case", ref.hand_cases(), ids=lambda c: c.name)
def test_hand_made_cases(case, oracle):
    r = ref.decode(oracle, case.p, case.cand, case.nlevels)
    assert r.chosen == case.chosen
    assert lref.brackets(r.ss, r.level) == case.text


def test_what_the_hand_made_cases_are_for(oracle):
    by_name = {c.name: c for c in ref.hand_cases()}
    c = by_name["helix-and-scatter"]
    r = ref.decode(oracle, c.p, c.cand, 1)
    assert r.cand_pairs[0] == [5, 5, 5, 9, 9, 9] and r.chosen[0] != len(c.cand) - 1  # not the lowest threshold
    assert r.cand_tp[0][3] > r.cand_tp[0][0] and not ref.beats((r.cand_tp[0][3], 9), (r.cand_tp[0][0], 5), r.sum_p)
    c = by_name["nothing"]
    r = ref.decode(oracle, c.p, c.cand, 2)
    assert r.launched == 1 and not any(r.cand_pairs[0]) and r.sum_p > 0 and r.f == 0.0
    c = by_name["equal-values"]
    r = ref.decode(oracle, c.p, c.cand, 1)
    assert r.cand_tp[0][0] == r.cand_tp[0][1] > 0 and r.cand_pairs[0] == [1, 1] and r.chosen == [0]
    c = by_name["h-type-12"]
    r = ref.decode(oracle, c.p, c.cand, 2)
    assert r.npairs == [2, 2] and sorted(set(r.level.tolist())) == [0, 1, FREE]
    c = by_name["crosses-nothing"]
    r = ref.decode(oracle, c.p, c.cand, 2)
    assert r.launched == 2 and max(r.cand_pairs[1]) == 1 and r.chosen[1] == NONE and r.ss[3] == NONE  # (3, 10) was decoded, and not kept
    assert ref.decode(oracle, np.zeros((0, 0), np.float32), c.cand, 2).launched == 0


def test_auto_thresholds_object():
    from dafs_amd import capi  # host code only
    a = capi.AutoThresholds()
    assert a.gammas == tuple(float(g) for g in ref.GAMMAS) and a.levels == 1
    assert a.candidates.tobytes() == ref.candidates().tobytes()
    for kw in (dict(gammas=()), dict(gammas=range(1, 18)), dict(gammas=(2, 1)), dict(gammas=(1, 1)), dict(gammas=(0, 1)),
               dict(gammas=(-1, 2)), dict(levels=0), dict(levels=5), dict(gammas=(1, float("inf")))):
        with pytest.raises(ValueError):
            capi.AutoThresholds(**kw)
    assert capi.pseudo_f(3 * 2 ** 29, 3, 3 * 2 ** 29) == pytest.approx(2 * 1.5 / 4.5) and capi.pseudo_f(0, 0, 0) == 0.0


def test_new_abi_symbols_and_the_memory_estimate():
    lib = C.CDLL(os.path.join(ROOT, "dafs_amd", "libdafs_hip.so"))
    for name in ("dafs_hip_consensus_structures_auto", "dafs_hip_nussinov_decode_auto", "dafs_host_structure_auto_bytes"):
        assert hasattr(lib, name), name
    from dafs_amd import capi
    for n, length in ((1, 1), (2, 170), (40, 300), (1, 12000)):
        lv = int(capi._structure_levels_bytes(n, length))
        sizes = [int(capi._structure_auto_bytes(n, length, c)) for c in (1, 2, 6, 16)]
        assert lv < sizes[0] and sizes == sorted(set(sizes))
        # every candidate has a structure of its own, one entry more than the columns, a score and a decoder descriptor
        assert all(s - lv >= c * (4 * (length + 1) + 4 + 72) for s, c in zip(sizes, (1, 2, 6, 16)))
        assert sizes[-1] - lv < 16 * (4 * length + 256) + 8192  # ... and not much more: the tables are shared
