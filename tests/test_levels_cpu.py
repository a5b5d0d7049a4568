"""CPU tests of the level-by-level decode's contract: the numpy restatement of tests/levels_ref.py on
random matrices and on hand-made cases whose structure and levels are written out.  No device: these pin the contract the
GPU tests compare the library with."""
import numpy as np
import pytest

import levels_ref as ref

NONE, FREE = ref.NONE, ref.FREE
THS = (0.2, 0.15, 0.1, 0.05)


def _random_matrix(rs, L, quarters):
    p = np.triu(rs.rand(L, L).astype(np.float32), 1) if L else np.zeros((0, 0), np.float32)
    p[rs.rand(L, L) < 0.55] = 0
    if quarters:
        p = (np.round(p * 4) / 4).astype(np.float32)
    return p


@pytest.fixture(scope="module")
def random_cases(oracle):
    """(p, K, restatement) for L = 0 .. 33, a third of them rounded to quarters so that ties occur; built once"""
    rs = np.random.RandomState(25)
    cases = []
    for L in range(34):
        p = _random_matrix(rs, L, quarters=(L % 3 == 1))
        K = 1 + L % 4
        cases.append((p, K, ref.decode(oracle, p, THS[:K])))
    return cases


def test_level_0_is_the_plain_decode(random_cases, oracle):
    for p, K, (scores, merged, level, per_level) in random_cases:
        if p.shape[0] == 0:
            continue
        s, ss = oracle.nussinov(p, None, THS[0])
        assert per_level[0].tobytes() == ss.tobytes() and scores[0].tobytes() == np.float32(s).tobytes()
        assert np.array_equal(merged[level == 0], ss[level == 0])


def test_constraints_of_the_program_hold(random_cases):
    knots = 0
    for p, K, (scores, merged, level, per_level) in random_cases:
        L = p.shape[0]
        used = np.zeros(L, int)
        for k, ss in enumerate(per_level):
            prs = ref.pairs_of(ss)
            for i, j in prs:
                used[i] += 1
                used[j] += 1
                assert p[i, j] - np.float32(THS[k]) > 0
                assert level[i] == level[j] == k and merged[i] == j
                for u in range(k):  # constraint 3: a pair of level k crosses a pair of every lower level
                    assert any(ref.crosses(a, b, i, j) for a, b in ref.pairs_of(per_level[u])), (L, k, u, i, j)
                    knots += 1
            for x, (i, j) in enumerate(prs):  # constraint 2: no crossing inside a level
                assert not any(ref.crosses(a, b, i, j) for a, b in prs[x + 1:])
        assert used.max(initial=0) <= 1  # constraint 1
        assert np.array_equal(level == FREE, used == 0)
        assert np.all(merged[level == FREE] == NONE)
    assert knots > 20  # the cases do produce crossing pairs


def test_enclosers_decide_the_crossing(random_cases):
    """for columns i, j unpaired at level u: (i, j) crosses a level-u pair exactly when their innermost enclosing pairs
    differ -- on every cell of every case"""
    cells = 0
    for p, K, (scores, merged, level, per_level) in random_cases:
        L = p.shape[0]
        for ss in per_level:
            enc = ref.enclosers(ss)
            prs = ref.pairs_of(ss)
            free = np.ones(L, bool)
            for a, b in prs:
                free[a] = free[b] = False
            for i in range(L):
                for j in range(i + 1, L):
                    if free[i] and free[j]:
                        assert (enc[i] != enc[j]) == any(ref.crosses(a, b, i, j) for a, b in prs)
                        cells += 1
    assert cells > 1000


def test_levels_above_an_empty_level_are_empty(random_cases, oracle):
    seen = 0
    for p, K, (scores, merged, level, per_level) in random_cases:
        for k in range(1, K):
            if not ref.pairs_of(per_level[k - 1]):
                assert not ref.pairs_of(per_level[k]) and scores[k] == 0
                seen += 1
    assert seen > 0
    # and one made for it: nothing above the first threshold
    p = np.zeros((9, 9), np.float32)
    p[0, 8] = p[2, 6] = 0.1
    scores, merged, level, per_level = ref.decode(oracle, p, (0.5, 0.05, 0.05))
    assert np.all(merged == NONE) and np.all(level == FREE) and np.all(scores == 0)


def test_scores_are_the_sums_over_the_levels_pairs(random_cases):
    checked = 0
    for p, K, (scores, merged, level, per_level) in random_cases:
        for k, ss in enumerate(per_level):
            prs = ref.pairs_of(ss)
            th = np.float32(THS[k])
            in_double = sum(float(np.float32(p[i, j] - th)) for i, j in prs)
            # the decoder adds in float32 along its own tree; the double sum agrees to the rounding of those additions
            assert abs(float(scores[k]) - in_double) <= len(prs) * 2.0 ** -23 * max(in_double, 1.0)
            assert scores[k].tobytes() == ref.tree_score(p, ss, th).tobytes(), (p.shape[0], k)
            checked += len(prs)
    assert checked > 50


@pytest.mark.parametrize("case", ref.hand_cases(), ids=lambda c: c.name)
def test_hand_made_cases(case, oracle):
    scores, merged, level, per_level = ref.decode(oracle, case.p, case.ths)
    assert merged.tolist() == case.ss.tolist() and level.tolist() == case.level.tolist()
    for k, prs in enumerate(case.by_level):
        assert ref.pairs_of(per_level[k]) == sorted(prs)
        assert scores[k].tobytes() == ref.tree_score(case.p, per_level[k], case.ths[k]).tobytes()
    assert ref.brackets(merged, level) == case.text
    from dafs_amd import capi  # host code only
    assert capi.make_brackets_levels(case.ss, case.level) == case.text


def test_absent_cells_of_the_hand_made_cases():
    by_name = {c.name: c for c in ref.hand_cases()}
    c = by_name["crosses-nothing"]
    assert c.p[8, 12] - np.float32(c.ths[1]) > c.p[3, 10] - np.float32(c.ths[1]) > 0 and c.ss[8] == NONE and c.level[12] == FREE
    assert not ref.crosses(0, 6, 8, 12) and ref.crosses(3, 10, 8, 12)
    c = by_name["k3"]
    assert c.p[2, 15] > c.ths[2] and c.ss[2] == NONE  # crosses level 0's (0,5), not level 1's (3,12): absent from level 2
    assert ref.crosses(0, 5, 2, 15) and not ref.crosses(3, 12, 2, 15)
    c = by_name["column-taken"]
    assert c.p[5, 11] > c.p[2, 9] and c.ss[5] == NONE and c.level[5] == 0  # column 5 is level 0's
