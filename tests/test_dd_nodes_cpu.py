"""The conditions of the node-level solver tests (test_dd_nodes_gpu.py), checked without a GPU: the shape table reaches every
plan class the planner has up to 1025 columns, the inputs keep the oracle's solver busy and meet ties, and the oracle's
node-level entry point (orc_pipeline_solve_node) is the solve its own pipeline runs."""
import os

import numpy as np

import dd_nodes_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF


def _default_switches(monkeypatch):
    for name in R.ALL_SWITCHES:
        monkeypatch.delenv("DAFS_HIP_DD_" + name, raising=False)


def _fixture_classes():
    """{(L1, L2): (lds_flags, fold_fast)} of the default-switch rows of the fixture with both sides <= 1025"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "dd_node_plan.npz"))
    cols = [str(c) for c in g["columns"]]
    assert cols[:5] == ["switch", "L1", "L2", "lds_flags", "fold_fast"] and str(g["switches"][0]) == ""
    rows = g["plans"][g["plans"][:, 0] == 0]
    return {(int(r[1]), int(r[2])): (int(r[3]), int(r[4])) for r in rows if max(r[1], r[2]) <= 1025}


def test_the_table_reaches_every_plan_class(monkeypatch):
    _default_switches(monkeypatch)
    recorded = _fixture_classes()
    classes = set(recorded.values())
    assert len(classes) == 29                         # the fixture as it is now; a new form must come with its shapes
    planned = {s: R.plan_class(*s) for s in R.TABLE}  # through the planner itself, as nodes_open runs it
    for s, c in planned.items():
        assert recorded.get(s, c) == c, s
    assert set(planned.values()) >= classes, sorted(classes - set(planned.values()))
    # per class the smallest shape whose short side is at least 30 (63 on the fixture's grid) ...
    by_class = {}
    for s, c in recorded.items():
        if min(s) >= 30:
            by_class.setdefault(c, []).append(s)
    assert set(by_class) == classes
    smallest = {min(v, key=lambda s: (s[0] * s[1], s[0])) for v in by_class.values()}
    assert smallest <= set(R.SHAPES), sorted(smallest - set(R.SHAPES))
    assert min(min(s) for s in smallest) == 63
    # ... its mirror wherever the two classes differ, nothing else, and the degenerate shapes
    for a, b in R.SHAPES:
        if recorded[(a, b)] != recorded[(b, a)]:
            assert (b, a) in R.SHAPES, (a, b)
        assert (a, b) in smallest or (b, a) in smallest, (a, b)
    assert len(set(R.TABLE)) == len(R.TABLE)
    assert set(R.DEGENERATE) == {(1, 1), (1, 2), (2, 1), (1, 65), (1, 769), (769, 1), (1025, 1)}
    # the quantised cases: one table shape per form family, no two in one class
    assert set(R.FAMILIES.values()) <= set(R.SHAPES)
    assert len({planned[s] for s in R.FAMILIES.values()}) == len(R.FAMILIES)


def test_the_cases_keep_the_solver_busy(oracle):
    """on the recipe's inputs the oracle alone: consensus pairs and at least 3 iterations wherever both sides have 30 columns;
    over the table one case at least settles before its cap and a third at least runs into it"""
    settled = capped = 0
    for L1, L2 in R.TABLE:
        case = R.cached(R.shape_case, L1, L2)
        assert 3 <= case.t_max <= 25 or (case.t_max == 600 and max(L1, L2) < 100)
        o = R.reference(oracle, case)[0]
        if min(L1, L2) >= 30:
            assert o["ncbp"] > 0 and o["iterations"] >= 3, (L1, L2, o["ncbp"], o["iterations"])
            settled += o["violated"] == 0 and o["iterations"] < case.t_max   # a coupled node whose multipliers settle
        else:
            assert o["ncbp"] == 0
        capped += o["iterations"] == case.t_max
        assert (o["z"] != NONE).sum() > 0, (L1, L2)
    assert settled >= 1
    assert 3 * capped >= len(R.TABLE)
    assert sum(R.t_max_of(*s) == 600 for s in R.SHAPES) in (1, 2, 3)   # "a few shapes below 100 columns"


def test_the_quantised_cases_meet_ties(oracle):
    """in every quantised case the first iteration's DPs (multipliers zero) meet equal float sums: two predecessors of an
    alignment cell, and two candidates of a folding cell of which one closes or joins a pair"""
    cases = [R.cached(R.shape_case, L1, L2, True) for L1, L2 in R.FAMILIES.values()] + [R.cached(R.supplied_case, *s) for s in R.SUPPLIED_SHAPES]
    for case in cases:
        p_x, p_y, p_z = R.averaged(oracle, case)
        for p in (p_x, p_y, p_z):
            assert np.array_equal(p * 8, np.round(p * 8))
        assert R.alignment_ties(oracle, p_z) > 0, case.key
        short = p_x if p_x.shape[0] <= p_y.shape[0] else p_y         # the replay is plain Python: the shorter side will do
        w = 4.0 * 2 * 1 / (1 + 1)
        assert R.folding_ties(short, w) > 0, case.key
        o = R.reference(oracle, case)[0]
        assert o["ncbp"] > 0 and o["iterations"] >= 3, case.key


def test_multi_row_and_supplied_inputs_are_what_they_claim(oracle):
    for nseq in (5, 9):
        for L1, L2 in R.MULTIROW_SHAPES:
            case = R.cached(R.multirow_case, nseq, L1, L2)
            i1, m1, i2, m2 = case.nodes[0]
            assert sorted(list(i1) + list(i2)) == list(range(nseq)) and 2 <= len(i1) <= 5 and 2 <= len(i2) <= 5
            for idx, m, L in ((i1, m1, L1), (i2, m2, L2)):
                assert m.shape == (len(idx), L) and m.any(axis=0).all()
                assert [int(v) for v in m.sum(axis=1)] == [len(case.seqs[i]) for i in idx]
                assert (m == 0).any()
            o = R.reference(oracle, case)[0]
            assert o["ncbp"] > 0 and o["iterations"] >= 3, case.key
    spans = [R.plan_class(*s) for s in R.MULTIROW_SHAPES]
    assert spans[0][0] & 64 and not spans[1][0] & 64 and max(R.MULTIROW_SHAPES[2]) > 1024
    for s in R.SUPPLIED_SHAPES:
        case = R.cached(R.supplied_case, *s)
        p_x, p_y = case.nodes[0][4:]
        assert p_x.shape == (s[0], s[0]) and p_y.shape == (s[1], s[1])
        assert (p_x > 0).sum() > 2 * s[0] and (p_y > 0).sum() > 2 * s[1]        # denser than the stores' rows
        plain = R.reference(oracle, R.cached(R.shape_case, s[0], s[1], True))[0]
        o = R.reference(oracle, case)[0]
        assert o["ncbp"] > 0 and o["ncbp"] != plain["ncbp"]                     # the supplied matrices are what it solved


def _z_of_rows(row1, row2, L1):
    """the column map z of the first sequence that two printed rows imply"""
    z = np.full(L1, NONE, np.uint32)
    i = k = 0
    for a, b in zip(row1, row2):
        if a != "-" and b != "-":
            z[i] = k
        i += a != "-"
        k += b != "-"
    return z


def test_solve_node_is_the_pipelines_own_solve(oracle):
    """for two-sequence pipelines -- one on ProbCons + CONTRAfold, one on supplied stores -- orc_pipeline_solve_node(leaf 0,
    leaf 1) gives what the node log holds for the root after phase 2, and the z the printed rows imply; the entry point
    leaves the log alone, and orc_pipeline_dd_log is the node log's first two columns"""
    recs = oracle.fasta(os.path.join(ROOT, "tests", "golden", "RF00005_0.fa"))[:2]   # two tRNAs: they share a structure
    names, seqs = [n for n, _ in recs], [s for _, s in recs]
    model = oracle.pipeline(names, seqs, oracle.params())
    model.phase1()
    supplied_case = R.cached(R.shape_case, 63, 65)
    supplied = R.oracle_pipeline(oracle, supplied_case)
    for pl, sq in ((model, seqs), (supplied, supplied_case.seqs)):
        node = (np.array([0], np.uint32), np.ones((1, len(sq[0])), np.uint8), np.array([1], np.uint32), np.ones((1, len(sq[1])), np.uint8))
        o = pl.solve_node(*node)
        assert pl.node_log() == {}
        pl.phase2()
        log = pl.node_log()
        assert list(log) == [2]
        it, vi, ncbp, score = log[2]
        assert (o["iterations"], o["violated"], o["ncbp"]) == (it, vi, ncbp) and o["score"].tobytes() == score.tobytes()
        assert ncbp > 0 and it >= 3
        rows = pl.output().splitlines()
        assert rows[3] == "> " + (names if pl is model else ["s0", "s1"])[0]
        assert np.array_equal(o["z"], _z_of_rows(rows[4], rows[6], len(sq[0])))
        again = pl.solve_node(*node)
        assert R.first_difference(again, o) is None and pl.node_log() == log
        d_it, d_vi = pl.dd_log()
        assert [int(v) for v in d_it] == [it] and [int(v) for v in d_vi] == [vi]
        pl.close()


def test_node_log_names_the_guide_tree_nodes(oracle):
    """the node log of a whole run: one entry per internal node, children before parents, in the order of orc_pipeline_dd_log"""
    from test_oracle_cpu import _golden_bp
    recs = oracle.fasta(os.path.join(ROOT, "tests", "golden", "RF00005_0.fa"))
    names, seqs = [n for n, _ in recs], [s for _, s in recs]
    pl = oracle.pipeline(names, seqs, oracle.params(fold_model=1), bp=_golden_bp(seqs))
    pl.phase1(); pl.phase2()
    log = pl.node_log()
    _, left, right = pl.tree()
    n = len(seqs)
    assert sorted(log) == list(range(n, 2 * n - 1))
    order = list(log)
    for k, node in enumerate(order):
        for child in (int(left[node]), int(right[node])):
            assert child < n or child in order[:k]
    it, vi = pl.dd_log()
    assert [log[k][0] for k in order] == [int(v) for v in it] and [log[k][1] for k in order] == [int(v) for v in vi]
    pl.close()


def test_first_difference_names_the_output():
    a = dict(x=np.array([1, NONE], np.uint32), y=np.array([NONE], np.uint32), z=np.array([0, 1], np.uint32), score=np.float32(1.5), ncbp=3,
             iterations=4, violated=0)
    assert R.first_difference(a, dict(a)) is None
    assert R.first_difference(a, dict(a, z=np.array([0, NONE], np.uint32))).startswith("z differs first at column 1: 1, oracle -1")
    assert R.first_difference(a, dict(a, score=np.nextafter(np.float32(1.5), np.float32(2)))).startswith("score differs")
    assert R.first_difference(a, dict(a, ncbp=2, violated=1)) == "ncbp differs: 3, oracle 2"
    assert R.first_difference(a, dict(a, ncbp=2), outputs=("z",)) is None
