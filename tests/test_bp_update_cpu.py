"""CPU tests of the --bp-update cases (bp_update_cases.py): that orc_pipeline_update_basepairing and
orc_pipeline_average_basepairing are the reference's two functions (dafs.cpp:561-607, :609-712) restated in numpy, bit for bit;
that every case reaches what it is for; that the cases tell each rule of the update from a near miss; and that the whole
runs of the command-line test are not vacuous.  The part test_pct_edges_cpu.py has for the consistency-transform cases."""
import numpy as np
import pytest

import bp_update_cases as B

NONE = B.NONE


@pytest.fixture(scope="module")
def pipes(oracle):
    """per case the oracle's pipeline on the supplied free rows, its plain average and its updated matrix (read-only)"""
    out = {}
    for key in B.KEYS:
        c = B.CASES[key]
        pl = B.oracle_pipeline(oracle, c)
        avg = pl.average_basepairing(c.idx, c.mask)
        upd = pl.update_basepairing(c.idx, c.mask, c.ss)
        avg.flags.writeable = False
        upd.flags.writeable = False
        out[key] = (pl, avg, upd)
    yield out
    for pl, _, _ in out.values():
        pl.close()


def _strings(c):
    text = B.brackets(c.ss)
    return [B.constraint(c.mask[r], c.ss, text) for r in range(c.n)]


def _forced(con):
    """the pairs (i, j) of a constraint string, in residues"""
    open_, out = [], []
    for k, ch in enumerate(con):
        if ch == "(":
            open_.append(k)
        elif ch == ")":
            out.append((open_.pop(), k))
    assert not open_
    return out


def test_the_decoders_convention(oracle, pipes):
    """ss[i] = j at the left column only (oracle/decoders.c:66,70): what the cases' ss follows"""
    for key in ("mid", "wide"):
        _, ss = oracle.nussinov(pipes[key][1], None, B.TH)
        left = np.flatnonzero(ss != NONE)
        assert len(left) >= 1, key  # the first decode of the chain in test_bp_update_gpu.py holds a pair
        assert np.all(ss[left] > left) and np.all(ss[ss[left]] == NONE), key
    for c in B.CASES.values():
        left = np.flatnonzero(c.ss != NONE)
        assert np.all(c.ss[left] > left) and np.all(c.ss[c.ss[left]] == NONE)
        assert B.brackets(c.ss).count("(") == len(c.pairs) == len(left)


@pytest.mark.parametrize("key", B.KEYS)
def test_entry_points_equal_the_restatement(oracle, pipes, key):
    c = B.CASES[key]
    _, avg, upd = pipes[key]
    assert avg.tobytes() == B.restated_average(oracle, c).tobytes()
    assert upd.tobytes() == B.restated_update(oracle, c).tobytes()


@pytest.mark.parametrize("key", B.KEYS)
def test_case_reaches_what_it_is_for(pipes, key):
    c = B.CASES[key]
    _, avg, upd = pipes[key]
    assert c.n in (3, 5) and len(c.seqs) == c.n + 2
    # row r, its sequence idx[r] and sequence r of the context are three things; the context's first two are in no row
    assert all(int(c.idx[r]) != r for r in range(c.n)) and list(c.idx) != sorted(c.idx) and min(c.idx) == 2
    for m in (avg, upd):
        assert np.all(np.isfinite(m)) and not np.any(np.tril(m)) and np.any(m)
    if key == "none":
        assert not c.pairs and set("".join(_strings(c))) == {"?"}
        assert upd.tobytes() == avg.tobytes()  # free folds, averaged at the same cut-off
        return
    assert upd.tobytes() != avg.tobytes()
    cons = _strings(c)
    forced = [_forced(s) for s in cons]
    assert any(len(f) == len(c.pairs) for f in forced)  # a row that forces every pair
    gap_drop = [sum(1 for i, j in c.pairs if c.mask[r, i] != c.mask[r, j]) for r in range(c.n)]
    assert any(gap_drop) and all(len(f) + sum(1 for i, j in c.pairs if not (c.mask[r, i] and c.mask[r, j])) == len(c.pairs) for r, f in enumerate(forced))
    if key == "small":
        assert [s for s in cons if len(s) == 2] == ["??"]
    if key == "mid":
        assert c.ss[0] == c.L - 1 and sorted(int(v) for v in c.mask.sum(1)) == [63, 64, 65]
    if key == "wide":
        assert sum("()" in s for s in cons) == 1  # the pair (100, 230) of the row without the columns between them
        seq = c.seqs[c.idx[2]]
        assert sum(seq[i] + seq[j] not in B.PAIRS for i, j in forced[2]) >= 2  # forced pairs that cannot form
        for r in (0, 1, 3):
            seq = c.seqs[c.idx[r]]
            assert all(seq[i] + seq[j] in B.PAIRS for i, j in forced[r]), r


@pytest.mark.parametrize("rule", B.RULES)
def test_cases_tell_the_rules_apart(oracle, pipes, rule):
    """the restatement with one rule altered differs from the oracle on at least one case"""
    differs = [key for key in B.KEYS if B.restated_update(oracle, B.CASES[key], rule=rule).tobytes() != pipes[key][2].tobytes()]
    assert differs, rule


def test_refusals(oracle, pipes):
    c = B.CASES["small"]
    pl, avg, upd = pipes["small"]
    short = c.mask.copy()
    short[1, np.flatnonzero(short[1])[0]] = 0
    beyond = c.idx.copy()
    beyond[2] = len(c.seqs)
    for idx, mask in ((c.idx, short), (beyond, c.mask)):
        out = np.full((c.L, c.L), -7.5, np.float32)
        assert pl.average_basepairing(idx, mask, out=out) == -1 and np.all(out == -7.5)
        assert pl.update_basepairing(idx, mask, c.ss, out=out) == -1 and np.all(out == -7.5)
    bad_ss = c.ss.copy()
    bad_ss[5] = c.L
    out = np.full((c.L, c.L), -7.5, np.float32)
    assert pl.update_basepairing(c.idx, c.mask, bad_ss, out=out) == -1 and np.all(out == -7.5)
    bare = B.oracle_pipeline(oracle, c, with_rows=False)  # no base-pairing store: nothing to average, but the update folds for itself
    try:
        assert bare.average_basepairing(c.idx, c.mask, out=out) == -1 and np.all(out == -7.5)
        assert bare.update_basepairing(c.idx, c.mask, c.ss).tobytes() == upd.tobytes()
    finally:
        bare.close()
    assert pl.average_basepairing(c.idx, c.mask).tobytes() == avg.tobytes()


@pytest.mark.parametrize("which", [0, 1], ids=["RF00005_0", "structured"])
def test_whole_runs_are_not_vacuous(oracle, tmp_path, which):
    """both flags change the oracle's output on the inputs test_cli_gpu.py::test_fourway_and_bp_update_flags adds"""
    key, text = B.whole_run_inputs()[which]
    fa = tmp_path / (key + ".fa")
    fa.write_text(text)
    recs = oracle.fasta(str(fa))
    names, seqs = [n for n, _ in recs], [s for _, s in recs]
    out = {}
    for flag in (None, "bp_update", "bp_update1"):
        pl = oracle.pipeline(names, seqs, oracle.params(fold_model=0, **({flag: 1} if flag else {})))
        pl.phase1(); pl.phase2()
        out[flag] = pl.output()
        pl.close()
    assert out["bp_update"] != out[None] and out["bp_update1"] != out[None]
