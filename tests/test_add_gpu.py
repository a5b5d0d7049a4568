"""GPU tests of adding sequences to a fixed seed alignment (pipeline.add, `dafs --seed`): equal to a
normal run whose guide tree joins the new sequence last, each node the node it claims to be, the seed untouched, the
command line equal to Python, and the reliability annotation equal to its restatement."""
import os
import subprocess

import numpy as np
import pytest

import reliability_ref as rr
import text_ref
from dafs_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
NONE = 0xFFFFFFFF


def _split(recs):
    return [r[0] for r in recs], [r[1] for r in recs]


def run_cli(*args):
    r = subprocess.run([DAFS] + list(args), capture_output=True, text=True, timeout=600)
    return r.returncode, r.stdout, r.stderr


def _seed_of(res, rows_idx, names):
    """the printed rows rows_idx of a run as a seed: those rows without the columns that are gaps in all of them"""
    rows = [res.rows[r] for r in rows_idx]
    keep = [c for c in range(len(rows[0])) if any(row[c] != "-" for row in rows)]
    return [names[r] for r in rows_idx], ["".join(row[c] for c in keep) for row in rows]


def _leaves(left, right, i):
    return [i] if left[i] < 0 else _leaves(left, right, left[i]) + _leaves(left, right, right[i])


def test_equal_to_a_normal_run():
    """[a, b, s]: a and b from one family, s unrelated.  When the guide tree joins (a, b) first and s last, the root node
    is the add node, and add prints the normal run's output without its tree line, byte for byte"""
    from dafs_amd import capi, pipeline
    names, seqs = _split(synth.family_set(2, 80, seed=301) + [("s", synth.random_set(1, 80, seed=302)[0][1])])
    ctx = capi.Context(0)
    try:
        res = pipeline.run(names, seqs, ctx=ctx)
        score, left, right = res.tree
        assert left[4] == 2 and right[4] == 3 and left[3] == 0 and right[3] == 1  # the precondition
        snames, srows = _seed_of(res, [0, 1], names)
        got = pipeline.add(snames, srows, [names[2]], [seqs[2]], ctx=ctx)
        assert got.output == res.output.split("\n", 1)[1]
        assert got.dd_log[0] == res.dd_log[4]  # the root node's iterations, violations, consensus pairs and score
        assert got.rf.sum() == len(srows[0])
    finally:
        ctx.close()


def test_equal_to_a_normal_run_larger():
    """three family members and an outlier, over a fixed list of synth seeds: wherever the outlier is joined last (the
    root's left child) and the family's subtree lists its leaves in ascending order, add equals the normal run"""
    from dafs_amd import capi, pipeline
    hits = 0
    ctx = capi.Context(0)
    try:
        for sd in range(400, 416):
            names, seqs = _split(synth.family_set(3, 90, seed=sd) + [("out", synth.random_set(1, 90, seed=sd + 1000)[0][1])])
            res = pipeline.run(names, seqs, ctx=ctx)
            score, left, right = res.tree
            root = len(left) - 1
            if not (left[root] == 3 and _leaves(left, right, right[root]) == [0, 1, 2]):
                continue
            hits += 1
            snames, srows = _seed_of(res, [0, 1, 2], names)
            got = pipeline.add(snames, srows, [names[3]], [seqs[3]], ctx=ctx)
            assert got.output == res.output.split("\n", 1)[1], sd
    finally:
        ctx.close()
    assert hits >= 1


def _seed_and_new(k=4, seed=310):
    """a seed of 4 rows aligned by a run, and k new sequences of the same family"""
    from dafs_amd import pipeline
    names, seqs = _split(synth.family_set(4 + k, 80, seed=seed))
    res = pipeline.run(names[:4], seqs[:4])
    snames, srows = _seed_of(res, [0, 1, 2, 3], names)
    return snames, srows, names[4:], seqs[4:]


def test_nodes_and_merge():
    """k = 4: every z_j is Context.solve_nodes([(leaf j, seed)]) on the same stores, bit for bit; removing the new rows and
    the insert columns gives back the seed; every new row without gaps is its sequence"""
    from dafs_amd import capi, pipeline
    snames, srows, names, seqs = _seed_and_new()
    m, k = len(srows), len(seqs)
    ctx = capi.Context(0)
    try:
        res = pipeline.add(snames, srows, names, seqs, ctx=ctx)
        seed_mask = np.array([[ch != "-" for ch in r] for r in srows], np.uint8)
        seed_idx = np.arange(m, dtype=np.uint32)
        prm = capi.dd_params(skip_uncoupled_folds=1)
        outs = ctx.solve_nodes([(np.array([m + j], np.uint32), np.ones((1, len(seqs[j])), np.uint8), seed_idx, seed_mask)
                                for j in range(k)], prm)
        for j in range(k):
            assert res.z[j].dtype == np.uint32 and res.z[j].tobytes() == outs[j]["z"].tobytes(), j
            assert res.dd_log[j][0] == outs[j]["iterations"]
    finally:
        ctx.close()
    rows = res.output.split("\n")
    assert rows[0] == ">SS_cons" and rows[1] == res.ss_str
    assert rows[2::2][:m + k] == ["> " + n for n in snames + names]
    assert len(res.rows) == m + k and all(len(r) == len(res.rf) for r in res.rows)
    rf = np.asarray(res.rf, bool)
    assert ["".join(ch for ch, f in zip(r, rf) if f) for r in res.rows[:m]] == srows
    assert all(ch == "-" for r in res.rows[:m] for ch, f in zip(r, rf) if not f)
    assert [r.replace("-", "") for r in res.rows[m:]] == seqs


def _write_sto(path, names, rows, block=30):
    """an interleaved Stockholm file with '.' gaps and annotation lines"""
    w = max(len(n) for n in names) + 2
    lines = ["# STOCKHOLM 1.0", "#=GF ID seed"]
    for b in range(0, len(rows[0]), block):
        lines.append("")
        for n, r in zip(names, rows):
            lines.append(n.ljust(w) + r[b:b + block].replace("-", "."))
        lines.append("#=GC SS_cons".ljust(w) + "." * len(rows[0][b:b + block]))
    lines.append("//")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def test_cli_matches_python(tmp_path):
    from dafs_amd import pipeline, stockholm
    names, seqs = _split(synth.family_set(7, 90, seed=320))
    seed_fa, new_fa = str(tmp_path / "seed.fa"), str(tmp_path / "new.fa")
    with open(seed_fa, "w") as f:
        f.write(synth.to_fasta(list(zip(names[:4], seqs[:4]))))
    with open(new_fa, "w") as f:
        f.write(synth.to_fasta(list(zip(names[4:], seqs[4:]))))
    # the seed as `dafs seed.fa` prints it (aligned FASTA with the tree line and SS_cons) and as Stockholm
    rc, aln, err = run_cli(seed_fa)
    assert rc == 0, err
    seed_aln = str(tmp_path / "seed.aln")
    with open(seed_aln, "w") as f:
        f.write(aln)
    snames, srows = stockholm.read_seed(seed_aln)
    assert snames == names[:4]
    seed_sto = str(tmp_path / "seed.sto")
    _write_sto(seed_sto, snames, srows)
    assert stockholm.read_seed(seed_sto) == (snames, srows)
    # the reader is the command line's own: the restatement reads both files alike
    for seed in (seed_sto, seed_aln):
        assert text_ref.clean_seed(*text_ref.parse_seed(open(seed, "rb").read().decode("latin-1"))) == (snames, srows)
    want = pipeline.add(snames, srows, names[4:], seqs[4:], reliability=True)
    for seed in (seed_sto, seed_aln):
        out_sto = str(tmp_path / "out.sto")
        rc, out, err = run_cli("--seed", seed, "--stockholm", out_sto, new_fa)
        assert rc == 0, err
        assert out == want.output
        assert open(out_sto).read() == want.stockholm
        # and the block writer: the restatement builds the same bytes from the result's arrays
        assert open(out_sto).read() == text_ref.result_block(want, snames + names[4:], want.rf)
    assert "#=GC RF" in want.stockholm and "#=GF CC" not in want.stockholm
    # -f and --bp-update1 agree too
    for flags, kw in ((["-f", "0.5"], dict(w_pct_f=0.5)), (["--bp-update1"], dict(bp_update1=True))):
        rc, out, err = run_cli(*flags, "--seed", seed_sto, new_fa)
        assert rc == 0, err
        assert out == pipeline.add(snames, srows, names[4:], seqs[4:], **kw).output, flags
    # the refused combinations
    for flags in (["-r", "2"], ["--bp-update"], ["--devices", "0"], ["--fold-aux", "X"]):
        rc, out, err = run_cli(*flags, "--seed", seed_sto, new_fa)
        assert rc != 0 and "--seed" in err and out == "", flags


def test_reliability_against_restatement():
    from dafs_amd import capi, pipeline
    snames, srows, names, seqs = _seed_and_new(k=3, seed=330)
    ctx = capi.Context(0)
    try:
        res = pipeline.add(snames, srows, names, seqs, ctx=ctx, reliability=True)
        seq = np.arange(len(res.rows), dtype=np.uint32)
        mask = np.array([[ch != "-" for ch in row] for row in res.rows], np.uint8)
        want = rr.restate(seq, mask, res.ss, *rr.context_stores(ctx, 1, 1))
    finally:
        ctx.close()
    assert np.concatenate(res.reliability["residue"]).tobytes() == want["residue"].tobytes()
    for key in ("col", "pair", "pair_rows"):
        assert res.reliability[key].tobytes() == want[key].tobytes(), key
    assert np.float64(res.reliability["expected_accuracy"]).tobytes() == np.float64(want["expected_accuracy"]).tobytes()
