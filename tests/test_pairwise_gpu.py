"""GPU tests of the all-against-all pairwise mode: dafs_hip_pairs_from (the two-sequence families gathered on the device
from one N-sequence phase 1), pipeline.pairwise and `dafs --pairwise`.  Every pair must be, bit for bit, the plain run of
its two sequences."""
import os
import subprocess

import numpy as np
import pytest

import text_ref
from dafs_amd import capi, pipeline, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
RF00005 = os.path.join(G, "RF00005_0.fa")


def _fasta(path):
    """(name, sequence) records as the command line reads this simple layout: the name is the rest of the '>' line"""
    recs = []
    for line in open(path).read().splitlines():
        if line.startswith(">"):
            recs.append([line[1:], ""])
        elif recs:
            recs[-1][1] += line.strip()
    return [tuple(r) for r in recs]


def _mixed():
    """ten sequences of 40 to 300 nt: two synthetic families, unrelated random ones and two tRNAs"""
    recs = (synth.family_set(3, 60, seed=41) + synth.random_set(2, 40, seed=42) + synth.random_set(1, 300, seed=43, jitter=0.0)
            + synth.family_set(2, 150, seed=44) + _fasta(RF00005)[:2])
    return ["s%d_%s" % (k, n) for k, (n, _) in enumerate(recs)], [s for _, s in recs]


def _log(r):
    return {k: (v[0], v[1], v[2], np.float32(v[3]).tobytes()) for k, v in r.dd_log.items()}


def _same(got, want, stockholm=False):
    assert got.output == want.output
    assert _log(got) == _log(want)
    assert got.ss.tobytes() == want.ss.tobytes()
    assert got.rows == want.rows
    assert got.sim.tobytes() == want.sim.tobytes()
    if stockholm:
        assert got.stockholm == want.stockholm


def _mp_bytes(pp):
    return (pp.pair_x.tobytes(), pp.pair_y.tobytes(), pp.nnz.tobytes(), pp._rowptr.tobytes(), pp._col.tobytes(), pp._val.tobytes())


def _bp_bytes(rows):
    return [(r.tobytes(), c.tobytes(), v.tobytes()) for r, c, v in rows]


def _direct(seqs, pairs):
    """a context built directly with the 2P sequences of `pairs` as P families"""
    ref = capi.Context(0)
    ref.set_sequences([seqs[i] for pr in pairs for i in pr])
    if len(pairs) > 1:
        ref.set_families(np.arange(0, 2 * len(pairs) + 1, 2))
    ref.fold_posteriors(0.01)
    ref.align_posteriors(capi.ALIGN_PROBCONS, 0.01, fetch=False)
    return ref


def test_pairs_from_stores_equal_a_direct_build():
    _, seqs = _mixed()
    src = capi.Context(0)
    src.set_sequences(seqs)
    src.fold_posteriors(0.01)
    src.align_posteriors(capi.ALIGN_PROBCONS, 0.01, fetch=False)
    before = (_mp_bytes(src.mp(0)), _bp_bytes(src.bp(0)), src.sim().tobytes())
    dst = capi.Context(0)
    # sequences in several pairs, the 300-nt one, pairs out of row-major order
    pairs = [(0, 1), (2, 9), (0, 5), (5, 6), (3, 7), (1, 8)]
    dst.pairs_from(src, [x for x, _ in pairs], [y for _, y in pairs])
    ref = _direct(seqs, pairs)
    assert _mp_bytes(dst.mp(0)) == _mp_bytes(ref.mp(0))
    assert _bp_bytes(dst.bp(0)) == _bp_bytes(ref.bp(0))
    blocks = dst.sim_blocks()
    assert [b.tobytes() for b in blocks] == [b.tobytes() for b in ref.sim_blocks()]
    assert all(b[0, 1].tobytes() == src.sim()[x, y].tobytes() for b, (x, y) in zip(blocks, pairs))
    for c in (dst, ref):  # the family-aware transforms, unchanged, on both
        c.consistency_match(0.25)
        c.consistency_bp(0.25)
    assert _mp_bytes(dst.mp(1)) == _mp_bytes(ref.mp(1))
    assert _bp_bytes(dst.bp(1)) == _bp_bytes(ref.bp(1))
    # a second chunk from the same source, one pair, then the four-way transform (replaces the raw store and the scores)
    pairs = [(4, 9)]
    dst.pairs_from(src, [4], [9])
    ref.close()
    ref = _direct(seqs, pairs)
    for c in (dst, ref):
        c.fourway_consistency(0.3)
    assert _mp_bytes(dst.mp(0)) == _mp_bytes(ref.mp(0))
    assert [b.tobytes() for b in dst.sim_blocks()] == [b.tobytes() for b in ref.sim_blocks()]
    assert (_mp_bytes(src.mp(0)), _bp_bytes(src.bp(0)), src.sim().tobytes()) == before  # the source is left as it was
    for c in (src, dst, ref):
        c.close()


def test_every_pair_equals_a_two_sequence_run():
    names, seqs = _mixed()
    n = len(seqs)
    ctx = capi.Context(0)
    pw = pipeline.pairwise(names, seqs, ctx=ctx)
    assert pw.pairs == pipeline.all_pairs(n) and len(pw.results) == n * (n - 1) // 2
    assert pw.sim.shape == (n, n) and np.array_equal(pw.sim, pw.sim.T) and np.all(np.diag(pw.sim) == 1)
    assert np.all(np.isnan(np.diag(pw.score))) and np.all(np.diag(pw.iterations) == -1)
    for k, (x, y) in enumerate(pw.pairs):
        want = pipeline.run([names[x], names[y]], [seqs[x], seqs[y]], ctx=ctx)
        _same(pw.results[k], want)
        assert pw.sim[x, y].tobytes() == want.sim[0, 1].tobytes()
        assert pw.score[x, y].tobytes() == pw.score[y, x].tobytes() == np.float32(want.dd_log[2][3]).tobytes()
        assert pw.iterations[x, y] == pw.iterations[y, x] == want.dd_log[2][0]
    ctx.close()


@pytest.mark.parametrize("kw", [dict(align_model=capi.ALIGN_CONTRALIGN), dict(w_pct_f=0.1), dict(bp_update=True), dict(bp_update1=True),
                                dict(reliability=True)], ids=["contralign", "fourway", "bp_update", "bp_update1", "reliability"])
def test_options_equal_two_sequence_runs(kw):
    names, seqs = _mixed()
    pairs = [(0, 1), (3, 8), (2, 7), (8, 9)]
    ctx = capi.Context(0)
    pw = pipeline.pairwise(names, seqs, pairs=pairs, ctx=ctx, **kw)
    assert pw.pairs == pairs
    for k, (x, y) in enumerate(pairs):
        want = pipeline.run([names[x], names[y]], [seqs[x], seqs[y]], ctx=ctx, **kw)
        _same(pw.results[k], want, stockholm=kw.get("reliability", False))
    ctx.close()


def test_chunks_give_the_same_results():
    names, seqs = _mixed()
    names, seqs = names[:6], seqs[:6]
    whole = pipeline.pairwise(names, seqs)
    budget = 3 * min(pipeline.pair_bytes(len(seqs[x]), len(seqs[y])) for x, y in whole.pairs)
    parts = pipeline.pairwise(names, seqs, max_bytes=budget)
    assert len(whole.chunks) == 1 and len(parts.chunks) >= 10
    assert sorted(k for c in parts.chunks for k in c) == list(range(15))
    for a, b in zip(whole.results, parts.results):
        _same(a, b)
    assert whole.score.tobytes() == parts.score.tobytes() and np.array_equal(whole.iterations, parts.iterations)


def test_pairs_equal_the_oracle(oracle):
    names, seqs = _mixed()
    pairs = [(0, 1), (3, 4), (8, 9)]
    pw = pipeline.pairwise(names, seqs, pairs=pairs)
    # the solver as the reference runs it: with skip_uncoupled_folds (the default) a pair without consensus base pairs keeps
    # the oracle's text but not its iteration count and score (dafs_dd_params)
    full = pipeline.pairwise(names, seqs, pairs=pairs, skip_uncoupled_folds=False)
    coupled = 0
    for k, (x, y) in enumerate(pairs):
        pl = oracle.pipeline([names[x], names[y]], [seqs[x], seqs[y]], oracle.params(fold_model=0, align_model=0))
        pl.phase1(); pl.phase2()
        want = pl.output()
        its, viol, ncbp, score = pl.node_log()[2]  # the root: the pair's only node
        pl.close()
        assert pw.results[k].output == want, (x, y)
        assert full.results[k].output == want, (x, y)
        # the --pairwise-scores columns are the oracle's: solve_by_dd's return value, by its bytes, and its iteration count
        for r in [full] + ([pw] if ncbp else []):
            assert r.score[x, y].tobytes() == r.score[y, x].tobytes() == np.float32(score).tobytes(), (x, y, r.score[x, y], score)
            assert r.iterations[x, y] == r.iterations[y, x] == its, (x, y)
            assert r.results[k].dd_log[2][:3] == (its, viol, ncbp), (x, y)
        coupled += ncbp > 0
    assert coupled >= 1


def _cli(*args):
    r = subprocess.run([DAFS] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_cli_pairwise_equals_two_sequence_files(tmp_path):
    """headers plus each pair's plain `dafs` stdout; --stockholm one block per pair; --pairwise-scores the Python writer's bytes"""
    recs = _fasta(RF00005)[:5]
    fa = tmp_path / "five.fa"
    fa.write_text(synth.to_fasta(recs))
    sto, tsv = tmp_path / "pw.sto", tmp_path / "pw.tsv"
    out = _cli("--pairwise", "--stockholm", sto, "--pairwise-scores", tsv, fa)
    want, want_sto = "", ""
    for x in range(len(recs)):
        for y in range(x + 1, len(recs)):
            two, two_sto = tmp_path / ("p%d_%d.fa" % (x, y)), tmp_path / ("p%d_%d.sto" % (x, y))
            two.write_text(synth.to_fasta([recs[x], recs[y]]))
            want += "==> %d %d <==\n" % (x + 1, y + 1) + _cli("--stockholm", two_sto, two)
            want_sto += two_sto.read_text()
    assert out == want
    assert sto.read_text() == want_sto
    names, seqs = [n for n, _ in recs], [s for _, s in recs]
    pw = pipeline.pairwise(names, seqs)
    assert tsv.read_bytes() == pipeline.pairwise_scores_tsv(names, pw.pairs, pw.sim, pw.score, pw.iterations).encode()
    # that writer is the command line's own: the restatement builds the same bytes from the result's arrays
    assert tsv.read_bytes() == text_ref.pairwise_scores_tsv(names, pw.pairs, pw.sim, pw.score, pw.iterations).encode()
    assert out == "".join("==> %d %d <==\n" % (x + 1, y + 1) + r.output for (x, y), r in zip(pw.pairs, pw.results))


def test_cli_pairwise_rf00005_prints_45_blocks():
    recs = _fasta(RF00005)
    out = _cli("--pairwise", RF00005)
    assert out.count("==> ") == 45
    pw = pipeline.pairwise([n for n, _ in recs], [s for _, s in recs])
    assert out == "".join("==> %d %d <==\n" % (x + 1, y + 1) + r.output for (x, y), r in zip(pw.pairs, pw.results))


def test_cli_two_sequences_give_one_block(tmp_path):
    fa = tmp_path / "two.fa"
    fa.write_text(synth.to_fasta(_fasta(RF00005)[3:5]))
    assert _cli("--pairwise", fa) == "==> 1 2 <==\n" + _cli(fa)


def test_refused_pairs_from_leaves_both_contexts_usable():
    names, seqs = _mixed()
    names, seqs = names[:4], seqs[:4]
    src, dst = capi.Context(0), capi.Context(0)

    def refused(a, px, py):
        with pytest.raises(capi.DafsHipError, match=r"code -1\b"):
            dst.pairs_from(a, px, py)
    src.set_sequences(seqs)
    src.set_families([0, 2, 4])  # two families
    src.fold_posteriors(0.01)
    src.align_posteriors(fetch=False)
    refused(src, [0], [1])
    src.set_sequences(seqs)  # no base-pairing store
    src.align_posteriors(fetch=False)
    refused(src, [0], [1])
    src.fold_posteriors(0.01)
    src.align_posteriors(pair_begin=0, pair_end=3, fetch=False)  # a partial matching store
    refused(src, [0], [1])
    src.align_posteriors(fetch=False)  # complete now
    refused(src, [1], [1])
    refused(src, [2], [1])
    refused(src, [0], [4])
    with pytest.raises(capi.DafsHipError, match=r"code -1\b"):
        src.pairs_from(src, [0], [1])
    # both go on: dst takes two pairs and runs the transforms, src a plain run
    dst.pairs_from(src, [0, 2], [3, 3])
    dst.consistency_match(0.25)
    dst.consistency_bp(0.25)
    assert list(dst.mp(1).pair_x) == [0, 2] and list(dst.mp(1).pair_y) == [1, 3]
    got = pipeline.run(names[:2], seqs[:2], ctx=src)
    assert got.output == pipeline.run(names[:2], seqs[:2]).output
    src.close()
    dst.close()
