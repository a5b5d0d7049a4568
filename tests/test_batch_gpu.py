"""GPU tests of the many-family batch: pipeline.run_batch and the family partition of a context (dafs_hip_set_families)
against separate one-family runs, bit for bit, and `dafs A B C` against separate `dafs A`, `dafs B`, `dafs C`."""
import os
import subprocess

import numpy as np
import pytest

from dafs_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")


def _fasta(path):
    names, seqs, cur = [], [], None
    with open(path) as fh:
        for line in fh:
            line = line.rstrip("\n")
            if line.startswith(">"):
                names.append(line[1:].strip())
                seqs.append("")
            elif line:
                seqs[-1] += line.strip()
    return names, seqs


def _split(recs):
    return [r[0] for r in recs], [r[1] for r in recs]


def _mixed():
    fams = [_fasta(os.path.join(G, "RF00005_0.fa")), _fasta(os.path.join(G, "RF00017_4.fa"))]
    fams.append(_split(synth.random_set(1, 40, seed=31)))
    fams.append(_split(synth.family_set(2, 300, seed=32)))
    fams.append(_split(synth.random_set(3, 120, seed=33)))
    fams.append(_split(synth.family_set(8, 90, seed=34)))
    fams.append(_split(synth.family_set(24, 60, seed=35)))
    return fams


def _ctx():
    from dafs_amd import capi
    return capi.Context(0)


def _oracle_output(oracle, names, seqs, **kw):
    pl = oracle.pipeline(names, seqs, oracle.params(fold_model=0, **kw))
    pl.phase1(); pl.phase2()
    out = pl.output()
    pl.close()
    return out


def test_mixed_batch_equals_separate_runs(oracle):
    from dafs_amd import pipeline
    fams = _mixed()
    ctx = _ctx()
    try:
        got = pipeline.run_batch(fams, ctx=ctx)
        assert len(got) == len(fams)
        for (names, seqs), r in zip(fams, got):
            one = pipeline.run(names, seqs, ctx=ctx)
            assert r.output == one.output, names[0]
            assert r.dd_log == one.dd_log, names[0]
            assert all(a.tobytes() == b.tobytes() for a, b in zip(r.sim, one.sim))
            if 2 <= len(seqs) <= 10:
                assert r.output == _oracle_output(oracle, names, seqs), names[0]
    finally:
        ctx.close()


@pytest.mark.parametrize("kw", [dict(w_pct_a=0.25, w_pct_s=0.25), dict(w_pct_a=0.4, w_pct_s=0.1, w_pct_f=0.1)])
def test_stores_equal_one_family_contexts(kw):
    """the relaxed and un-relaxed stores of every family, bit for bit, against a context holding that family alone: what a
    wrong z range or a weight taken from the whole batch would break"""
    from dafs_amd import capi, pipeline
    fams = [_split(synth.family_set(5, 70, seed=41)), _split(synth.random_set(2, 50, seed=42)), _split(synth.random_set(1, 30, seed=43)),
            _split(synth.family_set(9, 110, seed=44))]
    seqs, first = [], [0]
    for _, s in fams:
        seqs += s
        first.append(len(seqs))
    args = (capi.ALIGN_PROBCONS, 0.01, kw["w_pct_a"], kw["w_pct_s"])
    ctx, one = _ctx(), _ctx()
    try:
        sims = pipeline._phase1_local(ctx, seqs, None, None, *args, [], kw.get("w_pct_f", 0.0), first)
        mp = [ctx.mp(0), ctx.mp(1)]
        bp = [ctx.bp(0), ctx.bp(1)]
        p0 = 0
        for f, (_, s) in enumerate(fams):
            sim1 = pipeline._phase1_local(one, s, None, None, *args, [], kw.get("w_pct_f", 0.0))
            assert sims[f].tobytes() == sim1.tobytes()
            np_f = len(s) * (len(s) - 1) // 2
            for relaxed in (0, 1):
                ref = one.mp(relaxed)
                assert len(ref) == np_f
                for p in range(np_f):
                    assert mp[relaxed].pair_x[p0 + p] == ref.pair_x[p] + first[f]
                    assert mp[relaxed].pair_y[p0 + p] == ref.pair_y[p] + first[f]
                    for tr in (False, True):
                        a, b = mp[relaxed].csr(p0 + p, tr), ref.csr(p, tr)
                        assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b)), (f, relaxed, p, tr)
                rb = one.bp(relaxed)
                for k in range(len(s)):
                    assert all(u.tobytes() == v.tobytes() for u, v in zip(bp[relaxed][first[f] + k], rb[k])), (f, relaxed, k)
            p0 += np_f
        assert p0 == len(mp[0])
    finally:
        ctx.close()
        one.close()


def test_contralign_bp_update_batch():
    from dafs_amd import capi, pipeline
    fams = [_fasta(os.path.join(G, "RF00005_0.fa")), _split(synth.family_set(4, 80, seed=51)), _split(synth.random_set(2, 60, seed=52))]
    kw = dict(align_model=capi.ALIGN_CONTRALIGN, bp_update=True)
    ctx = _ctx()
    try:
        got = pipeline.run_batch(fams, ctx=ctx, **kw)
        for (names, seqs), r in zip(fams, got):
            one = pipeline.run(names, seqs, ctx=ctx, **kw)
            assert r.output == one.output and r.dd_log == one.dd_log
    finally:
        ctx.close()


def test_order_and_packing_invariance():
    from dafs_amd import pipeline
    fams = [_split(synth.family_set(n, L, seed=60 + n)) for n, L in ((3, 70), (6, 50), (2, 90), (5, 60))]
    ctx = _ctx()
    try:
        base = pipeline.run_batch(fams, ctx=ctx)
        perm = [2, 0, 3, 1]
        got = pipeline.run_batch([fams[k] for k in perm], ctx=ctx)
        for j, k in enumerate(perm):
            assert got[j].output == base[k].output and got[j].dd_log == base[k].dd_log
        alone = pipeline.run_batch(fams, ctx=ctx, max_bytes=1)  # one family per sub-batch
        for a, b in zip(alone, base):
            assert a.output == b.output and a.dd_log == b.dd_log
    finally:
        ctx.close()


def _run_cli(*args):
    r = subprocess.run([DAFS] + list(args), capture_output=True, text=True, timeout=600)
    return r.returncode, r.stdout, r.stderr


def test_cli_several_files(tmp_path):
    """`dafs A B ...` (one context, shared launches) prints per file exactly what `dafs A`, `dafs B`, ... print: two Rfam
    sets, a synthetic family, unrelated sequences and a single sequence, with and without refinement"""
    files = [os.path.join(G, "RF00005_0.fa"), os.path.join(G, "RF00017_4.fa")]
    for k, recs in enumerate((synth.family_set(5, 80, seed=71), synth.random_set(4, 60, seed=72), synth.random_set(1, 50, seed=74),
                              synth.family_set(8, 120, seed=73))):
        p = tmp_path / ("in%d.fa" % k)
        p.write_text(synth.to_fasta(recs))
        files.append(str(p))
    for opts in ([], ["-r", "2"]):
        want = ""
        for f in files:
            rc, out, err = _run_cli(*opts, f)
            assert rc == 0, err
            want += "==> %s <==\n" % f + out
        rc, out, err = _run_cli(*(opts + files))
        assert rc == 0, err
        assert out == want, opts
    rc, out, err = _run_cli(files[0], str(tmp_path / "missing.fa"))
    assert rc == 1 and "missing.fa" in err and out == ""


def test_cli_several_files_row_structures(tmp_path):
    """`dafs --stockholm OUT --row-structures A B C`: one block per file with a #=GR SS line per row, each the Python driver's; a
    file of one sequence among them"""
    from dafs_amd import pipeline
    fams = [_split(synth.family_set(4, 50, seed=91)), _split(synth.random_set(3, 40, seed=92)), _split(synth.random_set(1, 30, seed=93))]
    files = []
    for k, (names, seqs) in enumerate(fams):
        p = tmp_path / ("rs%d.fa" % k)
        p.write_text(synth.to_fasta(list(zip(names, seqs))))
        files.append(str(p))
    sto = str(tmp_path / "out.sto")
    rc, out, err = _run_cli("--stockholm", sto, "--row-structures", *files)
    assert rc == 0, err
    ctx = _ctx()
    try:
        want = pipeline.run_batch(fams, ctx=ctx, reliability=True, row_structures=True)
    finally:
        ctx.close()
    assert out == "".join("==> %s <==\n" % f + r.output for f, r in zip(files, want))
    assert open(sto).read() == "".join(r.stockholm for r in want)
    assert sum(1 for ln in open(sto).read().split("\n") if ln.startswith("#=GR ") and ln.split()[2] == "SS") == 8


def test_errors_leave_the_context_usable():
    from dafs_amd import capi, pipeline
    good = [_split(synth.family_set(4, 60, seed=81)), _split(synth.random_set(3, 50, seed=82))]
    bad = [good[0], (["a", "b"], ["ACGU" * 20, "ACGU" * 513])]  # 2052 nt: beyond the pair kernels' columns
    ctx = _ctx()
    try:
        with pytest.raises(capi.DafsHipError) as e:
            pipeline.run_batch(bad, ctx=ctx)
        assert "code -4" in str(e.value)
        got = pipeline.run_batch(good, ctx=ctx)
        for (names, seqs), r in zip(good, got):
            assert r.output == pipeline.run(names, seqs, ctx=ctx).output
        # a node whose rows come from two families is refused
        seqs = good[0][1] + good[1][1]
        pipeline._phase1_local(ctx, seqs, None, None, capi.ALIGN_PROBCONS, 0.01, 0.25, 0.25, [], 0.0, [0, 4, 7])
        one = lambda i: (np.array([i], np.uint32), np.ones((1, len(seqs[i])), np.uint8))
        with pytest.raises(capi.DafsHipError) as e:
            ctx.nodes_open([one(0) + one(5)], capi.dd_params())
        assert "code -1" in str(e.value)
        h, _ = ctx.nodes_open([one(0) + one(1)], capi.dd_params())  # within a family: accepted
        assert len(h) == 1
        ctx.nodes_close()
    finally:
        ctx.close()


def test_many_small_families():
    from dafs_amd import pipeline
    fams = [_split(synth.family_set(8, 100, seed=1000 + k)) for k in range(256)]
    ctx = _ctx()
    try:
        got = pipeline.run_batch(fams, ctx=ctx)
        assert len(got) == 256 and all(r.output for r in got)
        for k in range(0, 256, 32):
            one = pipeline.run(*fams[k], ctx=ctx)
            assert got[k].output == one.output and got[k].dd_log == one.dd_log
    finally:
        ctx.close()
