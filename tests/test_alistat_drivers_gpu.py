"""GPU tests of the drivers of the alignment statistics: pipeline.run / run_batch / add with identity,
pipeline.add_each with nearest and nr, pipeline.describe, and the command line's --identity, --identity-matrix, --seed-nearest,
--seed-nr and --describe against them.  The numbers are checked against tests/alistat_ref.py, bit for bit."""
import functools
import os
import subprocess

import numpy as np
import pytest

import alistat_ref as ar
from dafs_amd import capi, pipeline, stockholm, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
NONE = ar.NONE


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _split(recs):
    return [r[0] for r in recs], [r[1] for r in recs]


def _cli(*args, ok=True):
    r = subprocess.run([DAFS] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert (r.returncode == 0) == ok, r.stderr
    return r.stdout if ok else r.stderr


def _check_identity(idn, rows, use=None):
    cell = ar.cells(rows)
    res, ident, aligned = ar.counts(cell, use)
    near, ni, nd = ar.nearest(res, ident)
    assert idn.res.tolist() == res and idn.ident.tolist() == ident and idn.aligned.tolist() == aligned
    assert idn.nearest.tolist() == near and idn.nearest_ident.tolist() == ni and idn.nearest_den.tolist() == nd
    assert np.asarray(idn.weights).tobytes() == np.array(ar.weights(cell, use), np.float64).tobytes()
    assert idn.pid.tolist() == [float(i) / float(d) for i, d in zip(ni, nd)]
    assert np.array(idn.summary).tobytes() == np.array(ar.summary(res, ident)).tobytes()


def _without_wt(block):
    return "".join(ln + "\n" for ln in block.split("\n")[:-1] if not ln.startswith("#=GS "))


def test_run_with_identity(ctx):
    names, seqs = _split(synth.family_set(6, 60))
    plain = pipeline.run(names, seqs, ctx=ctx, reliability=True)
    res = pipeline.run(names, seqs, ctx=ctx, reliability=True, identity=True)
    assert res.output == plain.output and not hasattr(plain, "identity")
    _check_identity(res.identity, res.rows)
    # the block gains the WT lines directly after the #=GF line and nothing else
    lines = res.stockholm.split("\n")
    assert lines[1].startswith("#=GF CC ") and all(ln.startswith("#=GS ") for ln in lines[2:8]) and not lines[8].startswith("#")
    assert lines[2:8] == ["#=GS %s WT %.6f" % (nm, w) for nm, w in zip(res.row_names, res.identity.weights)]
    assert _without_wt(res.stockholm) == plain.stockholm
    assert pipeline.run(names, seqs, ctx=ctx, identity=True).output == plain.output
    # a batch and an added sequence: a direct call on the printed rows
    fams = [(names, seqs), _split(synth.random_set(1, 30, seed=5)), _split(synth.family_set(3, 40, seed=6))]
    got = pipeline.run_batch(fams, ctx=ctx, identity=True)
    assert pipeline.identity_tsv(got[0].row_names, got[0].identity) == pipeline.identity_tsv(res.row_names, res.identity)
    assert got[1].identity.nearest.tolist() == [NONE] and got[1].identity.weights.tolist() == [1.0] and np.isnan(got[1].identity.summary).all()
    _check_identity(got[2].identity, got[2].rows)
    seed = pipeline.run(names[:4], seqs[:4], ctx=ctx)
    added = pipeline.add(names[:4], seed.rows, names[4:], seqs[4:], ctx=ctx, identity=True)
    assert added.output == pipeline.add(names[:4], seed.rows, names[4:], seqs[4:], ctx=ctx).output
    _check_identity(added.identity, added.rows)
    with pytest.raises(ValueError):
        pipeline.pairwise(names, seqs, ctx=ctx, identity=True)


def _comp(s):
    return "".join({"A": "U", "U": "A", "G": "C", "C": "G"}[ch] for ch in reversed(s))


def _row(stem1, stem2):
    return "AU" + stem1 + "AAUCAAUA" + _comp(stem1) + "AUACAUA" + stem2 + "UUAACUUAAC" + _comp(stem2) + "AUAUCAUACAUAU"


STRUCTURE = ".." + "(((((" + "........" + ")))))" + "......." + "<<<<<" + ".........." + ">>>>>" + "............."
SEED_NAMES = ["s0", "s1", "s2", "s3"]


@functools.lru_cache(maxsize=None)
def _seed():
    """a 4-row seed and 6 hits, two of them exact copies of seed row 2 (and so of one another)"""
    rows = [_row("GGCGC", "CCGGA"), _row("GCCGC", "CGGCA"), _row("GGCGU", "CCGGA"), _row("GGUGC", "CUGGA")]
    rows[1] = rows[1][:22] + "-" + rows[1][23:]
    names, rows, ss = stockholm.clean_seed_structure(SEED_NAMES, rows, STRUCTURE)
    base = _row("GGCGC", "CUGGA")
    far = list(_row("GCGCG", "GGCCU"))
    for c in range(1, 60, 4):  # the stems of another family and every fourth residue changed
        far[c] = {"A": "C", "C": "A", "G": "U", "U": "G"}[far[c]]
    new_names = ["h0", "copy1", "h2", "copy3", "h4", "h5"]
    new_seqs = ["GACC" + base, rows[2], base[:9] + "GGG" + base[9:36] + base[39:], rows[2], "".join(far),
                synth.random_set(1, 50, seed=953, jitter=0.0)[0][1]]
    return rows, ss, new_names, new_seqs


@pytest.fixture(scope="module")
def each(ctx):
    rows, ss, names, seqs = _seed()
    return pipeline.add_each(SEED_NAMES, rows, names, seqs, ctx=ctx, seed_ss=ss, nearest=True, merged=True, nr=0.9)


def test_add_each_nearest_and_nr(ctx, each, tmp_path):
    rows, ss, names, seqs = _seed()
    m, k = len(rows), len(seqs)
    plain = pipeline.add_each(SEED_NAMES, rows, names, seqs, ctx=ctx, seed_ss=ss, merged=True)
    assert not hasattr(plain, "nearest") and not hasattr(plain.merged, "kept")
    for a, b in zip(each.results, plain.results):
        assert a.output == b.output and a.rows == b.rows and a.rf.tobytes() == b.rf.tobytes()
    mg = each.merged
    assert mg.stockholm == plain.merged.stockholm and mg.rows == plain.merged.rows and mg.names == plain.merged.names
    # the nearest seed row of every hit, in the columns of its own result
    for j, r in enumerate(each.results):
        cell = ar.cells(r.rows)
        res, ident, _ = ar.counts(cell, r.rf.tolist())
        near, ni, nd = ar.nearest(res, ident, [True] * m + [False])
        assert (each.nearest.row[j], each.nearest.ident[j], each.nearest.den[j]) == (near[m], ni[m], nd[m])
        assert each.nearest.pid[j] == float(ni[m]) / float(nd[m])
    assert each.nearest.row[1] == each.nearest.row[3] == 2 and each.nearest.pid[1] == each.nearest.pid[3] == 1.0
    # the table: two more columns, and without the option the bytes of before
    table = pipeline.seed_scores_tsv(names, each)
    old = pipeline.seed_scores_tsv(names, plain)
    assert [ln.split("\t")[:-2] for ln in table.splitlines()] == [ln.split("\t") for ln in old.splitlines()]
    assert [ln.split("\t")[-2:] for ln in table.splitlines()] == [["s%d" % each.nearest.row[j], "%.9g" % each.nearest.pid[j]] for j in range(k)]
    # the subset: the copies fall to a seed row; the walk is the restatement's
    res, ident, _ = ar.counts(ar.cells(mg.rows), mg.rf.tolist())
    order = list(range(m)) + [m + int(j) for j in np.argsort(-each.score.astype(np.float64), kind="stable")]
    kept, by = ar.nr_select(ar.red_matrix(res, ident, 0.9), order, [True] * m + [False] * k)
    assert mg.kept.tolist() == kept and mg.by.tolist() == by
    assert not mg.kept[m + 1] and not mg.kept[m + 3] and mg.by[m + 1] < m and mg.by[m + 3] < m and mg.kept[:m].all() and mg.kept[m + 5]  # by: a seed row
    assert mg.nr_rows == [r for r, keep in zip(mg.rows, kept) if keep] and mg.nr_names == [n for n, keep in zip(mg.names, kept) if keep]
    # the block: the merged block without the dropped rows' lines, one comment line more; a seed again
    lines = mg.nr_stockholm.split("\n")
    assert lines[1] == "#=GF CC nr 0.9 kept %d of %d hits" % (sum(kept[m:]), k)
    dropped = [n for n, keep in zip(mg.names, kept) if not keep]
    want = [ln for ln in mg.stockholm.split("\n") if not any(ln.startswith(d + " ") or ln.startswith("#=GR " + d + " ") for d in dropped)]
    assert lines[:1] + lines[2:] == want
    got = stockholm.parse_seed_structure(mg.nr_stockholm)
    assert got[0] == mg.nr_names and got[1] == mg.nr_rows and got[2] == mg.ss_str
    # read back as a seed: the all-gap columns go, the seed's columns are all there with the seed's rows and structure
    (tmp_path / "nr.sto").write_text(mg.nr_stockholm)
    back = stockholm.read_seed_structure(str(tmp_path / "nr.sto"))
    keep = [c for c in range(len(mg.rf)) if any(r[c] != "-" for r in mg.nr_rows)]
    assert back[0] == mg.nr_names and back[1] == ["".join(r[c] for c in keep) for r in mg.nr_rows]
    rf_back = [bool(mg.rf[c]) for c in keep]
    assert sum(rf_back) == len(rows[0])  # no seed column was lost
    assert ["".join(ch for ch, x in zip(r, rf_back) if x) for r in back[1][:m]] == list(rows)
    assert "".join(ch for ch, x in zip(capi.make_brackets(back[2]), rf_back) if x) == capi.make_brackets(ss)
    assert all(ch == "." for ch, x in zip(capi.make_brackets(back[2]), rf_back) if not x)
    with pytest.raises(ValueError):
        pipeline.add_each(SEED_NAMES, rows, names, seqs, ctx=ctx, seed_ss=ss, nr=0.9)
    with pytest.raises(ValueError):
        pipeline.add_each(SEED_NAMES, rows, names, seqs, ctx=ctx, seed_ss=ss, merged=True, nr=0.0)


def test_cli_seed_nearest_and_nr(each, tmp_path):
    rows, ss, names, seqs = _seed()
    seed, new_fa, out, tsv = tmp_path / "seed.sto", tmp_path / "new.fa", tmp_path / "nr.sto", tmp_path / "hits.tsv"
    seed.write_text("# STOCKHOLM 1.0\n" + "".join("%s %s\n" % (n, r) for n, r in zip(SEED_NAMES, rows)) + "#=GC SS_cons %s\n//\n" % STRUCTURE)
    new_fa.write_text(synth.to_fasta(list(zip(names, seqs))))
    want_out = "".join("==> %d <==\n" % (j + 1) + r.output for j, r in enumerate(each.results))
    got = _cli("--seed", seed, "--seed-structure", "--seed-each", "--seed-scores", tsv, "--seed-nearest", "--seed-merged", out, "--seed-nr", "0.9", new_fa)
    assert got == want_out
    assert tsv.read_text() == pipeline.seed_scores_tsv(names, each) and out.read_text() == each.merged.nr_stockholm


def test_cli_identity(ctx, tmp_path):
    recs, recs2 = synth.family_set(6, 60), synth.family_set(4, 50, seed=77)
    fa, fa2 = tmp_path / "a.fa", tmp_path / "b.fa"
    fa.write_text(synth.to_fasta(recs))
    fa2.write_text(synth.to_fasta(recs2))
    tsv, mat, sto = tmp_path / "id.tsv", tmp_path / "id.mat", tmp_path / "a.sto"
    plain = _cli(fa)
    assert _cli("--identity", tsv, "--identity-matrix", mat, "--stockholm", sto, fa) == plain  # stdout never changes
    res = pipeline.run(*_split(recs), ctx=ctx, reliability=True, identity=True)
    assert res.output == plain
    assert tsv.read_text() == pipeline.identity_tsv(res.row_names, res.identity)
    assert mat.read_text() == pipeline.identity_matrix_tsv(res.row_names, res.identity) and sto.read_text() == res.stockholm
    head = tsv.read_text().split("\n")[0].split(" ")
    assert head[:5] == ["#", "rows", "6", "columns", str(len(res.rows[0]))] and head[5::2] == ["average", "min", "max"]
    assert [float(x) for x in head[6::2]] == [float("%.9g" % x) for x in res.identity.summary]
    # two files: a block per file under its header line; without --stockholm the tables alone
    res2 = pipeline.run(*_split(recs2), ctx=ctx, identity=True)
    both = _cli("--identity", tsv, "--identity-matrix", mat, fa, fa2)
    assert both == "==> %s <==\n%s==> %s <==\n%s" % (fa, plain, fa2, res2.output)
    assert tsv.read_text() == "==> %s <==\n%s==> %s <==\n%s" % (fa, pipeline.identity_tsv(res.row_names, res.identity), fa2,
                                                              pipeline.identity_tsv(res2.row_names, res2.identity))
    assert mat.read_text() == "==> %s <==\n%s==> %s <==\n%s" % (fa, pipeline.identity_matrix_tsv(res.row_names, res.identity), fa2,
                                                              pipeline.identity_matrix_tsv(res2.row_names, res2.identity))
    # --seed: the added sequences and the seed rows, in printed order
    names, seqs = _split(recs)
    seed_aln = tmp_path / "seed.aln"
    seed_aln.write_text(pipeline.run(names[:4], seqs[:4], ctx=ctx).output)
    new_fa = tmp_path / "new.fa"
    new_fa.write_text(synth.to_fasta(recs[4:]))
    snames, srows = stockholm.read_seed(str(seed_aln))
    added = pipeline.add(snames, srows, names[4:], seqs[4:], ctx=ctx, identity=True)
    assert _cli("--seed", seed_aln, "--identity", tsv, new_fa) == added.output
    assert tsv.read_text() == pipeline.identity_tsv(added.row_names, added.identity)


@pytest.mark.parametrize("form", ["stockholm", "fasta"])
def test_cli_describe(ctx, tmp_path, form):
    names, seqs = _split(synth.family_set(6, 60))
    res = pipeline.run(names, seqs, ctx=ctx, reliability=True)
    aln = tmp_path / "aln"
    aln.write_text(res.stockholm if form == "stockholm" else res.output)
    tsv, mat, cov = tmp_path / "id.tsv", tmp_path / "id.mat", tmp_path / "cov.tsv"
    assert _cli("--describe", aln, "--identity", tsv, "--identity-matrix", mat, "--covariation", cov, "--cov-shuffles", "20") == ""
    got = stockholm.read_seed_structure(str(aln))
    d = pipeline.describe(*got, ctx=ctx, covariation=dict(shuffles=20))
    assert d.rows == got[1] and d.ss.tobytes() == got[2].tobytes()
    _check_identity(d.identity, d.rows)
    assert tsv.read_text() == pipeline.identity_tsv(d.row_names, d.identity) and mat.read_text() == pipeline.identity_matrix_tsv(d.row_names, d.identity)
    assert cov.read_text() == pipeline.covariation_tsv(d)
    # the alignment the run printed: the same rows, so the same numbers as the run's own annotation
    with_id = pipeline.run(names, seqs, ctx=ctx, identity=True)
    keep = [c for c in range(len(with_id.rows[0])) if any(r[c] != "-" for r in with_id.rows)]
    assert d.rows == ["".join(r[c] for c in keep) for r in with_id.rows]
    assert d.identity.ident.tobytes() == with_id.identity.ident.tobytes() and d.identity.weights.tobytes() == with_id.identity.weights.tobytes()
