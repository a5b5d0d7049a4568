"""GPU tests of adding each new sequence to a seed on its own (pipeline.add_each, `dafs --seed SEED --seed-each`; DESIGN.md
section 15).  The contract: result j is, bit for bit, pipeline.add of that one sequence -- so the order of the new sequences,
which others are present, the chunking and the form of the matching transform do not matter."""
import functools
import os
import subprocess

import numpy as np
import pytest

from dafs_amd import capi, pipeline, stockholm, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")


@functools.lru_cache(maxsize=None)
def _inputs():
    """a seed of 4 members of a 9-member family aligned by a run; the new sequences: the 5 other members, an unrelated
    sequence of 30 nt and one of 9 nt"""
    recs = synth.family_set(9, 60, seed=601)
    names, seqs = [n for n, _ in recs], [s for _, s in recs]
    res = pipeline.run(names[:4], seqs[:4])
    rows = res.rows
    keep = [c for c in range(len(rows[0])) if any(r[c] != "-" for r in rows)]
    srows = ["".join(r[c] for c in keep) for r in rows]
    new_names = names[4:] + ["unrelated", "short"]
    new_seqs = seqs[4:] + [synth.random_set(1, 30, seed=602, jitter=0.0)[0][1], synth.random_set(1, 9, seed=603, jitter=0.0)[0][1]]
    assert [len(s) for s in new_seqs[5:]] == [30, 9]
    return names[:4], srows, new_names, new_seqs, res.output


def _log(r):
    return {k: (v[0], v[1], v[2], np.float32(v[3]).tobytes()) for k, v in r.dd_log.items()}


def _same(got, want, kw=()):
    assert got.output == want.output
    assert [z.tobytes() for z in got.z] == [z.tobytes() for z in want.z]
    assert got.rf.tobytes() == want.rf.tobytes()
    assert _log(got) == _log(want)
    assert got.ss.tobytes() == want.ss.tobytes()
    assert got.rows == want.rows and got.ss_str == want.ss_str
    if "reliability" in kw:
        assert got.stockholm == want.stockholm
        for key in ("col", "pair", "pair_rows"):
            assert got.reliability[key].tobytes() == want.reliability[key].tobytes()
        assert [a.tobytes() for a in got.reliability["residue"]] == [a.tobytes() for a in want.reliability["residue"]]
        assert got.reliability["expected_accuracy"] == want.reliability["expected_accuracy"]
    if "row_structures" in kw:
        assert [a.tobytes() for a in got.row_ss] == [a.tobytes() for a in want.row_ss] and got.row_ss_str == want.row_ss_str


@functools.lru_cache(maxsize=None)
def _plain():
    snames, srows, names, seqs, _ = _inputs()
    return pipeline.add_each(snames, srows, names, seqs)


@pytest.mark.parametrize("kw", [{}, dict(reliability=True), dict(w_pct_f=0.5), dict(bp_update1=True), dict(align_model=capi.ALIGN_CONTRALIGN),
                                dict(row_structures=True, reliability=True), dict(row_structures=True)],
                         ids=["default", "reliability", "fourway", "bp_update1", "contralign", "row_structures_sto", "row_structures"])
def test_each_result_equals_add_of_that_sequence(kw):
    snames, srows, names, seqs, _ = _inputs()
    ctx = capi.Context(0)
    each = pipeline.add_each(snames, srows, names, seqs, ctx=ctx, **kw) if kw else _plain()
    assert len(each.results) == len(seqs) and [k for c in each.chunks for k in c] == list(range(len(seqs)))
    for j, got in enumerate(each.results):
        want = pipeline.add(snames, srows, [names[j]], [seqs[j]], ctx=ctx, **kw)
        _same(got, want, kw)
        assert each.score[j].tobytes() == np.float32(want.dd_log[0][3]).tobytes() and each.iterations[j] == want.dd_log[0][0]
        assert each.matched[j] == int((want.z[0] != pipeline.NONE).sum()) and each.lengths[j] == len(seqs[j])
        assert each.matched[j] == sum(1 for c, ch in enumerate(got.rows[-1]) if ch != "-" and got.rf[c])
    assert set(each.seconds) == {"phase1", "gather", "transforms", "nodes", "final", "total"}
    ctx.close()


def test_one_row_seed():
    snames, srows, names, seqs, _ = _inputs()
    snames, srows = snames[:1], [srows[0].replace("-", "")]
    ctx = capi.Context(0)
    each = pipeline.add_each(snames, srows, names[3:], seqs[3:], ctx=ctx, reliability=True)
    for j, got in enumerate(each.results):
        _same(got, pipeline.add(snames, srows, [names[3 + j]], [seqs[3 + j]], ctx=ctx, reliability=True), ("reliability",))
    ctx.close()


def test_full_and_listed_transform_agree():
    """with reliability the full matching transform runs, without it the listed one: the results minus the reliability fields
    are the same"""
    snames, srows, names, seqs, _ = _inputs()
    full = pipeline.add_each(snames, srows, names, seqs, reliability=True)
    for a, b in zip(full.results, _plain().results):
        _same(a, b)
        assert hasattr(a, "stockholm") and not hasattr(b, "stockholm")
    assert full.score.tobytes() == _plain().score.tobytes() and np.array_equal(full.iterations, _plain().iterations)


def test_order_and_company_do_not_matter():
    snames, srows, names, seqs, _ = _inputs()
    base = _plain()
    rev = pipeline.add_each(snames, srows, names[::-1], seqs[::-1])
    for a, b in zip(rev.results, base.results[::-1]):
        _same(a, b)
    assert rev.score.tobytes() == base.score[::-1].tobytes()
    pick = [5, 1, 6]
    sub = pipeline.add_each(snames, srows, [names[j] for j in pick], [seqs[j] for j in pick])
    for a, j in zip(sub.results, pick):
        _same(a, base.results[j])
    assert np.array_equal(sub.matched, base.matched[pick])


def test_chunks_give_the_same_results():
    snames, srows, names, seqs, _ = _inputs()
    base = _plain()
    seed_lens = [len(r.replace("-", "")) for r in srows]
    sizes = [pipeline.seed_each_bytes(seed_lens, len(srows[0]), len(s)) for s in seqs]
    parts = pipeline.add_each(snames, srows, names, seqs, max_bytes=sizes[0] + sizes[1])
    assert len(base.chunks) == 1 and len(parts.chunks) >= 3 and len(parts.dd_memory) == len(parts.chunks)
    assert [k for c in parts.chunks for k in c] == list(range(len(seqs)))
    for a, b in zip(parts.results, base.results):
        _same(a, b)
    assert parts.score.tobytes() == base.score.tobytes() and np.array_equal(parts.matched, base.matched)
    alone = pipeline.add_each(snames, srows, names[:3], seqs[:3], max_bytes=1)  # every sequence over the budget: each alone
    assert alone.chunks == [[0], [1], [2]]
    for a, b in zip(alone.results, base.results):
        _same(a, b)


def _cli(*args):
    r = subprocess.run([DAFS] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout


def _write_sto(path, names, rows, block=30):
    """an interleaved Stockholm file with '.' gaps and annotation lines"""
    w = max(len(n) for n in names) + 2
    lines = ["# STOCKHOLM 1.0", "#=GF ID seed"]
    for b in range(0, len(rows[0]), block):
        lines.append("")
        for n, r in zip(names, rows):
            lines.append(n.ljust(w) + r[b:b + block].replace("-", "."))
    lines.append("//")
    path.write_text("\n".join(lines) + "\n")


def test_cli_equals_python_and_single_sequence_files(tmp_path):
    snames, srows, names, seqs, seed_output = _inputs()
    pick = [0, 5, 6, 0]  # a family member, the unrelated one, the 9-nt one, and the first again under its repeated name
    names, seqs = [names[j] for j in pick], [seqs[j] for j in pick]
    new_fa = tmp_path / "new.fa"
    new_fa.write_text(synth.to_fasta(list(zip(names, seqs))))
    seed_aln, seed_sto = tmp_path / "seed.aln", tmp_path / "seed.sto"
    seed_aln.write_text(seed_output)  # aligned FASTA as dafs prints it, tree line and SS_cons included
    _write_sto(seed_sto, snames, srows)
    assert stockholm.read_seed(str(seed_aln)) == stockholm.read_seed(str(seed_sto)) == (snames, srows)
    want = pipeline.add_each(snames, srows, names, seqs, reliability=True)
    want_out = "".join("==> %d <==\n" % (j + 1) + r.output for j, r in enumerate(want.results))
    want_tsv = pipeline.seed_scores_tsv(names, want)
    assert [ln.split("\t")[1] for ln in want_tsv.splitlines()] == stockholm.names(names) and stockholm.names(names)[3].endswith(".2")
    for seed in (seed_sto, seed_aln):
        sto, tsv = tmp_path / "out.sto", tmp_path / "out.tsv"
        assert _cli("--seed", seed, "--seed-each", "--stockholm", sto, "--seed-scores", tsv, new_fa) == want_out
        assert sto.read_text() == "".join(r.stockholm for r in want.results)
        assert sto.read_text().count("#=GC RF") == len(names)
        assert tsv.read_text() == want_tsv
    # without --stockholm the listed transform runs: the same stdout and table
    tsv = tmp_path / "plain.tsv"
    out = _cli("--seed", seed_sto, "--seed-each", "--seed-scores", tsv, new_fa)
    assert out == want_out and tsv.read_text() == want_tsv
    blocks = out.split("==> ")[1:]
    for j in range(3):
        one = tmp_path / ("one_%d.fa" % j)
        one.write_text(synth.to_fasta([(names[j], seqs[j])]))
        assert blocks[j] == "%d <==\n" % (j + 1) + _cli("--seed", seed_sto, one)


def test_cli_covariation_and_row_structures_equal_python(tmp_path):
    """--seed-each with --covariation and --stockholm --row-structures: per new sequence a table under its "==> j <==" line and a
    block with the #=GR SS lines and the cov_SS_cons line, all the Python driver's"""
    snames, srows, names, seqs, _ = _inputs()
    pick = [0, 5, 6]  # a family member, the unrelated one, the 9-nt one
    names, seqs = [names[j] for j in pick], [seqs[j] for j in pick]
    new_fa, seed_sto = tmp_path / "new.fa", tmp_path / "seed.sto"
    new_fa.write_text(synth.to_fasta(list(zip(names, seqs))))
    _write_sto(seed_sto, snames, srows)
    want = pipeline.add_each(snames, srows, names, seqs, reliability=True, row_structures=True, covariation=dict(shuffles=20, seed=5))
    sto, cov = tmp_path / "out.sto", tmp_path / "cov.tsv"
    out = _cli("--seed", seed_sto, "--seed-each", "--stockholm", sto, "--row-structures", "--covariation", cov, "--cov-shuffles", 20,
               "--cov-seed", 5, new_fa)
    heads = ["==> %d <==\n" % (j + 1) for j in range(len(names))]
    assert out == "".join(h + r.output for h, r in zip(heads, want.results))
    assert sto.read_text() == "".join(r.stockholm for r in want.results)
    lines = sto.read_text().split("\n")
    assert sum(1 for ln in lines if ln.startswith("#=GR ") and ln.split()[2] == "SS") == len(names) * (len(snames) + 1)
    assert sum(1 for ln in lines if ln.startswith("#=GC cov_SS_cons")) == len(names)
    assert cov.read_text() == "".join(h + pipeline.covariation_tsv(r) for h, r in zip(heads, want.results))
