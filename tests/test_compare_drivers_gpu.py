"""GPU tests of the drivers of the alignment comparison: pipeline.run / add / describe / add_each with
compare=, and the command line's --compare, --compare-columns and --compare-matrix against them, byte for byte.  The numbers
are checked against tests/compare_ref.py."""
import os
import subprocess

import numpy as np
import pytest

import compare_ref as cr
from dafs_amd import capi, pipeline, stockholm, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
G = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _split(recs):
    return [r[0] for r in recs], [r[1] for r in recs]


def _fasta(path):
    names, seqs = [], []
    with open(path) as fh:
        for line in fh:
            line = line.rstrip("\n")
            if line.startswith(">"):
                names.append(line[1:].strip())
                seqs.append("")
            elif line:
                seqs[-1] += line.strip()
    return names, seqs


def _cli(*args):
    r = subprocess.run([DAFS] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout


def _check(cmp, ref, row_names, rows, ss, use_test=None):
    """a driver's .compare against the restatement on the rows it names"""
    ref_names = [n.split()[0] for n in ref[0]]
    common = [n for n in ref_names if n in row_names]
    assert cmp.row_names == common and len(common) >= 2
    cell_r = cr.cells([ref[1][ref_names.index(n)] for n in common])
    cell_t = cr.cells([rows[row_names.index(n)] for n in common])
    both = len(ref) == 3 and ref[2] is not None and ss is not None
    want = cr.compare(cell_r, cell_t, None, use_test, ref[2].tolist() if both else None, ss.tolist() if both else None)
    for k in ("shared", "refp", "testp", "k", "colshared") + (("tp", "nref", "ntest") if both else ()):
        assert [int(x) for x in getattr(cmp, k)] == want[k], k
    for k in ("sps", "ppv", "tc"):
        assert np.array(getattr(cmp, k)).tobytes() == np.array(want[k]).tobytes(), k
    mats = cr.pair_counts(cr.keys(cell_r, cell_t, None, use_test))
    assert cmp.pair_shared.tolist() == mats[0] and cmp.pair_refp.tolist() == mats[1] and cmp.pair_testp.tolist() == mats[2]
    assert cmp.columns_table == cr.columns_table(want) and cmp.matrix_table == cr.matrix_table(common, *mats)
    return want


@pytest.mark.parametrize("family", ["RF00005_0", "synth"])
def test_run_against_its_refined_self(ctx, tmp_path, family):
    if family == "synth":
        names, seqs = _split(synth.family_set(6, 60))
        fa = tmp_path / "in.fa"
        fa.write_text(synth.to_fasta(list(zip(names, seqs))))
    else:
        fa = os.path.join(G, family + ".fa")
        names, seqs = _fasta(fa)
    ref_file, tsv, cols, mat, sto, sto2 = (tmp_path / n for n in ("ref.aln", "cmp.tsv", "cmp.cols", "cmp.mat", "a.sto", "b.sto"))
    ref_file.write_text(_cli("-r", "1", fa))
    ref = stockholm.read_seed_structure(str(ref_file))
    plain = _cli("--stockholm", sto, fa)
    # stdout and the Stockholm file are the same bytes with and without the option
    assert _cli("--compare", tsv, "--compare-ref", ref_file, "--compare-columns", cols, "--compare-matrix", mat, "--stockholm", sto2, fa) == plain
    assert sto2.read_text() == sto.read_text()
    res = pipeline.run(names, seqs, ctx=ctx, reliability=True, compare=ref)
    assert res.output == plain and res.stockholm == sto.read_text()
    assert tsv.read_text() == res.compare.table and cols.read_text() == res.compare.columns_table and mat.read_text() == res.compare.matrix_table
    want = _check(res.compare, ref, res.row_names, res.rows, res.ss)
    assert res.compare.table == cr.table(res.compare.row_names, 0, 0, want)
    assert res.compare.table.split("\n")[3].startswith("# structure tp ")
    # a run compared with its own output scores 1
    own = tmp_path / "own.aln"
    own.write_text(plain)
    assert _cli("--compare", tsv, "--compare-ref", own, fa) == plain
    me = pipeline.run(names, seqs, ctx=ctx, compare=stockholm.read_seed_structure(str(own))).compare
    assert tsv.read_text() == me.table
    assert me.sps == 1.0 and me.ppv == 1.0 and me.tc == 1.0 and me.sensitivity == 1.0 and me.ss_ppv == 1.0 and me.f == 1.0
    assert me.tp.tolist() == me.nref.tolist() == me.ntest.tolist()
    if family == "synth":  # two files follow the ==> FILE <== convention; the reference lacks the second file's names
        two = _cli("--compare", tsv, "--compare-ref", ref_file, fa, fa)
        assert two == "==> %s <==\n%s==> %s <==\n%s" % (fa, plain, fa, plain)
        assert tsv.read_text() == ("==> %s <==\n%s" % (fa, res.compare.table)) * 2


def test_describe_seed_and_merged(ctx, tmp_path):
    names, seqs = _split(synth.family_set(6, 60))
    res = pipeline.run(names, seqs, ctx=ctx, reliability=True)
    refined = tmp_path / "ref.aln"
    fa = tmp_path / "in.fa"
    fa.write_text(synth.to_fasta(list(zip(names, seqs))))
    refined.write_text(_cli("-r", "1", fa))
    ref = stockholm.read_seed_structure(str(refined))
    tsv, cols, mat = tmp_path / "cmp.tsv", tmp_path / "cmp.cols", tmp_path / "cmp.mat"
    # --describe of the Stockholm block: its PP lines give the PP part, and --compare* alone is enough
    aln = tmp_path / "a.sto"
    aln.write_text(res.stockholm)
    assert _cli("--describe", aln, "--compare", tsv, "--compare-ref", refined, "--compare-columns", cols, "--compare-matrix", mat) == ""
    got = stockholm.read_seed_structure(str(aln))
    pp = stockholm.read_seed_pp(str(aln))
    assert pp is not None
    d = pipeline.describe(*got, ctx=ctx, identity=False, compare=ref, pp=pp)
    assert tsv.read_text() == d.compare.table and cols.read_text() == d.compare.columns_table and mat.read_text() == d.compare.matrix_table
    assert "# pp " in d.compare.table and int(d.compare.pp_residues.sum()) == sum(len(s) for s in seqs)
    _check(d.compare, ref, d.row_names, d.rows, d.ss)
    # the aligned FASTA the run printed: no PP part, the same pair counts
    plain_aln = tmp_path / "a.aln"
    plain_aln.write_text(res.output)
    assert _cli("--describe", plain_aln, "--compare", tsv, "--compare-ref", refined) == ""
    d2 = pipeline.describe(*stockholm.read_seed_structure(str(plain_aln)), ctx=ctx, identity=False, compare=ref)
    assert tsv.read_text() == d2.compare.table and "# pp " not in d2.compare.table
    assert d2.compare.shared.tolist() == d.compare.shared.tolist()
    # --seed: four rows as the seed, two added, against the refined run of all six
    seed_aln, new_fa = tmp_path / "seed.aln", tmp_path / "new.fa"
    seed_aln.write_text(pipeline.run(names[:4], seqs[:4], ctx=ctx).output)
    new_fa.write_text(synth.to_fasta(list(zip(names[4:], seqs[4:]))))
    snames, srows = stockholm.read_seed(str(seed_aln))
    plain_add = pipeline.add(snames, srows, names[4:], seqs[4:], ctx=ctx)
    added = pipeline.add(snames, srows, names[4:], seqs[4:], ctx=ctx, compare=ref)
    assert added.output == plain_add.output
    assert _cli("--seed", seed_aln, "--compare", tsv, "--compare-ref", refined, "--compare-matrix", mat, new_fa) == added.output
    assert tsv.read_text() == added.compare.table and mat.read_text() == added.compare.matrix_table
    _check(added.compare, ref, added.row_names, added.rows, added.ss)
    # --seed-each --seed-merged: the merged alignment in the seed's columns, with the PP classes of its own block
    sn, sr, sss = stockholm.read_seed_structure(str(seed_aln))
    seed_sto = tmp_path / "seed.sto"
    seed_sto.write_text("# STOCKHOLM 1.0\n" + "".join("%s %s\n" % (n.split()[0], r) for n, r in zip(sn, sr)) + "#=GC SS_cons %s\n//\n" % capi.make_brackets(sss))
    sn, sr, sss = stockholm.read_seed_structure(str(seed_sto))
    merged_file, merged_plain = tmp_path / "m.sto", tmp_path / "m0.sto"
    each = pipeline.add_each(sn, sr, names[4:], seqs[4:], ctx=ctx, seed_ss=sss, merged=True, compare=ref)
    out = _cli("--seed", seed_sto, "--seed-structure", "--seed-each", "--seed-merged", merged_file, "--compare", tsv, "--compare-ref", refined,
               "--compare-columns", cols, "--compare-matrix", mat, new_fa)
    assert out == _cli("--seed", seed_sto, "--seed-structure", "--seed-each", "--seed-merged", merged_plain, new_fa)
    assert merged_file.read_text() == merged_plain.read_text() == each.merged.stockholm
    mc = each.merged.compare
    assert tsv.read_text() == mc.table and cols.read_text() == mc.columns_table and mat.read_text() == mc.matrix_table
    assert "# pp " in mc.table and int(mc.pp_residues.sum()) == sum(len(s) for s in seqs[4:])
    _check(mc, ref, each.merged.names, each.merged.rows, each.merged.ss, use_test=each.merged.rf.tolist())
    with pytest.raises(ValueError):
        pipeline.add_each(sn, sr, names[4:], seqs[4:], ctx=ctx, seed_ss=sss, compare=ref)
