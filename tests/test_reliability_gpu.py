"""GPU tests of the alignment-reliability annotation (dafs_hip_alignment_reliability, Context.alignment_reliability,
pipeline.run(reliability=True), dafs --stockholm) against the restatement of the definitions in tests/reliability_ref.py,
bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import reliability_ref as rr
import text_ref
from dafs_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
NONE = rr.NONE


def _split(recs):
    return [r[0] for r in recs], [r[1] for r in recs]


def _headers(path):
    """names as the command line sees them: the whole header line after '>'"""
    names, seqs = [], []
    with open(path) as fh:
        for line in fh:
            line = line.rstrip("\n")
            if line.startswith(">"):
                names.append(line[1:])
                seqs.append("")
            elif line:
                seqs[-1] += "".join(ch for ch in line if ch.isalpha())
    return names, seqs


def _alignment(res, first=0):
    """(seq, mask) of a Result's printed alignment (rows in output order = ascending sequence index)"""
    mask = np.array([[ch != "-" for ch in row] for row in res.rows], np.uint8)
    return np.arange(first, first + len(res.rows), dtype=np.uint32), mask


def _same(a, b):
    assert a["residue"].tobytes() == b["residue"].tobytes()
    for k in ("col", "pair", "pair_rows"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert np.float64(a["expected_accuracy"]).tobytes() == np.float64(b["expected_accuracy"]).tobytes()


def _ctx():
    from dafs_amd import capi
    return capi.Context(0)


@pytest.mark.parametrize("weights", [dict(), dict(w_pct_a=0.0, w_pct_s=0.0)])
@pytest.mark.parametrize("which", ["family", "random", "rf00005"])
def test_against_restatement(which, weights):
    from dafs_amd import pipeline
    if which == "rf00005":  # a family with a consensus structure: the pair values are exercised
        names, seqs = _headers(os.path.join(G, "RF00005_0.fa"))
    else:
        names, seqs = _split(synth.family_set(8, 90, seed=61) if which == "family" else synth.random_set(6, 80, seed=62))
    ctx = _ctx()
    try:
        res = pipeline.run(names, seqs, ctx=ctx, reliability=True, **weights)
        mpr = 1 if weights.get("w_pct_a", 0.25) != 0 else 0
        bpr = 1 if weights.get("w_pct_s", 0.25) != 0 else 0
        seq, mask = _alignment(res)
        got = ctx.alignment_reliability(seq, mask, res.ss, mp_relaxed=mpr, bp_relaxed=bpr)
        want = rr.restate(seq, mask, res.ss, *rr.context_stores(ctx, mpr, bpr))
        _same(got, want)
        if which == "rf00005":
            assert (res.ss != NONE).any() and want["pair_rows"].max() > 0 and want["pair"].max() > 0
        # the driver's annotation is this one (it picks the stores phase 2 read), rows in output order
        assert np.concatenate(res.reliability["residue"]).tobytes() == got["residue"].tobytes()
        assert res.reliability["col"].tobytes() == got["col"].tobytes()
        # the order of the given rows changes no bit; repeated calls repeat
        perm = np.random.RandomState(5).permutation(len(seq))
        pg = ctx.alignment_reliability(seq[perm], mask[perm], res.ss, mp_relaxed=mpr, bp_relaxed=bpr)
        lens = mask.sum(1)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        back = np.concatenate([got["residue"][off[r]:off[r + 1]] for r in perm])
        assert pg["residue"].tobytes() == back.tobytes()
        _same(dict(pg, residue=got["residue"]), got)
        _same(ctx.alignment_reliability(seq, mask, res.ss, mp_relaxed=mpr, bp_relaxed=bpr), got)
        # no structure: no pairs, the rest unchanged
        ns = ctx.alignment_reliability(seq, mask, None, mp_relaxed=mpr, bp_relaxed=bpr)
        assert ns["residue"].tobytes() == got["residue"].tobytes() and not ns["pair_rows"].any()
        assert ((got["residue"] >= 0) & (got["residue"] <= 1)).all()
    finally:
        ctx.close()


def test_batch_equals_separate_runs_and_single_sequence():
    from dafs_amd import pipeline
    fams = [_headers(os.path.join(G, "RF00005_0.fa")), _split(synth.random_set(1, 40, seed=63)), _split(synth.family_set(5, 70, seed=64)),
            _split(synth.random_set(3, 60, seed=65))]
    ctx = _ctx()
    try:
        got = pipeline.run_batch(fams, ctx=ctx, reliability=True)
        for (names, seqs), r in zip(fams, got):
            one = pipeline.run(names, seqs, ctx=ctx, reliability=True)
            assert r.output == one.output
            assert r.stockholm == one.stockholm, names[0]
            for a, b in zip(r.reliability["residue"], one.reliability["residue"]):
                assert a.tobytes() == b.tobytes()
            for k in ("col", "pair", "pair_rows"):
                assert r.reliability[k].tobytes() == one.reliability[k].tobytes()
            assert r.reliability["expected_accuracy"] == one.reliability["expected_accuracy"]
        single = got[1]
        assert single.reliability["residue"][0].tolist() == [1.0] * len(fams[1][1][0]) and single.reliability["expected_accuracy"] == 1.0
        pp = [ln for ln in single.stockholm.split("\n") if ln.startswith("#=GR") or ln.startswith("#=GC PP_cons")]
        assert len(pp) == 2 and all(set(ln.split()[-1]) == {"*"} for ln in pp)
    finally:
        ctx.close()


def test_rows_from_two_families_are_refused_and_the_context_stays_usable():
    from dafs_amd import capi, pipeline
    fams = [_split(synth.family_set(4, 60, seed=66)), _split(synth.random_set(3, 50, seed=67))]
    ctx = _ctx()
    try:
        got = pipeline.run_batch(fams, ctx=ctx)
        seq, mask = _alignment(got[1], first=4)
        good = ctx.alignment_reliability(seq, mask)
        mixed = np.array([0, 4], np.uint32)
        L = max(len(s) for s in fams[0][1][:1] + fams[1][1][:1])
        m2 = np.zeros((2, L), np.uint8)
        m2[0, :len(fams[0][1][0])] = 1
        m2[1, :len(fams[1][1][0])] = 1
        with pytest.raises(capi.DafsHipError):
            ctx.alignment_reliability(mixed, m2)
        short = mask.copy()
        short[0, np.nonzero(short[0])[0][0]] = 0
        with pytest.raises(capi.DafsHipError):  # a mask that does not place every residue of its sequence
            ctx.alignment_reliability(seq, short)
        with pytest.raises(capi.DafsHipError):  # a pair that ends before it starts
            ctx.alignment_reliability(seq, mask, np.array([NONE] * (mask.shape[1] - 1) + [0], np.uint32))
        with pytest.raises(capi.DafsHipError):  # one sequence twice
            ctx.alignment_reliability(np.array([4, 4], np.uint32), np.stack([mask[0], mask[0]]))
        _same(ctx.alignment_reliability(seq, mask), good)
    finally:
        ctx.close()


def run_cli(*args):
    r = subprocess.run([DAFS] + list(args), capture_output=True, text=True, timeout=600)
    return r.returncode, r.stdout, r.stderr


def _parse(sto):
    """per block: ([rows], SS_cons, [PP lines])"""
    out = []
    for blk in sto.split("//\n")[:-1]:
        rows, ss, pps = [], None, []
        for ln in blk.split("\n"):
            if not ln or ln.startswith("# STOCKHOLM") or ln.startswith("#=GF"):
                continue
            if ln.startswith("#=GC SS_cons"):
                ss = ln.split()[-1]
            elif ln.startswith("#=GR") or ln.startswith("#=GC PP_cons"):
                pps.append(ln)
            else:
                rows.append(ln.split()[-1])
        out.append((rows, ss, pps))
    return out


@pytest.mark.parametrize("flags", [[], ["-a", "CONTRAlign"]])
def test_cli_stockholm(tmp_path, flags):
    from dafs_amd import capi, pipeline
    path = os.path.join(G, "RF00005_0.fa")
    rc, want, err = run_cli(*flags, path)
    assert rc == 0, err
    sto = str(tmp_path / "a.sto")
    rc, out, err = run_cli(*flags, "--stockholm", sto, path)
    assert rc == 0, err
    assert out == want  # stdout unchanged
    text = open(sto).read()
    (rows, ss, pps), = _parse(text)
    lines = out.split("\n")
    assert ss == lines[2]
    assert rows == lines[4::2][:len(rows)] and len(rows) == (len(lines) - 4) // 2
    # the Python driver writes the same bytes, with the same writer; the restatement builds them from the result's arrays
    names, seqs = _headers(path)
    res = pipeline.run(names, seqs, reliability=True, align_model=capi.ALIGN_CONTRALIGN if flags else capi.ALIGN_PROBCONS)
    assert res.output == out
    assert res.stockholm == text
    assert text_ref.result_block(res, names) == text
    # several files: one block each, in input order, each the file's own
    fam = str(tmp_path / "fam.fa")
    with open(fam, "w") as f:
        f.write(synth.to_fasta(synth.family_set(5, 70, seed=68)))
    sto2, sto3 = str(tmp_path / "b.sto"), str(tmp_path / "c.sto")
    rc, _, err = run_cli(*flags, "--stockholm", sto2, fam)
    assert rc == 0, err
    rc, _, err = run_cli(*flags, "--stockholm", sto3, path, fam)
    assert rc == 0, err
    assert open(sto3).read() == text + open(sto2).read()


def test_cli_stockholm_devices_and_refinement(tmp_path):
    path = os.path.join(G, "RF00005_0.fa")
    a, b = str(tmp_path / "a.sto"), str(tmp_path / "b.sto")
    rc, out0, err = run_cli("--stockholm", a, path)
    assert rc == 0, err
    rc, out1, err = run_cli("--devices", "0,0", "--stockholm", b, path)
    assert rc == 0, err
    assert out1 == out0 and open(b).read() == open(a).read()
    # -r and --bp-update1: the annotation is of what is printed
    for fl in (["-r", "3"], ["--bp-update1"]):
        rc, out, err = run_cli(*fl, "--stockholm", a, path)
        assert rc == 0, err
        (rows, ss, pps), = _parse(open(a).read())
        lines = out.split("\n")
        assert ss == lines[2] and rows == lines[4::2][:len(rows)]


@pytest.mark.parametrize("cfg", [(128, 150), (256, 200)])
def test_size(cfg):
    """c3-sized and c4 random sets: values in [0, 1] and a sample of residues against the restatement"""
    from dafs_amd import pipeline
    names, seqs = _split(synth.random_set(cfg[0], cfg[1], seed=12345))
    ctx = _ctx()
    try:
        res = pipeline.run(names, seqs, ctx=ctx, reliability=True)
        seq, mask = _alignment(res)
        got = ctx.alignment_reliability(seq, mask, res.ss)
        for k in ("residue", "col", "pair"):
            assert ((got[k] >= 0) & (got[k] <= 1)).all(), k
        assert 0 < got["expected_accuracy"] <= 1
        mp_row, _ = rr.context_stores(ctx, 1, 1)
        off = np.concatenate([[0], np.cumsum(mask.sum(1))]).astype(np.int64)
        pos = np.cumsum(mask, axis=1) - 1
        rs = np.random.RandomState(9)
        for r in rs.choice(len(seq), 6, replace=False):
            cols = np.nonzero(mask[r])[0]
            for c in rs.choice(cols, 4, replace=False):
                i = int(pos[r, c])
                acc = 0.0
                for q in range(len(seq)):
                    if q == r:
                        continue
                    cc, vv = mp_row(int(seq[r]), int(seq[q]), i)
                    if mask[q, c]:
                        acc += rr._lookup(cc, vv, int(pos[q, c]))
                    else:
                        acc += max(0.0, 1.0 - rr._mass(vv))
                assert got["residue"][off[r] + i] == acc / (len(seq) - 1), (r, c)
    finally:
        ctx.close()
