"""GPU tests of the covariation statistics (dafs_hip_alignment_covariation, Context.alignment_covariation,
pipeline.run(covariation=...), dafs --covariation) against the restatement of the definitions in tests/covariation_ref.py,
bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

import covariation_ref as cr
import text_ref
from dafs_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
NONE = cr.NONE
FLOATS = ("best_score", "best_e", "pair_score", "pair_e")
INTS = ("col_sum", "best", "pair_rows", "pair_canonical", "pair_types")


def _ctx():
    from dafs_amd import capi
    return capi.Context(0)


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


def _same(got, want, keys=FLOATS + INTS + ("total", "g")):
    """every output equal to the bit; a NaN equals a NaN"""
    for k in keys:
        if k == "g" and ("g" not in got or "g" not in want):
            continue
        if k == "total":
            assert int(got[k]) == int(want[k])
        elif k in FLOATS:
            a, b = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
            assert np.array_equal(np.isnan(a), np.isnan(b)), k
            assert a[~np.isnan(a)].tobytes() == b[~np.isnan(b)].tobytes(), (k, a, b)
        else:
            assert np.asarray(got[k]).astype(np.int64).tobytes() == np.asarray(want[k]).astype(np.int64).tobytes(), k


def _random_code(n, length, seed, other=0.12):
    rs = np.random.RandomState(seed)
    code = rs.randint(0, 4, (n, length)).astype(np.uint8)
    if n > 1 and length > 3:  # some signal: column 1 follows column 0, column 2 is almost conserved
        code[:, 1] = (3 - code[:, 0]) % 4
        code[:, 2] = 2
        code[rs.rand(n) < 0.2, 2] = 0
    code[rs.rand(n, length) < other] = 4
    if length > 8:
        code[:, 5] = 4        # an all-gap column
        code[:, 7] = 4        # a column with a single nucleotide
        code[n // 2, 7] = 1
    return code


def _random_ss(length, seed, pairs=None):
    """a valid structure: disjoint column pairs (left -> right), nested or not"""
    ss = np.full(length, NONE, np.uint32)
    cols = list(np.random.RandomState(seed).permutation(length))
    for _ in range(length // 4 if pairs is None else pairs):
        if len(cols) < 2:
            break
        a, b = sorted((int(cols.pop()), int(cols.pop())))
        ss[a] = b
    return ss


# (n, len, shuffles, with a structure); the planes are words of 32 rows: 31, 32, 33 and 63, 64, 65 sit at word edges
HAND = [(1, 9, 3, True), (2, 12, 3, True), (63, 40, 1, True), (64, 40, 0, True), (65, 40, 100, True), (200, 300, 1, True),
        (31, 20, 2, True), (32, 20, 2, True), (33, 20, 2, True), (6, 1, 2, False), (6, 2, 2, True), (1, 1, 0, False), (33, 70, 100, False), (40, 65, 0, False), (17, 17, 1, True)]


@pytest.mark.parametrize("n,length,shuffles,with_ss", HAND)
def test_handmade_alignments_equal_the_restatement(n, length, shuffles, with_ss):
    code = _random_code(n, length, seed=1000 + n + length)
    ss = _random_ss(length, seed=n) if with_ss else None
    want = cr.restate(code, ss, shuffles, seed=77)
    ctx = _ctx()
    try:
        got = ctx.alignment_covariation(code, ss, shuffles=shuffles, seed=77, matrix=True)
        _same(got, want)
        assert got["total"] == int(got["col_sum"].sum())
        # text rows give the same codes; without the matrix nothing else changes
        text = ["".join("ACGU-"[v] for v in row) for row in code]
        _same(ctx.alignment_covariation(text, ss, shuffles=shuffles, seed=77), want)
        # codes of another integer type are cast, not reinterpreted; anything else is refused
        _same(ctx.alignment_covariation(code.astype(np.int64), ss, shuffles=shuffles, seed=77), want)
        with pytest.raises(ValueError):
            ctx.alignment_covariation(code.astype(np.float64), ss)
        with pytest.raises(ValueError):
            ctx.alignment_covariation(code.astype(np.int64) + 300, ss)
    finally:
        ctx.close()


RUNS = {"rf00005": lambda: _headers(os.path.join(G, "RF00005_0.fa")),
        "family": lambda: _split(synth.family_set(8, 90, seed=71)),
        "random": lambda: _split(synth.random_set(6, 80, seed=72))}


@pytest.mark.parametrize("which", sorted(RUNS))
def test_runs_equal_the_restatement(which):
    """pipeline.run(covariation=...) is a direct call on the printed rows and structure, which is the restatement"""
    from dafs_amd import pipeline
    names, seqs = RUNS[which]()
    ctx = _ctx()
    try:
        plain = pipeline.run(names, seqs, ctx=ctx)
        res = pipeline.run(names, seqs, ctx=ctx, covariation=dict(shuffles=100, seed=5))
        assert res.output == plain.output and not hasattr(plain, "covariation")
        want = cr.restate(cr.encode(res.rows), res.ss, 100, seed=5)
        _same(res.covariation, want)
        _same(ctx.alignment_covariation(res.rows, res.ss, shuffles=100, seed=5, matrix=True), want)
        if which == "rf00005":
            assert (res.ss != NONE).any() and want["pair_rows"].max() > 0
        assert pipeline.run(names, seqs, ctx=ctx, covariation=True).covariation["best_e"].tobytes() == \
            ctx.alignment_covariation(res.rows, res.ss, shuffles=100, seed=1)["best_e"].tobytes()
    finally:
        ctx.close()


def test_planted_covariation():
    code, ss = cr.planted_alignment()
    ctx = _ctx()
    try:
        got = ctx.alignment_covariation(code, ss, shuffles=100, seed=12345)
    finally:
        ctx.close()
    for c in np.nonzero(ss != NONE)[0]:
        print("planted", c, int(ss[c]), got["pair_score"][c], got["pair_e"][c])
    others = np.array([c for c in range(len(ss)) if got["best_e"][c] > 0.05])
    print("largest other best score", got["best_score"][others].max(), "E", got["best_e"][others].min())
    cr.check_planted(got, ss)


def test_row_order_and_chunking_change_no_bit(monkeypatch):
    code = _random_code(200, 90, seed=31)  # 7 words of 32 rows
    ss = _random_ss(90, seed=3)
    ctx = _ctx()
    try:
        monkeypatch.delenv("DAFS_COV_CHUNK_WORDS", raising=False)
        want = ctx.alignment_covariation(code, ss, shuffles=0, matrix=True)
        perm = np.random.RandomState(8).permutation(len(code))
        _same(ctx.alignment_covariation(code[perm], ss, shuffles=0, matrix=True), want)
        null = ctx.alignment_covariation(code, ss, shuffles=3, seed=9, matrix=True)
        _same(null, cr.restate(code, ss, 3, seed=9))
        for chunk in ("1", "2", "3", "7", "32"):  # the LDS stage in words; 3 leaves a short last chunk
            monkeypatch.setenv("DAFS_COV_CHUNK_WORDS", chunk)
            _same(ctx.alignment_covariation(code, ss, shuffles=3, seed=9, matrix=True), null)
    finally:
        ctx.close()


def test_batch_and_add_equal_a_direct_call():
    from dafs_amd import pipeline
    fams = [_headers(os.path.join(G, "RF00005_0.fa")), _split(synth.random_set(1, 40, seed=73)), _split(synth.family_set(5, 70, seed=74))]
    opt = dict(shuffles=20, seed=3)
    ctx = _ctx()
    try:
        got = pipeline.run_batch(fams, ctx=ctx, reliability=True, covariation=opt)
        for (names, seqs), r in zip(fams, got):
            _same(r.covariation, ctx.alignment_covariation(r.rows, r.ss, **opt))
            one = pipeline.run(names, seqs, ctx=ctx, reliability=True, covariation=opt)
            assert one.stockholm == r.stockholm and pipeline.covariation_tsv(one) == pipeline.covariation_tsv(r)
            assert ("#=GC cov_SS_cons" in r.stockholm) and r.output == one.output
        assert not got[1].covariation["col_sum"].any() and (got[1].covariation["best"] == NONE).all()  # one row: no statistics
        names, seqs = fams[2]
        seed = pipeline.run(names[:3], seqs[:3], ctx=ctx)
        added = pipeline.add(names[:3], seed.rows, names[3:], seqs[3:], ctx=ctx, reliability=True, covariation=opt)
        _same(added.covariation, ctx.alignment_covariation(added.rows, added.ss, **opt))
        plain = pipeline.add(names[:3], seed.rows, names[3:], seqs[3:], ctx=ctx, reliability=True)
        assert plain.output == added.output and not hasattr(plain, "covariation")
        lines = added.stockholm.split("\n")
        k = [i for i, ln in enumerate(lines) if ln.startswith("#=GC cov_SS_cons")]
        assert len(k) == 1 and lines[k[0] - 1].startswith("#=GC PP_cons") and lines[k[0] + 1].startswith("#=GC RF")
    finally:
        ctx.close()


def run_cli(*args):
    r = subprocess.run([DAFS] + list(args), capture_output=True, text=True, timeout=600)
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("flags", [[], ["-a", "CONTRAlign"]])
def test_cli_equals_python(tmp_path, flags):
    from dafs_amd import capi, pipeline
    kw = dict(align_model=capi.ALIGN_CONTRALIGN if flags else capi.ALIGN_PROBCONS, reliability=True)
    path = os.path.join(G, "RF00005_0.fa")
    names, seqs = _headers(path)
    rc, want_out, err = run_cli(*flags, path)
    assert rc == 0, err
    tsv, sto = str(tmp_path / "a.tsv"), str(tmp_path / "a.sto")
    rc, out, err = run_cli(*flags, "--covariation", tsv, "--cov-shuffles", "30", "--cov-seed", "11", "--stockholm", sto, path)
    assert rc == 0, err
    assert out == want_out  # stdout never changes
    res = pipeline.run(names, seqs, covariation=dict(shuffles=30, seed=11), **kw)
    assert res.output == out
    assert open(tsv).read() == pipeline.covariation_tsv(res) and open(tsv).read().count("\tss\t") == int((res.ss != NONE).sum())
    assert open(sto).read() == res.stockholm and "#=GC cov_SS_cons" in res.stockholm
    # both sides of those two go through the library's formatter: the restatement builds the same bytes from the result's arrays
    assert open(tsv).read() == text_ref.covariation_tsv(res) and open(sto).read() == text_ref.result_block(res, names)
    # the defaults: 100 shuffles, seed 1; without --stockholm the table alone
    rc, out, err = run_cli(*flags, "--covariation", tsv, path)
    assert rc == 0 and out == want_out, err
    dflt = pipeline.run(names, seqs, covariation=True, **kw)
    assert open(tsv).read() == pipeline.covariation_tsv(dflt) == text_ref.covariation_tsv(dflt)
    if flags:
        return
    # two files: the blocks of stdout, in order, each the file's own
    fam = str(tmp_path / "fam.fa")
    recs = synth.family_set(5, 70, seed=75)
    with open(fam, "w") as f:
        f.write(synth.to_fasta(recs))
    rc, out2, err = run_cli(path, fam)
    assert rc == 0, err
    rc, out, err = run_cli("--covariation", tsv, "--cov-shuffles", "30", "--cov-seed", "11", "--stockholm", sto, path, fam)
    assert rc == 0 and out == out2, err
    res2 = pipeline.run(*_split(recs), covariation=dict(shuffles=30, seed=11), **kw)
    assert open(tsv).read() == "==> %s <==\n%s==> %s <==\n%s" % (path, pipeline.covariation_tsv(res), fam, pipeline.covariation_tsv(res2))
    assert open(sto).read() == res.stockholm + res2.stockholm
    assert open(tsv).read() == "==> %s <==\n%s==> %s <==\n%s" % (path, text_ref.covariation_tsv(res), fam, text_ref.covariation_tsv(res2))
    assert open(sto).read() == text_ref.result_block(res, names) + text_ref.result_block(res2, _split(recs)[0])
    # --seed: the new sequences of fam added to the alignment of its first three
    n5, s5 = _split(recs)
    seed_fa, new_fa, seed_aln = str(tmp_path / "seed.fa"), str(tmp_path / "new.fa"), str(tmp_path / "seed.aln")
    with open(seed_fa, "w") as f:
        f.write(synth.to_fasta(recs[:3]))
    with open(new_fa, "w") as f:
        f.write(synth.to_fasta(recs[3:]))
    rc, aln, err = run_cli(seed_fa)
    assert rc == 0, err
    with open(seed_aln, "w") as f:
        f.write(aln)
    from dafs_amd import stockholm
    snames, srows = stockholm.read_seed(seed_aln)
    rc, out3, err = run_cli("--seed", seed_aln, new_fa)
    assert rc == 0, err
    rc, out, err = run_cli("--seed", seed_aln, "--covariation", tsv, "--cov-shuffles", "30", "--cov-seed", "11", "--stockholm", sto, new_fa)
    assert rc == 0 and out == out3, err
    added = pipeline.add(snames, srows, n5[3:], s5[3:], reliability=True, covariation=dict(shuffles=30, seed=11))
    assert added.output == out and open(tsv).read() == pipeline.covariation_tsv(added) and open(sto).read() == added.stockholm
    assert open(tsv).read() == text_ref.covariation_tsv(added) and open(sto).read() == text_ref.result_block(added, snames + n5[3:], added.rf)
    assert text_ref.clean_seed(*text_ref.parse_seed(aln)) == (snames, srows)


def test_refusals_leave_the_context_usable():
    from dafs_amd import capi
    code = _random_code(12, 30, seed=41)
    ss = _random_ss(30, seed=4)
    ctx = _ctx()
    try:
        good = ctx.alignment_covariation(code, ss, shuffles=2, matrix=True)
        bad_ss = ss.copy()
        bad_ss[29] = 0  # a pair that ends before it starts
        with pytest.raises(capi.DafsHipError):
            ctx.alignment_covariation(code, bad_ss, shuffles=2)
        twice = np.full(30, NONE, np.uint32)
        twice[0], twice[1] = 5, 5  # a column in two pairs
        with pytest.raises(capi.DafsHipError):
            ctx.alignment_covariation(code, twice, shuffles=2)
        high = code.copy()
        high[3, 3] = 5
        with pytest.raises(capi.DafsHipError):
            ctx.alignment_covariation(high, ss, shuffles=2)
        out = np.zeros(8, np.float64)
        args = [None] * 11
        # n * len^2 above 2^45 and n above 2^20: refused from the sizes alone, before the codes are read
        for n, length in ((1 << 20, 1 << 13), ((1 << 20) + 1, 2)):
            assert capi._alignment_covariation(ctx._h, n, length, out.ctypes.data, None, 0, 1, *args) == -1
        _same(ctx.alignment_covariation(code, ss, shuffles=2, matrix=True), good)
    finally:
        ctx.close()


def test_size(tmp_path):
    """512 x 12 000 with two shuffles completes; sampled columns against the restatement's rows of Gq"""
    n, length = 512, 12000
    rs = np.random.RandomState(51)
    code = np.tile(rs.randint(0, 4, length), (n, 1))
    redraw = rs.rand(n, length) < 0.3
    code[redraw] = rs.randint(0, 4, int(redraw.sum()))
    code[rs.rand(n, length) < 0.1] = 4
    code = code.astype(np.uint8)
    # the large call runs in a process of its own, under its own time limit
    np.save(str(tmp_path / "code.npy"), code)
    child = ("import sys, numpy as np; sys.path.insert(0, %r); from dafs_amd import capi; ctx = capi.Context(0); "
             "out = ctx.alignment_covariation(np.load(sys.argv[1]), None, shuffles=2, seed=3); ctx.close(); np.savez(sys.argv[2], **out)" % ROOT)
    subprocess.run([sys.executable, "-c", child, str(tmp_path / "code.npy"), str(tmp_path / "out.npz")], check=True, timeout=300)
    got = dict(np.load(str(tmp_path / "out.npz")))
    got["total"] = int(got["total"])
    assert got["total"] == int(got["col_sum"].sum())
    assert not np.isnan(got["best_e"]).any() and (got["best_e"] >= 0).all()
    table = np.array(cr.lnq(n), np.int64)
    one = np.stack([(code == a) for a in range(4)]).astype(np.int64)  # [4, n, len]
    for c in rs.choice(length, 8, replace=False):
        nab = np.einsum("ar,brc->abc", one[:, :, c], one)  # [4, 4, len]
        ra, sb = nab.sum(1), nab.sum(0)
        m = ra.sum(0)
        row = np.zeros(length, np.int64)
        for a in range(4):
            for b in range(4):
                row += nab[a, b] * (table[nab[a, b]] + table[m] - table[ra[a]] - table[sb[b]])
        row *= 2
        row[c] = 0
        assert int(row.sum()) == int(got["col_sum"][c]), c
        s = np.array([cr.s_scalar(int(row[d]), int(got["col_sum"][c]), int(got["col_sum"][d]), got["total"], length) for d in range(length)])
        s[c] = -np.inf
        assert int(s.argmax()) == int(got["best"][c]) and s.max() == got["best_score"][c], c
