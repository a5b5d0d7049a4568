"""GPU parity of k_contrafold in the forms its launch plan and its F5 chain switch between: both sides of the plan's two
switch points (asked of dafs_hipk_contrafold_plan on the device), the F5 chain cut into rounds of the workgroup size, the
constrained single-branch walks at spans beyond CF_MAX_SINGLE and CF_RING, short sequences under a long one's plan,
k_bp_compact with the threshold on a stored value, and the refusal at the length limit.  Every comparison is against the
oracle, bit for bit: the dense triangle and log Z (= F5i[L])."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ALPHABETS = ("ACGU", "ACGUTNacgu-")
PAIRS = ("AU", "UA", "GC", "CG", "GU", "UG")
_oracle_cache = {}


@pytest.fixture(scope="module")
def ctx():
    from dafs_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def rand_seq(seed, L, wide=False):
    rng = np.random.default_rng(seed)
    return "".join(rng.choice(list(ALPHABETS[1 if wide else 0]), L))


def orc_fold(oracle, s, cons=None):
    """(triangle, log Z) of the oracle, computed once per (sequence, constraint) and never written to"""
    key = (s, cons)
    if key not in _oracle_cache:
        L = len(s)
        post = np.zeros((L + 1) * (L + 2) // 2, np.float32)
        c = None if cons is None else cons.encode()
        assert oracle.lib.orc_contrafold_posterior(s.encode(), L, c, post.ctypes.data) == len(post)
        z = np.float32(oracle.lib.orc_contrafold_logz(s.encode(), L) if cons is None else
                       oracle.lib.orc_contrafold_logz_constrained(s.encode(), L, c))
        post.setflags(write=False)
        _oracle_cache[key] = (post, z)
    return _oracle_cache[key]


def orc_rows(oracle, s, cons, th):
    L = len(s)
    rp = np.zeros(L + 1, np.uint32); col = np.zeros(L * L + 1, np.uint32); val = np.zeros(L * L + 1, np.float32)
    n = oracle.lib.orc_fold_calculate(s.encode(), L, None if cons is None else cons.encode(), th, rp.ctypes.data, col.ctypes.data,
                                      val.ctypes.data)
    assert n >= 0
    return rp, col[:n].copy(), val[:n].copy()


def check_fold(ctx, oracle, s, cons=None, tag=None):
    want, wz = orc_fold(oracle, s, cons)
    post, z = ctx.fold_posterior_dense(s, cons)
    at = (tag, len(s), cons if cons is None or len(cons) <= 40 else cons[:40] + "...")
    assert np.float32(z).tobytes() == wz.tobytes(), at + (float(z), float(wz))
    assert post.tobytes() == want.tobytes(), at + (int((post != want).sum()), float(np.abs(post - want).max()))


def tri_rows(post, L, th):
    """the rows (i - 1) -> (j - 1, p) with p > th of a dense triangle, as the store lays them out"""
    rp, col, val, k = [0], [], [], 0
    for i in range(L + 1):
        row = post[k:k + L + 1 - i]
        k += L + 1 - i
        if i == 0:
            continue
        keep = np.nonzero(row > np.float32(th))[0]
        col.extend((keep + i - 1).tolist())
        val.extend(row[keep].tolist())
        rp.append(len(col))
    return np.array(rp, np.uint32), np.array(col, np.uint32), np.array(val, np.float32)


def tri_index(L, i, j):
    """offset of cell (i, j), 1-based positions, in the triangle of a sequence of L residues"""
    return i * (2 * (L + 1) - i - 1) // 2 + j


# ----- constraint strings

def random_structure(seed, L):
    """a nested (non-crossing) structure of three to six stems over L positions: (i, j) pairs, 0-based, and the string with
    '.' inside the hairpins and '?' everywhere else outside the stems"""
    rng = np.random.default_rng(seed)
    while True:
        want = int(rng.integers(3, 7))
        stems, regions = [], [(0, L)]
        while len(stems) < want and regions:
            lo, hi = regions.pop(int(rng.integers(len(regions))))
            h = int(rng.integers(2, 5))
            if hi - lo < 2 * h + 3:
                h = 2
            if hi - lo < 2 * h + 3:
                continue
            i = int(rng.integers(lo, hi - 2 * h - 3 + 1))
            j = int(rng.integers(i + 2 * h + 2, hi))
            stems.append((i, j, h))
            regions += [(lo, i), (i + h, j - h + 1), (j + 1, hi)]
        if len(stems) >= 3:
            break
    cons = ["?"] * L
    pairs = []
    for i, j, h in stems:
        for t in range(h):
            cons[i + t], cons[j - t] = "(", ")"
            pairs.append((i + t, j - t))
    for i, j, h in stems:
        if not any(i + h <= a and b <= j - h for a, b, _ in stems if (a, b) != (i, j)):   # nothing inside: a hairpin
            for t in range(i + h, j - h + 1):
                cons[t] = "."
    return pairs, "".join(cons)


def with_pairs(s, pairs, seed, spoil=None):
    """s with the residues under each pair made complementary; pair number `spoil` is left as A-A, which cannot pair"""
    rng = np.random.default_rng(seed)
    b = list(s)
    for k, (i, j) in enumerate(pairs):
        b[i], b[j] = ("A", "A") if k == spoil else tuple(PAIRS[int(rng.integers(len(PAIRS)))])
    return "".join(b)


def constrained_cases(L, seed):
    """the six (tag, sequence, constraint) of one length"""
    base = rand_seq(seed, L)
    far = min(L - 1, 64)   # more than 62 apart where the sequence has the room: no single-branch loop reaches across
    i = (L - 1 - far) // 2
    one = ["?"] * L
    one[i], one[i + far] = "(", ")"
    pairs, struct = random_structure(seed + 1, L)
    a = L // 2
    adj = ["?"] * L
    adj[a], adj[a + 1] = "(", ")"
    return [("free", base, "?" * L),
            ("unpaired", base, "." * L),
            ("far pair", with_pairs(base, [(i, i + far)], seed + 2), "".join(one)),
            ("structure", with_pairs(base, pairs, seed + 3), struct),
            ("structure, one pair that cannot form", with_pairs(base, pairs, seed + 3, spoil=len(pairs) // 2), struct),
            ("adjacent pair", with_pairs(base, [(a, a + 1)], seed + 4), "".join(adj))]


# ----- the plan on the device

@pytest.fixture(scope="module")
def device_plan(ctx):
    """{max_len: plan} for 1..400 with the static LDS size the runtime reports for k_contrafold, and La, Lb"""
    from dafs_amd import capi
    plans = {}
    for L in range(1, 401):
        p = capi.ContrafoldPlan()
        assert capi.contrafold_plan(L, 0, p) == 0
        plans[L] = p
    two = [L for L, p in plans.items() if p.pool_bufs == 2]
    ring = [L for L, p in plans.items() if p.use_ring]
    assert two and ring and max(two) < 400 and max(ring) < 400, (two[-1:], ring[-1:])
    la, lb = max(two), max(ring)
    print("k_contrafold on the device: static LDS %d bytes, La = %d, Lb = %d" % (plans[1].static_lds, la, lb))
    return plans, la, lb


def form(p):
    return {"threads": p.threads, "cell_waves": p.cell_waves, "use_ring": p.use_ring, "pool_bufs": p.pool_bufs, "pool_on": int(p.pool_floats > 0)}


def differing(a, b):
    fa, fb = form(a), form(b)
    return sorted(k for k in fa if fa[k] != fb[k])


def test_plan_switch_points(device_plan):
    """La (the last length with two pool buffers) and Lb (the last with the ring) exist below 400, in that order, and
    the plans on either side of each differ in that form alone; the ring's room goes to the pool."""
    plans, la, lb = device_plan
    assert la < lb
    assert differing(plans[la], plans[la + 1]) == ["pool_bufs"] and (plans[la].pool_bufs, plans[la + 1].pool_bufs) == (2, 1)
    assert differing(plans[lb], plans[lb + 1]) == ["use_ring"] and (plans[lb].use_ring, plans[lb + 1].use_ring) == (1, 0)
    assert plans[lb + 1].pool_floats > plans[lb].pool_floats > 0
    for L in (la, la + 1, lb, lb + 1):
        assert plans[L].static_lds + plans[L].lds <= 160 * 1024 - 512, L
        assert plans[L].static_lds == plans[1].static_lds


@pytest.mark.parametrize("which", ["La", "La+1", "Lb", "Lb+1"])
def test_folds_at_the_switch_points(ctx, oracle, device_plan, which):
    _, la, lb = device_plan
    L = {"La": la, "La+1": la + 1, "Lb": lb, "Lb+1": lb + 1}[which]
    check_fold(ctx, oracle, rand_seq(100 + L, L), tag=which)


def test_lists_overflow_the_pool_without_the_ring(ctx, oracle, device_plan):
    """a GC repeat pairs everywhere, so most of its lists do not fit the pool and the cells walk their partners themselves,
    reading FC from global memory: the even length just above Lb"""
    _, _, lb = device_plan
    L = lb + 1 + (lb + 1) % 2
    check_fold(ctx, oracle, "GC" * (L // 2), tag="GC repeat")


def test_lists_overflow_a_half_of_the_pool_with_the_ring(ctx, oracle, device_plan):
    """the same repeat at the even length up to La: two buffers and the ring, so the wavefronts without cells lay out the next
    span's lists beside the cells of this one, most lists do not fit their half, and the cells that walk their partners
    themselves read FC from the ring"""
    _, la, _ = device_plan
    s = "GC" * (la // 2)
    want, wz = orc_fold(oracle, s)
    assert not np.isnan(want).any() and not np.isnan(wz)
    check_fold(ctx, oracle, s, tag="GC repeat, two buffers")


# ----- the chunked F5 chain

CHUNKED = [(64, L) for L in (63, 64, 65, 128, 129, 200)] + [(128, 300)]


@pytest.mark.parametrize("threads,L", CHUNKED)
def test_f5_chain_in_rounds(ctx, oracle, monkeypatch, threads, L):
    """For j beyond the workgroup size the addends of F5i[j] come in several rounds and lane 0 takes the chain up again
    from the stored F5i[j].  Workgroups of 64 and 128 threads put sequences of a few hundred residues there: one, two and
    four rounds on both sides of a round's end.  Each length free over both alphabets and once under a structure."""
    monkeypatch.setenv("DAFS_HIP_CF_THREADS", str(threads))
    check_fold(ctx, oracle, rand_seq(200 + L, L), tag=threads)
    check_fold(ctx, oracle, rand_seq(300 + L, L, wide=True), tag=(threads, "wide"))
    pairs, struct = random_structure(400 + L, L)
    check_fold(ctx, oracle, with_pairs(rand_seq(500 + L, L), pairs, 600 + L), struct, tag=(threads, "structure"))


# ----- constrained walks

@pytest.mark.parametrize("env", [{}, {"DAFS_HIP_CF_NORING": "1"}, {"DAFS_HIP_CF_THREADS": "64"}], ids=["default", "noring", "threads64"])
@pytest.mark.parametrize("which", ["34", "65", "100", "181", "Lb+1"])
def test_constrained_walks_dense(ctx, oracle, device_plan, monkeypatch, which, env):
    """The constrained single-branch walks (their own break / continue rules over cum and map) at spans on both sides of
    CF_MAX_SINGLE = 30 and CF_RING = 33, the whole triangle and log Z: nothing forced, everything unpaired, one far pair, a
    random structure, the same with a pair that cannot form (dafs_fold_rows_constrained lets such strings through), and a
    pair of neighbours.  The oracle's answer to the strings that cannot be met is finite; that is checked first.
    (Of the walk's rules, the `break` at `!cf_all_unpaired(c, q, j)` only saves work: cum is monotone, so every lower q fails
    the same test and `continue` gives the same terms.  Dropping the test, or `continue` for the `break` of the p loop at
    `!cf_unpaired_pos(c, p)`, changes log Z in the structure and far-pair cases at every length here.)"""
    _, _, lb = device_plan
    L = lb + 1 if which == "Lb+1" else int(which)
    cases = constrained_cases(L, 700 + L)
    for tag, s, cons in cases:
        want, wz = orc_fold(oracle, s, cons)
        assert not np.isnan(want).any() and not np.isnan(wz), (tag, L)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for tag, s, cons in cases:
        check_fold(ctx, oracle, s, cons, tag=tag)


# ----- a batch under its longest member's plan

@pytest.fixture(scope="module")
def batch(device_plan):
    _, la, lb = device_plan
    lens = [lb + 40, 2, 5, 33, 65, la + 1, 181]
    seqs = [rand_seq(800 + k, L, wide=bool(k % 2)) for k, L in enumerate(lens)]
    cons = [None] * len(seqs)
    for k in (0, 4, 6):   # the longest (it then has no pool while the others do), the 65 nt one, and 181
        pairs, cons[k] = random_structure(900 + k, lens[k])
        seqs[k] = with_pairs(rand_seq(800 + k, lens[k]), pairs, 950 + k)
    return seqs, cons


@pytest.mark.parametrize("constrained", [False, True], ids=["free", "constrained"])
def test_batch_under_the_longest_members_plan(ctx, oracle, batch, constrained):
    """Short sequences in a batch run under the long one's plan (no ring, one buffer, a pool sized for max_len) with their
    own smaller carve.  The rows of every sequence against the oracle's, and the 65 nt member against its own dense fold."""
    seqs, cons = batch
    cons = cons if constrained else [None] * len(seqs)
    ctx.set_sequences(seqs)
    ctx.fold_posteriors(0.01, constraints=cons if constrained else None)
    got = ctx.bp(0)
    for k, (s, c, (rp, col, val)) in enumerate(zip(seqs, cons, got)):
        orp, ocol, oval = orc_rows(oracle, s, c, 0.01)
        assert np.array_equal(rp, orp) and np.array_equal(col, ocol) and val.tobytes() == oval.tobytes(), (k, len(s))
    post, _ = ctx.fold_posterior_dense(seqs[4], cons[4])
    rp, col, val = tri_rows(post, len(seqs[4]), 0.01)
    assert np.array_equal(got[4][0], rp) and np.array_equal(got[4][1], col) and got[4][2].tobytes() == val.tobytes()


# ----- k_bp_compact at its threshold

def test_threshold_on_a_stored_value(ctx, oracle):
    """k_bp_compact keeps p > th, strictly: with th on a value that one cell holds the store has every greater cell and not
    that one; one step of the threshold towards zero brings the cell in."""
    L = 65
    s = rand_seq(1000, L)
    want, _ = orc_fold(oracle, s)
    vals, counts = np.unique(want, return_counts=True)
    ok = vals[(counts == 1) & (vals > np.float32(0.01)) & (vals < np.float32(0.5))]
    assert len(ok), "the sequence has no value between 0.01 and 0.5 that occurs once"
    v = np.float32(ok[len(ok) // 2])
    at = int(np.nonzero(want == v)[0][0])
    i = next(i for i in range(1, L + 1) if tri_index(L, i, i) <= at <= tri_index(L, i, L))
    j = at - tri_index(L, i, 0)
    below = np.nextafter(v, np.float32(0))
    assert below < v
    ctx.set_sequences([s])
    for th, present in ((v, False), (below, True)):
        ctx.fold_posteriors(float(th))
        rp, col, val = ctx.bp(0)[0]
        orp, ocol, oval = orc_rows(oracle, s, None, float(th))
        assert np.array_equal(rp, orp) and np.array_equal(col, ocol) and val.tobytes() == oval.tobytes(), present
        assert len(val) == int((want > th).sum()) and (val > th).all()
        row = col[rp[i - 1]:rp[i]]
        assert ((j - 1) in row.tolist()) == present, (float(th), i, j)


# ----- the limit

def test_refusal_at_the_limit(ctx, oracle):
    """2132 nt is one more than the integer tables allow: DAFS_HIP_ETOOLONG before any kernel is launched, and the context
    goes on folding."""
    from dafs_amd import capi
    p = capi.ContrafoldPlan()
    assert capi.contrafold_plan(2131, 0, p) == 0 and capi.contrafold_plan(2132, 0, p) == -4
    ctx.stage_timing(True)
    try:
        ctx.stage_report()
        with pytest.raises(capi.DafsHipError) as e:
            ctx.fold_posterior_dense(rand_seq(1100, 2132))
        assert "code -4" in str(e.value)
        assert ctx.stage_report() == {}
        s = rand_seq(1101, 33)
        check_fold(ctx, oracle, s)
        rep = ctx.stage_report()
        assert rep["k_contrafold"][2] == 1 and rep["k_contrafold_posterior"][2] == 1, rep
    finally:
        ctx.stage_timing(False)
