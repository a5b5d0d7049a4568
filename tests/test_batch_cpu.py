"""CPU tests of the many-family batch (pipeline.run_batch, `dafs A B C`): the sub-batch packer, the readiness order of the
guide-tree forest, the node schedule (pipeline._solve_nodes) on a stand-in context, and the command line's refusal of the
single-input options -- before any HIP call."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
G = os.path.join(ROOT, "tests", "golden")


def test_pack_families_is_greedy_in_input_order():
    from dafs_amd.pipeline import pack_families
    assert pack_families([3, 3, 3, 3], 6) == [[0, 1], [2, 3]]
    assert pack_families([3, 4, 3], 6) == [[0], [1], [2]]
    assert pack_families([1, 1, 1], 100) == [[0, 1, 2]]
    # a family over the budget runs alone, the others pack around it
    assert pack_families([2, 50, 2, 2], 5) == [[0], [1], [2, 3]]
    assert pack_families([50], 5) == [[0]]
    assert pack_families([], 5) == []


def test_family_bytes_grows_with_the_family():
    from dafs_amd.pipeline import family_bytes
    one = family_bytes([100])
    assert one > 0
    assert family_bytes([100, 100]) > 2 * one
    assert family_bytes([100] * 10) > family_bytes([100] * 5) > family_bytes([100] * 2)
    assert family_bytes([200, 200]) > family_bytes([100, 100])


def _tree(n, merges):
    """(left, right) of a guide tree of n leaves from a list of (a, b) merges (node n + k is merge k)"""
    left = -np.ones(2 * n - 1, np.int64)
    right = -np.ones(2 * n - 1, np.int64)
    for k, (a, b) in enumerate(merges):
        left[n + k], right[n + k] = a, b
    return left, right


def test_forest_ready_order():
    from dafs_amd.pipeline import forest_ready
    trees = [_tree(3, [(0, 1), (3, 2)]), _tree(1, []), _tree(4, [(2, 3), (0, 1), (4, 5)])]
    pending = [(0, 3), (0, 4), (2, 4), (2, 5), (2, 6)]
    done = {(0, 0), (0, 1), (0, 2), (1, 0), (2, 0), (2, 1), (2, 2), (2, 3)}
    # every node whose children are done, whatever its family, in scheduling order
    assert forest_ready(trees, pending, done) == [(0, 3), (2, 4), (2, 5)]
    done |= {(0, 3), (2, 4)}
    assert forest_ready(trees, [(0, 4), (2, 5), (2, 6)], done) == [(0, 4), (2, 5)]
    done |= {(2, 5)}
    assert forest_ready(trees, [(2, 6)], done) == [(2, 6)]
    assert forest_ready(trees, [], done) == []


def test_run_batch_refuses_single_family_options():
    from dafs_amd import pipeline
    for kw in (dict(mp=None), dict(bp=None), dict(shard=None)):
        with pytest.raises(ValueError):
            pipeline.run_batch([(["a"], ["ACGU"])], **kw)
    with pytest.raises(TypeError):
        pipeline.run_batch([(["a"], ["ACGU"])], no_such_option=1)


@pytest.mark.parametrize("opt", [["--align-aux", "X"], ["--fold-aux", "X"], ["--save-align-aux", "X"], ["--save-fold-aux", "X"],
                                 ["--devices", "0,1"]])
def test_cli_refuses_single_input_options_with_several_files(opt):
    if not os.path.exists(DAFS):
        pytest.skip("the dafs executable is built by build()")
    a, b = os.path.join(G, "RF00005_0.fa"), os.path.join(G, "RF00017_4.fa")
    r = subprocess.run([DAFS] + opt + [a, b], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "single input FILE" in r.stderr
    assert r.stdout == ""


class _FakeNodes:
    """Context stand-in for pipeline._solve_nodes.  Node tuples are (key, len1, len2); a resident node finishes in the
    round in which it has run runs(key) rounds.  events: ("open", key) and ("finish", key) in order.  old: per round the
    keys of the old handles as passed; opening: the same keys in opening order."""

    def __init__(self, events, runs):
        self.events, self.runs, self.nodes, self.age, self.old, self.opening, self.solved, self.closed = events, runs, [], [], [], [], [], 0

    def _out(self, node):
        from dafs_amd.pipeline import NONE
        return dict(z=np.full(node[1], NONE, np.uint32), iterations=1, violated=0, ncbp=0, score=np.float32(0))

    def nodes_round(self, new_nodes, old_handles, prm, max_iterations, budget_us):
        assert not self.closed
        self.old.append([self.nodes[h][0] for h in old_handles])
        self.opening.append([self.nodes[h][0] for h in sorted(old_handles)])
        hs = list(range(len(self.nodes), len(self.nodes) + len(new_nodes)))
        for node in new_nodes:
            self.events.append(("open", node[0]))
            self.nodes.append(node)
            self.age.append(0)
        fin = []
        for h in list(old_handles) + hs:
            self.age[h] += 1
            fin.append(self.age[h] == self.runs(self.nodes[h][0]))
        return hs, [n[1:] for n in new_nodes], np.array(fin[:len(old_handles)], bool), np.array(fin[len(old_handles):], bool)

    def nodes_result(self, h, len1, len2):
        assert self.age[h] == self.runs(self.nodes[h][0]) and (len1, len2) == self.nodes[h][1:]
        return self._out(self.nodes[h])

    def nodes_memory(self):
        return (0, 0, 0)

    def nodes_demotions(self):
        return 0

    def nodes_close(self):
        self.closed += 1

    def solve_nodes(self, nodes, prm):
        assert not self.closed
        self.solved.append([n[0] for n in nodes])
        self.events += [("open", n[0]) for n in nodes]
        return [self._out(n) for n in nodes]


def _schedule(take_ready_of, level_sync, runs):
    """take_ready_of(done): the take_ready of one walk; done: the keys handed to finish so far"""
    from dafs_amd.pipeline import _solve_nodes
    events, done = [], set()
    ctx = _FakeNodes(events, runs)

    def finish(k, out, dims):
        assert k not in done
        done.add(k)
        events.append(("finish", k))
    levels, rounds, _, _ = _solve_nodes(ctx, None, take_ready_of(done), finish, level_sync, slice_iters=1)
    return ctx, events, levels, rounds


def _check_forest_schedule(level_sync):
    from dafs_amd.pipeline import forest_ready
    # a two-family forest, keys (family, node)
    trees = [_tree(3, [(0, 1), (3, 2)]), _tree(5, [(2, 3), (0, 1), (5, 4), (6, 7)])]
    inner = [(f, i) for f, (left, _) in enumerate(trees) for i in range(len(left)) if left[i] >= 0]

    def forest(done):
        pending = list(inner)
        leaves = {(f, i) for f, (left, _) in enumerate(trees) for i in range(len(left)) if left[i] < 0}

        def take_ready():
            nonlocal pending
            ready = forest_ready(trees, pending, leaves | done)
            pending = [q for q in pending if q not in ready]
            return [(q, (q, 10 + q[1], 20 + q[1])) for q in ready]
        return take_ready
    # rounds each node runs: (0, 4), opened in round 2, is still open in round 3 beside (1, 6), opened in round 1, so that
    # key order and opening order differ there; (1, 8) waits for (1, 6) and opens in round 4
    runs = {(0, 3): 1, (0, 4): 3, (1, 5): 1, (1, 6): 3, (1, 7): 1, (1, 8): 1}
    ctx, events, levels, rounds = _schedule(forest, level_sync, runs.get)
    opened = [k for e, k in events if e == "open"]
    assert sorted(opened) == sorted(inner) and len(set(opened)) == len(opened)
    assert sorted(k for e, k in events if e == "finish") == sorted(inner)
    for f, i in inner:  # a node opens only after both of its children (leaves aside) have gone to finish
        at = events.index(("open", (f, i)))
        for c in (trees[f][0][i], trees[f][1][i]):
            assert trees[f][0][c] < 0 or events.index(("finish", (f, c))) < at
    if level_sync:
        depth = {}
        for f, i in inner:  # merges are numbered bottom-up: children before parents
            depth[(f, i)] = 1 + max(depth.get((f, int(c)), 0) for c in (trees[f][0][i], trees[f][1][i]))
        assert levels == len(ctx.solved) == max(depth.values()) == 3
        assert [sorted(b) for b in ctx.solved] == [sorted(k for k in inner if depth[k] == d) for d in (1, 2, 3)]
        assert ctx.closed == 0 and rounds == []
    else:
        assert ctx.closed == 1 and levels == len(rounds) == len(ctx.old) == 4
        assert ctx.old == [[], [(1, 6)], [(0, 4), (1, 6)], [(0, 4)]]  # sorted by key, not in opening order
        assert ctx.opening[2] == [(1, 6), (0, 4)]
        for old, (_, nodes) in zip(ctx.old, rounds):
            assert [k for k, _, _ in nodes][:len(old)] == old


def test_solve_nodes_schedule():
    """pipeline._solve_nodes over a two-family forest (resident and level mode) and over pipeline.add's k independent
    nodes, all ready in the first round"""
    _check_forest_schedule(False)
    _check_forest_schedule(True)
    k = 7

    def add(done):
        batches = iter([[(j, (j, 5, 9)) for j in range(k)]])
        return lambda: next(batches, [])
    ctx, events, levels, rounds = _schedule(add, False, lambda j: 1 + j % 3)
    assert [k_ for e, k_ in events[:k]] == list(range(k)) and all(e == "open" for e, _ in events[:k])
    assert sorted(k_ for e, k_ in events if e == "finish") == list(range(k)) and len(events) == 2 * k
    assert ctx.closed == 1 and ctx.old[0] == [] and all(old == sorted(old) for old in ctx.old) and len(ctx.old) == 3
