"""CPU tests of the many-family batch (pipeline.run_batch, `dafs A B C`): the sub-batch packer, the readiness order of the
guide-tree forest, and the command line's refusal of the single-input options -- before any HIP call."""
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
