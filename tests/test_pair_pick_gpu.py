"""GPU parity of k_pairhmm3's candidate pick (pairhmm3.hip sweep 2p, pair_sweeps.h sweeps 3b and 3c) and of its fallback.

Sweep 2p stores no F + B plane: it picks, per lane and step, the cells whose posterior can reach th (against totF, with
a margin) into per-lane candidate lists; sweep 3b turns the records into posteriors and exact entry masks, sweep 3c runs
the similarity DP and the counts from them and writes the final records over the dead forward plane.  A wavefront with
a pair whose margin did not hold, or with a full list, runs the classic sweeps from the intact forward plane.

Every launch is compared with the oracle bit for bit (pair_raw.check: row pointers, columns, values, transposed rows,
nnz, sim), so no tolerance is involved; test_modes_agree also compares the launches of the modes with one another.
The switches reach the library through the child's environment:
  default                            the pick, delta = 1/8
  DAFS_HIP_PAIR_PICK=0               every wavefront on the classic path
  DAFS_HIP_PAIR_PICK_MARGIN=0        every pair fails the trust check: sweep 2p, then the fallback
  DAFS_HIP_PAIR_PICK_MARGIN=1024     delta = 1: many false candidates, whose records sweep 3c must pass over
Which path a wavefront took cannot be seen from outside; where a case is built to overflow the candidate lists, the
assertion is equality."""
import random

import numpy as np
import pytest

import pair_raw
from dafs_amd import synth
from test_pair_rounds_gpu import ORDERS, SEQS

pytestmark = pytest.mark.gpu

FILL = 0x3F800000  # 1.0: as a slab sum far above `total`, as a record an entry mask with bits set
THS = (0.002, 0.01, 0.3, 0.999)
INSTANCES = ((16, 2), (16, 3), (32, 2), (64, 1), None)  # forced (G, W); None: the planner's choice
MODES = {"default": {}, "classic": {"DAFS_HIP_PAIR_PICK": "0"}, "margin0": {"DAFS_HIP_PAIR_PICK_MARGIN": "0"},
         "margin1024": {"DAFS_HIP_PAIR_PICK_MARGIN": "1024"}}


def _rand(n, seed):
    r = random.Random(seed)
    return "".join(r.choice("ACGU") for _ in range(n))


def _set_mode(monkeypatch, mode):
    for k in ("DAFS_HIP_PAIR_PICK", "DAFS_HIP_PAIR_PICK_MARGIN"):
        monkeypatch.delenv(k, raising=False)
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)  # pair_raw.run hands the parent's environment to its child


def _edge_lengths(inst):
    """1, 2, 3, the longest second sequence of the W - 1 form, the shortest of the W form, the longest the instance takes,
    and two first sequences far longer / shorter than the second ones"""
    if inst is None:
        return [1, 2, 3, 15, 16, 31, 47, 63, 70, 5]
    g, w = inst
    edges = [g * (w - 1) - 1, g * (w - 1), g * w - 1] if w > 1 else [g - 2, g - 1]
    return [1, 2, 3] + edges + [70, 5]


def _edge_tasks(seqs, inst):
    """every ordered pair the instance takes (second sequence below G * W), an odd number of them: at G = 16 and 32 the
    last batch has idle groups; the order mixes lengths, so wavefronts hold pairs of different L1 and the launch has
    wavefronts of the W and of the W - 1 form"""
    cap = inst[0] * inst[1] - 1 if inst else 10 ** 6
    tasks = [(x, y) for x in range(len(seqs)) for y in range(len(seqs)) if x != y and len(seqs[y]) <= cap]
    random.Random(len(tasks)).shuffle(tasks)
    return tasks if len(tasks) % 2 else tasks[:-1]


def _family(lengths, seed):
    """related sequences cut to the given lengths: a band of high posteriors"""
    base = [s for _, s in synth.family_set(len(lengths), max(lengths) + 8, seed=seed)]
    return [s[:n] for s, n in zip(base, lengths)]


def _edge_launches(oracle):
    launches = []
    for inst in INSTANCES:
        lens = _edge_lengths(inst)
        for seqs in ([_rand(n, 500 + 7 * k + n) for k, n in enumerate(lens)], _family(lens, 77)):
            assert [len(s) for s in seqs] == lens
            tasks = _edge_tasks(seqs, inst)
            assert len(tasks) % 2 == 1 and len(tasks) >= 9
            for th in THS:
                launches.append(pair_raw.spec(oracle, 0, th, seqs, tasks, FILL if not launches else "keep", force=inst))
    return launches


def _check_all(oracle, outs):
    for out in outs:
        L = out["spec"]
        if L["force"]:
            g = pair_raw.geometry(out)
            assert [g["group"], g["width"]] == L["force"], g
        pair_raw.check(oracle, out, L["seqs"], L["tasks"], L["th"], L["model"])


@pytest.mark.parametrize("mode", ["default", "margin0", "margin1024"])
def test_edges_of_every_form(oracle, tmp_path, monkeypatch, mode):
    """Second sequences of 1, 2, 3, G (W - 1) - 1, G (W - 1) and G W - 1 residues against first sequences of 1 .. 70, random
    and related, at four thresholds, on <16,2>, <16,3>, <32,2>, <64,1> and the planner's instance: wavefronts of both
    widths in one launch, groups with different L1 in one wavefront, an idle last group.  All launches of a mode share one
    scratch (each starts on what the one before left in both planes)."""
    _set_mode(monkeypatch, mode)
    launches = _edge_launches(oracle)
    assert len(launches) == len(INSTANCES) * 2 * len(THS)
    _check_all(oracle, pair_raw.run(tmp_path, launches, timeout=300))


# ---- posteriors at their extremes ---------------------------------------------------------------------------------
def _extreme_launches(oracle):
    """identical sequences: every diagonal cell is an entry with v clipped at 0, so one lane has records in long runs of
    consecutive rows; sequences of N only: flat posteriors, at th = 0.002 nearly every lane-step is a candidate and, on
    the W = 2 instances, a lane's list holds fewer records than it has steps: the lists overflow and the wavefront takes
    the classic path"""
    launches = []
    same = [_rand(n, 900 + n) for n in (17, 31, 17, 31, 9, 9)]
    same_tasks = [(0, 2), (1, 3), (3, 1), (4, 5), (2, 0)]
    assert all(same[x] == same[y] for x, y in same_tasks)
    flat = ["N" * n for n in (12, 16, 20, 14, 18, 60)]
    flat_tasks = [(x, y) for x in range(6) for y in range(5) if x != y]  # the long one gives rows only: every instance takes it
    assert len(flat_tasks) == 25
    for inst in ((16, 2), (32, 2), (64, 1), (16, 3), None):
        for th in (0.002, 0.01, 0.3):
            launches.append(pair_raw.spec(oracle, 0, th, same, same_tasks, FILL if not launches else "keep", force=inst))
            launches.append(pair_raw.spec(oracle, 0, th, flat, flat_tasks, "keep", force=inst))
    # What fills the lists: 60 rows against 12 columns of N at th = 0.002.  The lane that owns a column has a candidate record
    # for every entry of that column at least, and at up to two columns per lane a record is 16 bytes, so its list holds
    # (max_len1 + G) * W / 4 records: fewer than the column's entries on the three narrow instances.
    most = int(np.bincount(pair_raw.want(oracle, flat[5], flat[0], 0.002, 0)[1]).max())
    for g, w in ((16, 2), (32, 2), (64, 1)):
        assert most > (60 + g) * w // 4, (g, w, most)
    return launches


def _per_pair(out):
    """what a launch left, per task, independent of where the pool allocator put the pair"""
    res, rpo = [], 0
    for p, (x, y) in enumerate(out["spec"]["tasks"]):
        n = len(out["spec"]["seqs"][x]) + len(out["spec"]["seqs"][y]) + 2
        o, k = int(out["pair_off"][p]), int(out["pair_nnz"][p])
        res.append((out["rowptr"][rpo:rpo + n].tobytes(), out["col"][o:o + 2 * k].tobytes(), out["val"][o:o + 2 * k].tobytes(),
                    k, out["sim"][p:p + 1].tobytes()))
        rpo += n
    return res


_EXTREME = {}  # mode -> what its launches left, per pair: each mode runs once


def _extreme(oracle, tmp_path, monkeypatch, mode):
    if mode not in _EXTREME:
        _set_mode(monkeypatch, mode)
        d = tmp_path / mode
        d.mkdir()
        outs = pair_raw.run(d, _extreme_launches(oracle), timeout=300)
        _check_all(oracle, outs)
        _EXTREME[mode] = [_per_pair(o) for o in outs]
    return _EXTREME[mode]


@pytest.mark.parametrize("mode", ["classic", "margin0", "margin1024"])
def test_modes_agree(oracle, tmp_path, monkeypatch, mode):
    """identical sequences and sequences of N only: every mode equal to the oracle, and the launches of the classic path,
    of the forced fallback and of the wide margin equal to the default ones pair by pair"""
    assert _extreme(oracle, tmp_path, monkeypatch, mode) == _extreme(oracle, tmp_path, monkeypatch, "default"), mode


# ---- persistent wavefronts ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group,mode", [(16, "default"), (64, "default"), (32, "margin1024"), (16, "margin0")])
def test_rounds_on_four_wavefronts(oracle, tmp_path, monkeypatch, group, mode):
    """65 tasks of 1 .. 70 residues on nwaves = 4: 17, 33 or 65 batches of different lengths on four wavefronts, and three
    launches on one scratch.  When a wavefront's next forward sweep starts, plane 0 holds the final records of its last
    batch and plane 1 that batch's candidate records (longer lists than the next pair's where the order descends); the
    first launch starts on 1.0 in both planes.  Compared per pair with the oracle."""
    _set_mode(monkeypatch, mode)
    launches = [pair_raw.spec(oracle, 0, th, SEQS, ORDERS[order], fill, nwaves=4)
                for th, order, fill in ((0.01, "descending", FILL), (0.002, "shuffled", "keep"), (0.01, "ascending", "keep"))]
    nbatches = -(-len(ORDERS["descending"]) // (64 // group))
    assert nbatches >= 4 * 4 + 1  # some wavefront takes at least five batches, and all four together at least nine
    outs = pair_raw.run(tmp_path, launches, env={"DAFS_HIP_FORCE_GROUP": group})
    for out in outs:
        g = pair_raw.geometry(out)
        assert g["group"] == group and g["nwaves"] == 4, g
        pair_raw.check(oracle, out, SEQS, out["spec"]["tasks"], out["spec"]["th"], 0)
