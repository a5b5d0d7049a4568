"""CPU tests of the alignment-reliability annotation: the restatement of the definitions (tests/reliability_ref.py) on
hand-built stores with known answers, the PP characters, the Stockholm names and the Python Stockholm writer."""
import numpy as np

import reliability_ref as rr

NONE = rr.NONE


def _rows(*rows):
    return [(np.array(c, np.uint32), np.array(v, np.float32)) for c, v in rows]


def test_two_sequences_known_answers():
    # x = 0 (3 nt), y = 1 (2 nt); columns: x0 y0 | x1 - | x2 y1
    mask = np.array([[1, 1, 1], [1, 0, 1]], np.uint8)
    mp = {(0, 1): _rows(([0, 1], [0.5, 0.25]), ([1], [0.25]), ([1], [0.75])),
          (1, 0): _rows(([0], [0.5]), ([0, 1, 2], [0.25, 0.25, 0.75]))}
    mp_row, bp_row = rr.dict_stores(mp)
    got = rr.restate([0, 1], mask, None, mp_row, bp_row)
    # x0: mp(0,0) = 0.5; x1 opposite a gap: 1 - 0.25; x2: mp(2,1) = 0.75; y0: 0.5; y1: mp[y][x](1, 2) = 0.75
    assert got["residue"].tolist() == [0.5, 0.75, 0.75, 0.5, 0.75]
    assert got["col"].tolist() == [0.5, 0.75, 0.75]
    assert got["expected_accuracy"] == (0.5 + 0.75 + 0.75 + 0.5 + 0.75) / 5
    assert got["pair"].tolist() == [0.0, 0.0, 0.0] and got["pair_rows"].tolist() == [0, 0, 0]


def test_three_sequences_gaps_absent_entries_and_clipping():
    # rows 0, 1, 2 over 2 columns; row 2 has one residue in column 1
    mask = np.array([[1, 1], [1, 1], [0, 1]], np.uint8)
    mp = {(0, 1): _rows(([0], [0.875]), ([0], [0.125])),       # (1, 1) not stored
          (1, 0): _rows(([0, 1], [0.875, 0.125]), ((), ())),
          (0, 2): _rows(([0], [0.75]), ([0], [0.5])),
          (2, 0): _rows(([0, 1], [0.75, 0.5])),
          (1, 2): _rows(([0], [0.625]), ([0], [0.25])),
          (2, 1): _rows(([0, 1], [0.625, 0.25]))}
    mp_row, bp_row = rr.dict_stores(mp)
    got = rr.restate([0, 1, 2], mask, None, mp_row, bp_row)
    # row 0: i0 vs row1 j0 = 0.875, vs row2 gap: 1 - 0.75 -> (0.875 + 0.25) / 2; i1 vs row1 j1 (absent) 0, vs row2 j0 0.5 -> 0.25
    # row 1: i0 vs row0 0.875, vs gap 1 - 0.625; i1 vs row0 (1,1) absent 0, vs row2 0.25
    # row 2: i0 vs row0 (0,1) = 0.5, vs row1 (0,1) = 0.25; row mass of (2,0) row 0 is 1.25 > 1 (clipped, unused here)
    want = [(0.875 + 0.25) / 2, (0.0 + 0.5) / 2, (0.875 + (1.0 - 0.625)) / 2, (0.0 + 0.25) / 2, (0.5 + 0.25) / 2]
    assert got["residue"].tolist() == want
    assert got["col"][0] == (want[0] + want[2]) / 2
    assert got["col"][1] == ((want[1] + want[3]) + want[4]) / 3


def test_row_mass_above_one_is_clipped():
    mask = np.array([[1, 1], [1, 0]], np.uint8)
    mp = {(0, 1): _rows(([0], [0.75]), ([0], [0.5])),
          (1, 0): _rows(([0, 1], [0.75, 0.5]))}
    mp_row, bp_row = rr.dict_stores(mp)
    got = rr.restate([1, 0], mask[::-1], None, mp_row, bp_row)  # rows given in the other order
    # sequence 0 is the second given row: residue 1 sits opposite a gap; row mass 0.5 -> 0.5
    assert got["residue"].tolist() == [0.75, 0.75, 0.5]
    mp[(0, 1)] = _rows(([0], [0.75]), ([0, 1], [0.75, 0.5]))  # row mass 1.25
    got = rr.restate([1, 0], mask[::-1], None, mp_row, bp_row)
    assert got["residue"].tolist() == [0.75, 0.75, 0.0]


def test_single_sequence_and_pairs():
    mask = np.ones((1, 4), np.uint8)
    bp = {0: _rows(([3], [0.625]), ((), ()), ((), ()), ((), ()))}
    mp_row, bp_row = rr.dict_stores({}, bp)
    ss = np.array([3, NONE, NONE, NONE], np.uint32)
    got = rr.restate([0], mask, ss, mp_row, bp_row)
    assert got["residue"].tolist() == [1.0] * 4 and got["col"].tolist() == [1.0] * 4
    assert got["expected_accuracy"] == 1.0
    assert got["pair"].tolist() == [0.625, 0, 0, 0] and got["pair_rows"].tolist() == [1, 0, 0, 0]


def test_consensus_pairs_average_over_rows_holding_both():
    mask = np.array([[1, 1, 1], [1, 0, 1], [0, 1, 1]], np.uint8)
    mp = {}
    for x in range(3):
        for y in range(3):
            if x != y:
                mp[(x, y)] = [((), ())] * 3
    bp = {0: _rows(([2], [0.5]), ((), ()), ((), ())), 1: _rows(((), ()), ((), ())), 2: _rows(((), ()), ((), ()))}
    mp_row, bp_row = rr.dict_stores(mp, bp)
    got = rr.restate([0, 1, 2], mask, np.array([2, NONE, NONE], np.uint32), mp_row, bp_row)
    # rows 0 and 1 hold both residues of the pair (0, 2); row 1's (0, 1) is not stored
    assert got["pair"][0] == 0.25 and got["pair_rows"][0] == 2


def test_pp_characters():
    from dafs_amd import stockholm
    ps = [0.0, 0.04, 0.0499999, 0.05, 0.149, 0.15, 0.25, 0.45, 0.55, 0.75, 0.85, 0.94999, 0.95, 1.0]
    assert "".join(stockholm.pp_char(p) for p in ps) == "000112356899**"
    assert "".join(stockholm.pp_char(k / 100.0) for k in range(5, 100, 10)) == "123456789*"  # 0.05, 0.15, ..., 0.95
    assert "".join(stockholm.pp_char(k / 10.0) for k in range(10)) == "0123456789"


def test_names():
    from dafs_amd import stockholm
    assert stockholm.names(["a desc", "", "a", "  b\tx", "a other", " "]) == ["a", "seq2", "a.2", "b", "a.3", "seq6"]


def test_stockholm_writer_literal():
    from dafs_amd import stockholm
    rows = ["AC-G", "A-UG"]
    rel = [np.array([0.97, 0.5, 0.04]), np.array([0.96, 0.15, 0.25])]
    col = np.array([0.965, 0.5, 0.15, 0.145])
    got = stockholm.block("[ 0.5 s1 s2 ]", ["s1", "s2"], rows, rel, col, "(..)")
    want = ("# STOCKHOLM 1.0\n"
            "#=GF CC [ 0.5 s1 s2 ]\n"
            "s1           AC-G\n"
            "#=GR s1 PP   *5.0\n"
            "s2           A-UG\n"
            "#=GR s2 PP   *.23\n"
            "#=GC SS_cons (..)\n"
            "#=GC PP_cons *521\n"
            "//\n")
    assert got == want
    # a column without residues is '.' in PP_cons
    got = stockholm.block("x", ["a"], ["A-"], [np.array([0.5])], np.array([0.5, 0.0]), "..")
    assert got.split("\n")[-3] == "#=GC PP_cons 5."
