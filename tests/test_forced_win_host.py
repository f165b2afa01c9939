"""CPU: the host definition of forced wins by continuous fours (alpha_omok_amd.utils.forced_win) on hand-made positions and
on the fixture the device is compared with, the fast form of its two inner questions (utils.WindowPosition) against
utils.check_win / utils.win_cells, and the declaration of the entry point. Integer results: every comparison is exact.

Fixture: seeded uniformly random legal games -- np.random.RandomState(2000 + B), one permutation of the cells per game, cut
at the first terminal position -- every prefix of every game, searched with max_depth 6 and max_nodes 2000. Per board /
win_mark / games, the host gives (positions; positions of depth 1..6; budget exhausted; nodes):
    3/3/16   139   40  3 10  0  0  0   0    1425
    5/4/32   659  163 53 20 13  5  3   0    6321
    6/4/32   808  252 109 37 23 17 5   0    7826
    8/5/32  1587  399 155 37 16 16 4   1   20702
    9/5/32  1866  554 162 50  6 10 2   7   45211
   12/5/8    605  185 96  3  2  1  2   0    5568
   15/5/8    826  279 116 8  0  0  0   5   17030
The results are recorded in tests/golden/forced_win_fixture.npz (written by `python tests/test_forced_win_host.py`), which
the device test reads instead of searching again; test_fixture_conditions_and_golden holds the file to the live host."""
import functools
import os
import re

import numpy as np
import pytest

from conftest import REPO
from test_tactics_host import board_of, legal_id

GOLDEN = os.path.join(REPO, "tests", "golden", "forced_win_fixture.npz")
CASES = ((3, 3, 16), (5, 4, 32), (6, 4, 32), (8, 5, 32), (9, 5, 32), (12, 5, 8), (15, 5, 8))   # board, win_mark, games
MARK = {B: k for B, k, _ in CASES}
DEPTH, NODES, SMALL_NODES = 6, 2000, 50
# positions of depth 1..6 and with the budget exhausted, as the issue's prototype counted them
PROTOTYPE = {5: ([163, 53, 20, 13, 5, 3], 0), 6: ([252, 109, 37, 23, 17, 5], 0), 8: ([399, 155, 37, 16, 16, 4], 1),
             9: ([554, 162, 50, 6, 10, 2], 7), 12: ([185, 96, 3, 2, 1, 2], 0), 15: ([279, 116, 8, 0, 0, 0], 5)}
KEYS = ("result", "depth", "move", "moves", "line", "line_len", "nodes", "status", "turn")


def games_of(B, k, n):
    from alpha_omok_amd import utils
    rs = np.random.RandomState(2000 + B)
    games = []
    for _ in range(n):
        perm = rs.permutation(B * B).tolist()
        after = np.stack([utils.get_board([0] + perm[:t + 1], B) for t in range(B * B)])
        end = int(np.flatnonzero(utils.check_win_boards(after, k))[0])       # (the full board is terminal at the latest)
        games.append(perm[:end + 1])
    return games


def ids_of(B):
    """every prefix of every game of board B, the terminal one included, as reference-style ids"""
    k, n = [(k, n) for b, k, n in CASES if b == B][0]
    return [(0,) + tuple(g[:t]) for g in games_of(B, k, n) for t in range(len(g) + 1)]


def as_arrays(results, A, max_depth):
    """a list of utils.forced_win dicts as the arrays PositionBatch.forced_wins returns"""
    n = len(results)
    out = {key: np.array([r[key] for r in results], np.int32).reshape(n) for key in ("result", "depth", "move", "nodes", "status", "turn")}
    out["moves"] = np.array([r["moves"] for r in results], np.uint8).reshape(n, A)
    out["line"] = np.full((n, 2 * max_depth - 1), -1, np.int16)
    for i, r in enumerate(results):
        out["line"][i, :len(r["line"])] = r["line"]
    out["line_len"] = np.array([len(r["line"]) for r in results], np.int32).reshape(n)
    return out


@functools.lru_cache(maxsize=None)
def host_fixture():
    """Per board: the ids, utils.forced_win of each as arrays, the search statistics and which positions run out of
    SMALL_NODES nodes -- computed once; the fixture conditions are asserted here."""
    from alpha_omok_amd import utils
    fx = {}
    deep = np.zeros(7, np.int64)
    unknown = block_fours = multi_reply = 0
    for B, k, _ in CASES:
        ids = ids_of(B)
        res = [utils.forced_win(rid[1:], B, k, DEPTH, NODES) for rid in ids]
        arr = as_arrays(res, B * B, DEPTH)
        small = [utils.forced_win(rid[1:], B, k, DEPTH, SMALL_NODES) for rid in ids]
        arr["small_unknown"] = np.array([r["result"] == utils.FW_UNKNOWN for r in small], np.uint8)
        # the budget only cuts a search short: one that needs no more than SMALL_NODES nodes is the same search
        for r, s in zip(res, small):
            cut = r["result"] == utils.FW_UNKNOWN or r["nodes"] > SMALL_NODES
            assert (s["result"] == utils.FW_UNKNOWN) == cut
            if not cut:
                assert all(np.array_equal(r[key], s[key]) for key in KEYS)
        depth = np.bincount(arr["depth"][arr["result"] == 1], minlength=7)
        if B in PROTOTYPE:
            assert (depth[1:].tolist(), int((arr["result"] == 2).sum())) == PROTOTYPE[B], B
            assert depth[1] >= 1 and depth[2] >= 1 and depth[3] >= 1, B
            assert ((arr["result"] == 0) & (arr["status"] == 0)).any(), B
        deep += depth[:7]
        unknown += int((arr["result"] == 2).sum())
        block_fours += sum(r["stats"]["block_fours"] for r in res)
        multi_reply += sum(r["stats"]["multi_reply"] for r in res)
        fx[B] = dict(ids=ids, **arr)
    assert deep[4] >= 1 and deep[5] >= 1 and deep[6] >= 1, deep
    assert unknown >= 1 and block_fours >= 1 and multi_reply >= 1, (unknown, block_fours, multi_reply)
    return fx


def golden_fixture():
    """The recorded host results per board (with the ids, which are cheap to make again)."""
    with np.load(GOLDEN) as z:
        fx = {}
        for B, _, _ in CASES:
            d = {key: z["b%d_%s" % (B, key)] for key in KEYS + ("small_unknown",)}
            d["moves"] = np.unpackbits(d["moves"], axis=1, count=B * B)
            d["ids"] = ids_of(B)
            fx[B] = d
    return fx


def write_golden():
    fx = host_fixture()
    out = {}
    for B, d in fx.items():
        for key in KEYS + ("small_unknown",):
            out["b%d_%s" % (B, key)] = np.packbits(d[key], axis=1) if key == "moves" else d[key]
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    np.savez_compressed(GOLDEN, **out)


# ---------------------------------------------------------------------------------------------------------------------
# hand-made positions, 9x9, win_mark 5
# ---------------------------------------------------------------------------------------------------------------------
def cell(r, c):
    return r * 9 + c


def hand_made():
    """name -> (id, expected result, depth, winning first moves, line, nodes or None) with max_depth 4, max_nodes 2000"""
    out = {}
    # an open three; either end makes an open four (two replies, each loses to the other end): 2 moves. The stones next to
    # the far ends make closed fours with one reply, which lead nowhere. Nodes: 1 (D = 1) + 1 + the replies 1 + 2 + 2 + 1.
    b = board_of(9, black=[(4, 2), (4, 3), (4, 4)], white=[(0, 0), (0, 8), (8, 0)])
    out["open three"] = (legal_id(b, 0), 1, 2, [cell(4, 1), cell(4, 5)], [cell(4, 1), cell(4, 0), cell(4, 5)], 8)
    # a closed three in row 2 and two stones in column 4: the four on (2, 4) forces (2, 5) and makes column 4 an open
    # three, whose four on (1, 4) has two replies: 3 moves
    black = [(2, 1), (2, 2), (2, 3), (3, 4), (4, 4)]
    b = board_of(9, black=black, white=[(2, 0), (8, 0), (8, 2), (8, 6), (8, 8)])
    out["four-four chain"] = (legal_id(b, 0), 1, 3, [cell(2, 4)],
                              [cell(2, 4), cell(2, 5), cell(1, 4), cell(0, 4), cell(5, 4)], None)
    # the same chain, but the forced block on (2, 5) gives the defender an open four in column 5: two cells to answer
    b = board_of(9, black=black, white=[(2, 0), (3, 5), (4, 5), (5, 5), (8, 0)])
    out["the block makes a four"] = (legal_id(b, 0), 0, 0, [], [], None)
    # the same chain, but the defender already has a four: its winning cell is the attacker's only candidate (any other
    # stone would leave `his` not empty), and a stone there makes no four
    b = board_of(9, black=black, white=[(2, 0), (6, 5), (6, 6), (6, 7), (6, 8)])
    out["the defender wins first"] = (legal_id(b, 0), 0, 0, [], [], 4)
    # two cells to answer at the root: every iteration ends at the root
    b = board_of(9, black=black + [(8, 8)], white=[(2, 0), (6, 3), (6, 4), (6, 5), (6, 6), (0, 8)])
    out["two threats at the root"] = (legal_id(b, 0), 0, 0, [], [], 4)
    # a terminal root: white's five; black's chain no longer counts
    b = board_of(9, black=black + [(8, 8)], white=[(2, 0), (6, 3), (6, 4), (6, 5), (6, 6), (6, 7)])
    out["terminal root"] = (legal_id(b, 0), 0, 0, [], [], 4)
    return out


def test_hand_made_positions():
    from alpha_omok_amd import utils
    for name, (rid, result, depth, moves, line, nodes) in hand_made().items():
        r = utils.forced_win(rid[1:], 9, 5, 4, 2000)
        lit = utils.forced_win(rid[1:], 9, 5, 4, 2000, position=utils.ArrayPosition)
        for key in KEYS + ("stats",):
            assert np.array_equal(r[key], lit[key]), (name, key)
        assert (r["result"], r["depth"], np.flatnonzero(r["moves"]).tolist(), r["line"]) == (result, depth, moves, line), name
        assert r["move"] == (moves[0] if moves else -1) and r["turn"] == 0, name
        if nodes is not None:
            assert r["nodes"] == nodes, name
    assert utils.forced_win(hand_made()["terminal root"][0][1:], 9, 5)["status"] == 2
    # the chain is found at depth 3 exactly: max_depth 2 does not see it
    chain = hand_made()["four-four chain"][0]
    assert utils.forced_win(chain[1:], 9, 5, 2, 2000)["result"] == 0
    # the budget: the call number max_nodes + 1 makes it unknown, with nothing of the search left
    full = utils.forced_win(chain[1:], 9, 5, 4, 2000)
    r = utils.forced_win(chain[1:], 9, 5, 4, full["nodes"])
    assert all(np.array_equal(r[key], full[key]) for key in KEYS)
    r = utils.forced_win(chain[1:], 9, 5, 4, full["nodes"] - 1)
    assert (r["result"], r["depth"], r["move"], r["line"], r["nodes"]) == (2, 0, -1, [], full["nodes"] - 1) and not r["moves"].any()


def test_the_defenders_winning_cell_is_the_only_candidate():
    """`his` of the definition: a stone anywhere but on the defender's winning cell leaves it, so the search never makes
    such a four -- the position's other fours exist (the chain's first move is one without the defender's four)."""
    from alpha_omok_amd import utils
    rid = hand_made()["the defender wins first"][0]
    pos = utils.WindowPosition(9, 5)
    for t, m in enumerate(rid[1:]):
        pos.place(m, t % 2)
    mine, theirs = pos.win_cells(0)
    assert mine == [] and theirs == [cell(6, 4)]
    pos.place(cell(2, 4), 0)                    # the chain's four
    his, replies = pos.win_cells(1)
    assert his == [cell(6, 4)] and replies == [cell(2, 5)]


def test_full_board_draw_and_empty_board():
    from alpha_omok_amd import utils
    draw = [0, 1, 2, 4, 3, 5, 7, 6, 8]                                         # X O X / X O O / O X X
    r = utils.forced_win(draw, 3, 3, 5, 100)
    assert (r["result"], r["status"], r["nodes"], r["move"], r["line"]) == (0, 3, 5, -1, [])
    r = utils.forced_win(draw[:8], 3, 3, 5, 100)                               # the last cell only fills the board
    assert (r["result"], r["status"], r["nodes"]) == (0, 0, 5)
    r = utils.forced_win([], 9, 5, 3, 100)
    assert (r["result"], r["nodes"], r["turn"]) == (0, 3, 0)


def test_window_position_is_check_win_and_win_cells():
    """The fast form of the two inner questions against utils.check_win / utils.win_cells: every fixture position of the
    3x3, 5x5 and 6x6 boards, every seventh of the others."""
    from alpha_omok_amd import utils
    for B, k, _ in CASES:
        ids = ids_of(B)
        for rid in ids if B <= 6 else ids[::7]:
            pos = utils.WindowPosition(B, k)
            for t, m in enumerate(rid[1:]):
                pos.place(m, t % 2)
            board, turn = utils.get_board(rid, B), (len(rid) - 1) % 2
            assert pos.terminal() == (utils.check_win(board, k) != 0), rid
            mine, theirs = utils.win_cells(board, turn, k)
            assert pos.win_cells(turn) == (np.flatnonzero(mine).tolist(), np.flatnonzero(theirs).tolist()), rid
            assert pos.win_cells(1 - turn) == (np.flatnonzero(theirs).tolist(), np.flatnonzero(mine).tolist()), rid
            if len(rid) > 1:                                                   # and stones go as they came
                pos.remove(rid[-1], (len(rid) - 2) % 2)
                prev = utils.WindowPosition(B, k)
                for t, m in enumerate(rid[1:-1]):
                    prev.place(m, t % 2)
                assert np.array_equal(pos.code, prev.code) and np.array_equal(pos.board, prev.board) and pos.stones == prev.stones


def test_forced_win_with_the_literal_questions_on_small_boards():
    """the whole search with utils.check_win / utils.win_cells asked literally, on every 3x3 position and every fifth 5x5 one"""
    from alpha_omok_amd import utils
    for B, ids in ((3, ids_of(3)), (5, ids_of(5)[::5])):
        for rid in ids:
            r = utils.forced_win(rid[1:], B, MARK[B], DEPTH, NODES)
            lit = utils.forced_win(rid[1:], B, MARK[B], DEPTH, NODES, position=utils.ArrayPosition)
            for key in KEYS + ("stats",):
                assert np.array_equal(r[key], lit[key]), (rid, key)


def test_fixture_conditions_and_golden():
    fx = host_fixture()                                                        # asserts the conditions
    gold = golden_fixture()
    for B, _, _ in CASES:
        assert gold[B]["ids"] == fx[B]["ids"]
        for key in KEYS + ("small_unknown",):
            np.testing.assert_array_equal(gold[B][key], fx[B][key], err_msg="%d %s" % (B, key))


def test_lines_of_the_fixture_are_forced_wins():
    """For every result-1 position: replaying `line` is legal; every attacker stone but the last leaves `replies` not empty
    and `his` empty; every defender stone is one of `replies`; check_win is the attacker's index after the last stone and
    0 before. The first stone is min(moves), the line is no longer than 2 depth - 1."""
    from alpha_omok_amd import utils
    fx = host_fixture()
    checked = 0
    for B, k, _ in CASES:
        d = fx[B]
        for i in np.flatnonzero(d["result"] == 1):
            rid, a = d["ids"][i], int(d["turn"][i])
            line = d["line"][i, :d["line_len"][i]].tolist()
            assert 1 <= len(line) <= 2 * d["depth"][i] - 1 and len(line) % 2 == 1
            assert line[0] == d["move"][i] == np.flatnonzero(d["moves"][i])[0]
            assert (d["line"][i, len(line):] == -1).all()
            pos = utils.WindowPosition(B, k)
            for t, m in enumerate(rid[1:]):
                pos.place(m, t % 2)
            boards = []
            for j, m in enumerate(line):
                assert pos.board[m] == 0, (rid, line)
                if j % 2 == 1:
                    assert m in replies, (rid, line)
                pos.place(m, a if j % 2 == 0 else 1 - a)
                boards.append(pos.board.reshape(B, B).copy())
                if j % 2 == 0 and j < len(line) - 1:
                    his, replies = pos.win_cells(1 - a)
                    assert his == [] and replies != [], (rid, line)
            status = utils.check_win_boards(np.stack(boards), k)
            assert status[-1] == a + 1 and not status[:-1].any() and d["status"][i] == 0, (rid, line)
            checked += 1
    assert checked > 2000


# ---------------------------------------------------------------------------------------------------------------------
# declarations and argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_entry_point():
    from alpha_omok_amd import _lib, build, evaluate, positions, utils
    from alpha_omok_amd.agents import ZeroAgent
    hdr = open(os.path.join(REPO, "include", "omok_hip.h")).read()
    name, nargs = "ao_positions_forced_wins", 17
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert m, "omok_hip.h does not declare %s" % name
    assert len(m.group(1).split(",")) == nargs
    assert len(_lib.SYMBOLS[name][1]) == nargs
    assert "utils.py:30-59" in hdr[:m.start()].rsplit("/*", 1)[1]
    assert "positions.hip" in build.SOURCES and sorted(build.SOURCES) == sorted(f for f in os.listdir(build.CSRC) if f.endswith(".hip"))
    assert sorted(h for h in build.HEADERS if not os.path.isabs(h)) == sorted(f for f in os.listdir(build.CSRC) if f.endswith(".hpp"))
    build.build()
    lib = _lib.load(build_if_missing=False)
    assert hasattr(lib, name), "libomok_hip.so does not export %s" % name
    assert lib.ao_abi_version() == 2          # additive change
    assert (positions.FW_NONE, positions.FW_WIN, positions.FW_UNKNOWN) == (utils.FW_NONE, utils.FW_WIN, utils.FW_UNKNOWN) == (0, 1, 2)
    assert (positions.FW_MAX_DEPTH, positions.FW_MAX_NODES) == (utils.FW_MAX_DEPTH, utils.FW_MAX_NODES) == (16, 65536)
    assert callable(positions.PositionBatch.forced_wins) and callable(ZeroAgent.get_forced_win) and callable(evaluate.forced_win_summary)


def test_arguments_are_checked_before_touching_the_device():
    from alpha_omok_amd import utils
    from alpha_omok_amd.positions import PositionBatch

    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError("device call %s before validation" % name)

    pb = PositionBatch.__new__(PositionBatch)
    pb._h, pb._L, pb._evaluator = None, NoDevice(), None
    pb.board_size, pb.inplanes, pb.win_mark, pb.capacity, pb.device, pb.A = 9, 5, 5, 16, 0, 81
    for kw in (dict(max_depth=0), dict(max_depth=17), dict(max_nodes=0), dict(max_nodes=65537), dict(max_depth=2.0), dict(max_nodes=True)):
        with pytest.raises(ValueError):
            pb.forced_wins([(0, 1, 2)], **kw)
        with pytest.raises(ValueError):
            utils.forced_win([1, 2], 9, 5, **kw)
    for bad in ([(1, 2)], [(0, 1.5)]):                                         # lacks the leading 0; not an integer
        with pytest.raises(ValueError):
            pb.forced_wins(bad)
    for bad in ([3, 3], [81], [-1], list(range(81)) + [0]):
        with pytest.raises(ValueError):
            utils.forced_win(bad, 9, 5)
    assert utils.forced_win([1, 2], 9, 5, 16, 65536)["result"] == 0            # the limits themselves are fine


if __name__ == "__main__":
    write_golden()
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
