"""CPU: the host definition of the solver's verdict on a root position (alpha_omok_amd.utils.root_tactics), the host
definition of the root move restriction (utils.root_bar / check_allowed) and the declarations of the two entry points.
Integer results: every comparison is exact, `nodes` and `unknown` included.

root_tactics goes through forced_win alone, like forced_defences, so most of what it says about the fixture of
test_forced_defence_host (every prefix of its games, depth 6, 2000 nodes; 9x9 also with 50 nodes) is in
tests/golden/forced_defence_fixture.npz already: the threat and every reply. `expected` puts the verdict together from those
recorded rows and two live searches per position (the mover's own, and the opponent's for its node count); the live
utils.root_tactics is held to it on every 3x3 and 5x5 position and on every STEP-th of the larger boards, and the device test
reads `expected` instead of searching again. Verdicts of the open positions at depth 6 / 2000 nodes, where no search of an
open position runs out of nodes:

    board   NONE  DEFEND  WIN  LOST
     3x3       6      10   10     4
     5x5      39      23   59    11
     6x6      22      18   68     8
     8x8      73      22   68    33
     9x9     109      21   75    11
   15x15      31       1   46    25
"""
import functools
import os
import re

import numpy as np
import pytest

from conftest import REPO
from test_forced_defence_host import CASES, DEPTH, MARK, NODES, SMALL_BOARD, SMALL_NODES, STEP, _golden, ids_of

VERDICTS = {3: (6, 10, 10, 4), 5: (39, 23, 59, 11), 6: (22, 18, 68, 8), 8: (73, 22, 68, 33), 9: (109, 21, 75, 11),
            15: (31, 1, 46, 25)}       # NONE, DEFEND, WIN, LOST
KEYS = ("verdict", "depth", "allowed", "nodes", "unknown")
NEW_SYMBOLS = {"ao_set_root_bar": 2, "ao_root_tactics": 10}      # name -> arguments
KEPT_SYMBOLS = {"ao_begin_move_opts": 4, "ao_search_opts": 11}   # their signatures stay

# NCH = 3: a 12x12 game with a four. Black builds 63 64 65 66 67 along row 5 while white plays along row 0 and blocks once;
# the prefixes of 3 .. 8 moves hold an open three to answer (RT_DEFEND), a forced win (RT_WIN) and an open four (RT_LOST)
NCH3_BOARD, NCH3_MARK = 12, 5
NCH3_GAME = (63, 0, 64, 2, 65, 4, 66, 62, 67)


def nch3_ids():
    return [(0,) + NCH3_GAME[:t] for t in range(3, 9)]


def as_arrays(results, A):
    """a list of utils.root_tactics dicts as the arrays Engine.root_tactics returns"""
    n = len(results)
    out = {key: np.array([r[key] for r in results], np.int32).reshape(n) for key in ("verdict", "depth", "nodes", "unknown")}
    out["allowed"] = np.array([r["allowed"] for r in results], bool).reshape(n, A)
    return out


def host_rows(B, ids, max_nodes=NODES, max_depth=DEPTH, win_mark=None):
    from alpha_omok_amd import utils
    k = MARK[B] if win_mark is None else win_mark
    return as_arrays([utils.root_tactics(rid[1:], B, k, max_depth, max_nodes) for rid in ids], B * B)


@functools.lru_cache(maxsize=None)
def expected(B, small=False):
    """utils.root_tactics of every fixture position of board B by its own rules, with the threat and the replies taken from
    the recorded forced_defences rows: (ids, arrays)."""
    from alpha_omok_amd import utils
    g = _golden()[B]
    ids, A, nodes = g["ids"], B * B, SMALL_NODES if small else NODES
    if small:
        g = g["small"]
    rows = []
    for i, rid in enumerate(ids):
        mv = list(rid[1:])
        r = dict(verdict=utils.RT_NONE, depth=0, allowed=np.zeros(A, bool), nodes=0, unknown=0)
        rows.append(r)
        if g["status"][i] != 0:
            continue
        own = utils.forced_win(mv, B, MARK[B], DEPTH, nodes)
        r["nodes"] = own["nodes"]
        if own["result"] == utils.FW_WIN:
            r.update(verdict=utils.RT_WIN, depth=own["depth"], allowed=own["moves"])
            continue
        r["unknown"] = int(own["result"] == utils.FW_UNKNOWN) | 2 * int(g["threat"][i] == utils.FW_UNKNOWN)
        r["allowed"] = g["reply"][i] != utils.FD_NONE
        if g["threat"][i] != utils.FW_WIN:
            r["nodes"] += utils.forced_win(mv, B, MARK[B], DEPTH, nodes, attacker=1 - len(mv) % 2)["nodes"]
            continue
        r["nodes"] += int(g["nodes"][i])
        r["unknown"] |= 4 * int((g["reply"][i] == utils.FD_UNKNOWN).any())
        r["depth"] = int(g["threat_depth"][i])
        holds = (g["reply"][i] == utils.FD_SAFE) | (g["reply"][i] == utils.FD_UNKNOWN)
        if holds.any():
            r.update(verdict=utils.RT_DEFEND, allowed=holds)
        else:
            r["verdict"] = utils.RT_LOST
    return ids, as_arrays(rows, A)


def sample(B, n):
    """the positions the live host is asked about: all of them on 3x3 and 5x5, every STEP-th from 6x6 up"""
    return list(range(n)) if B <= 5 else list(range(0, n, STEP))


def assert_rows_equal(got, want, rows, tag):
    for key in KEYS:
        np.testing.assert_array_equal(got[key], want[key][rows], err_msg="%s: %s" % (tag, key))


@pytest.mark.parametrize("B", [b for b, _, _ in CASES])
def test_every_verdict_on_every_board(B):
    """The fixture holds all four verdicts on every board, no search of an open position runs out of nodes at 2000, and where
    the verdict is RT_DEFEND `allowed` is reply != FD_LOSES of the recorded rows (on its empty cells)."""
    from alpha_omok_amd import utils
    ids, e = expected(B)
    g = _golden()[B]
    live = g["status"] == 0
    counts = tuple(int(((e["verdict"] == v) & live).sum()) for v in (utils.RT_NONE, utils.RT_DEFEND, utils.RT_WIN, utils.RT_LOST))
    print("board %d: NONE %d, DEFEND %d, WIN %d, LOST %d" % ((B,) + counts))
    assert all(c > 0 for c in counts), counts
    assert counts == VERDICTS[B]
    assert (e["unknown"] == 0).all()
    assert (e["verdict"][~live] == utils.RT_NONE).all() and not e["allowed"][~live].any() and (e["nodes"][~live] == 0).all()
    d = e["verdict"] == utils.RT_DEFEND
    np.testing.assert_array_equal(e["allowed"][d], (g["reply"][d] != utils.FD_LOSES) & (g["reply"][d] != utils.FD_NONE))
    w = e["verdict"] == utils.RT_WIN
    assert (e["depth"][w] >= 1).all() and e["allowed"][w].any(axis=1).all()
    for i in np.flatnonzero(live & ~w & ~d):                   # NONE and LOST: every empty cell
        empty = np.ones(B * B, bool)
        empty[list(ids[i][1:])] = False
        np.testing.assert_array_equal(e["allowed"][i], empty)


@pytest.mark.parametrize("B", [b for b, _, _ in CASES])
def test_live_host_is_the_expected(B):
    ids, e = expected(B)
    rows = sample(B, len(ids))
    assert_rows_equal(host_rows(B, [ids[i] for i in rows]), e, rows, "board %d" % B)


def test_small_budget_unknown_bits():
    """9x9 at 50 nodes: searches run out. Every unknown bit occurs, a reply whose search ran out stays allowed, and the live
    host equals the rows put together from the recorded ones."""
    from alpha_omok_amd import utils
    B = SMALL_BOARD
    ids, e = expected(B, small=True)
    g = _golden()[B]["small"]
    for bit in (1, 2, 4):
        assert (e["unknown"] & bit).any(), "no position with unknown bit %d" % bit
    d = np.flatnonzero((e["verdict"] == utils.RT_DEFEND) & (e["unknown"] & 4 != 0))
    assert d.size > 0
    for i in d:
        ran_out = g["reply"][i] == utils.FD_UNKNOWN
        assert ran_out.any() and e["allowed"][i][ran_out].all()
    rows = sorted(set(sample(B, len(ids))) | set(d[:3].tolist()))
    assert_rows_equal(host_rows(B, [ids[i] for i in rows], SMALL_NODES), e, rows, "9x9 at %d nodes" % SMALL_NODES)


def test_nch3_game_holds_a_win_and_a_defence():
    from alpha_omok_amd import utils
    r = host_rows(NCH3_BOARD, nch3_ids(), 512, 6, NCH3_MARK)
    assert len(nch3_ids()) == 6
    assert (r["verdict"] == utils.RT_WIN).any() and (r["verdict"] == utils.RT_DEFEND).any()
    assert r["verdict"].tolist() == [utils.RT_NONE, utils.RT_NONE, utils.RT_DEFEND, utils.RT_WIN, utils.RT_LOST, utils.RT_WIN]
    assert r["allowed"][3, 66] and r["allowed"][3, 62] and r["allowed"][3].sum() == 2      # the open three: either end makes the open four
    assert r["allowed"][2, [62, 66]].all() and not r["allowed"][2, 100]                      # ... and the defender takes one of them
    assert r["allowed"][5].tolist() == [c == 67 for c in range(144)]                        # the four: the one cell that wins


def test_terminal_empty_and_full_boards():
    from alpha_omok_amd import utils
    A = 9
    r = utils.root_tactics([], 3, 3)                                                         # the empty board: nothing proven
    assert (r["verdict"], r["depth"], r["unknown"]) == (utils.RT_NONE, 0, 0) and r["allowed"].all() and r["nodes"] > 0
    won = utils.root_tactics([0, 3, 1, 4, 2], 3, 3)                                          # black has the top row
    full = utils.root_tactics([0, 1, 2, 4, 3, 5, 7, 6, 8], 3, 3)                             # a full board, nobody won
    for t in (won, full):
        assert (t["verdict"], t["depth"], t["nodes"], t["unknown"]) == (utils.RT_NONE, 0, 0, 0) and not t["allowed"].any()
    one = utils.root_tactics([0, 1, 2, 4, 3, 5, 7, 6], 3, 3)                                 # one empty cell left, no line to make
    assert one["verdict"] == utils.RT_NONE and one["allowed"].tolist() == [c == 8 for c in range(A)]


def test_argument_errors():
    from alpha_omok_amd import utils
    from alpha_omok_amd.positions import _check_limits
    for bad in (dict(max_depth=0), dict(max_depth=17), dict(max_nodes=0), dict(max_nodes=65537), dict(max_depth=True),
                dict(max_nodes=2.5)):
        with pytest.raises(ValueError):
            utils.root_tactics([4], 3, 3, **bad)
        with pytest.raises(ValueError):                                                      # what Engine.root_tactics asks before any device call
            _check_limits(bad.get("max_depth", 6), bad.get("max_nodes", 512))
    for moves in ([9], [-1], [4, 4]):
        with pytest.raises(ValueError):
            utils.root_tactics(moves, 3, 3)


def test_header_and_binding_declare_the_entry_points():
    from alpha_omok_amd import _lib, engine
    hdr = open(os.path.join(REPO, "include", "omok_hip.h")).read()
    for name, nargs in list(NEW_SYMBOLS.items()) + list(KEPT_SYMBOLS.items()):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, hdr)
        assert m, "omok_hip.h does not declare %s" % name
        assert len(m.group(1).split(",")) == nargs, name
        assert name in _lib.SYMBOLS, "_lib.SYMBOLS lacks %s" % name
        assert len(_lib.SYMBOLS[name][1]) == nargs
    assert "utils.root_tactics" in hdr                                                       # the header cites the host definition
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
    assert lib.ao_abi_version() == 2                                                          # additive change
    m = re.search(r"#define\s+AO_BAR_Q\s+\(([^)]*)\)", hdr)
    assert m and float(np.float32(float(m.group(1).rstrip("f")))) == engine.BAR_Q
    assert np.isfinite(engine.BAR_Q) and engine.BAR_Q < -1e29
    from alpha_omok_amd import utils
    assert (engine.RT_NONE, engine.RT_WIN, engine.RT_DEFEND, engine.RT_LOST) == (utils.RT_NONE, utils.RT_WIN, utils.RT_DEFEND, utils.RT_LOST)
    for name in ("NONE", "WIN", "DEFEND", "LOST"):
        assert re.search(r"AO_RT_%s\s*=\s*%d" % (name, getattr(utils, "RT_" + name)), hdr)


def test_allowed_mask_validation():
    """shape, values, an all-barred row, ones on stones, a row that allows everything"""
    from alpha_omok_amd import utils
    ids = [(0,), (0, 4, 0), (0, 0, 1, 2, 3, 4, 5, 7, 6)]                                      # empty, two stones, one cell left (8)
    ok = np.ones((3, 9), np.uint8)
    assert utils.check_allowed(None, 3, 9) is None
    assert utils.check_allowed(ok.astype(bool), 3, 9).dtype == np.uint8
    for bad in (np.ones((2, 9), np.uint8), np.ones(9, np.uint8), np.ones((3, 8), np.uint8), np.full((3, 9), 2), np.ones((3, 9)) * 0.5):
        with pytest.raises(ValueError):
            utils.check_allowed(bad, 3, 9)
    assert not utils.root_bar(ok, ids, 3).any()                                               # every empty cell allowed: no restriction
    a = ok.copy()
    a[1] = 0
    a[1, [4, 0]] = 1                                                                          # ones on the two stones only
    with pytest.raises(ValueError, match="game 1"):
        utils.root_bar(a, ids, 3)
    a[1, 5] = 1
    bar = utils.root_bar(a, ids, 3)
    assert bar[1].tolist() == [c not in (0, 4, 5) for c in range(9)] and not bar[0].any() and not bar[2].any()
    a[2] = 0
    with pytest.raises(ValueError, match="game 2"):                                          # the one empty cell is barred
        utils.root_bar(a, ids, 3)
    a[2] = 1
    a[0] = 0
    with pytest.raises(ValueError, match="game 0"):
        utils.root_bar(a, ids, 3)
