"""CPU: the host definition of leaf tactics (alpha_omok_amd.utils.leaf_tactics_value / leaf_tactics_evaluator: a leaf whose
mover has a proven forced win by continuous fours is valued exactly +1, every other leaf keeps the evaluator's value), the
declarations of the two entry points, and the conditions under which tests/test_gpu_leaf_tactics.py proves something --
asserted here with the oracle alone, so that nobody can run the device test on inputs that show nothing.

Roots (roots_of): per board, the ids of tests/golden/forced_win_fixture.npz with result 1, status 0, depth 2..4 and more than
three entries, their last two moves cut, the first 8 distinct ones: positions a move or two in front of a forced win, so the
leaves of a 24-simulation search keep running into proven wins. Game k is seeded 100 + k; 24 simulations, noise on, stub
B % 3, limits 4 / 64, win_mark from MARK."""
import os
import re

import numpy as np
import pytest

from conftest import REPO
from test_forced_win_host import MARK, golden_fixture, hand_made

BOARDS = (6, 9, 12, 15)
SIMS, DEPTH, NODES, GAMES, PLANES = 24, 4, 64, 8, 5
NEW_SYMBOLS = {"ao_set_leaf_tactics": 3, "ao_leaf_tactics_stats": 4}      # name -> arguments in include/omok_hip.h


def roots_of(B):
    d = golden_fixture()[B]
    out = []
    for i, rid in enumerate(d["ids"]):
        if d["result"][i] == 1 and d["status"][i] == 0 and 2 <= d["depth"][i] <= 4 and len(rid) > 3:
            root = tuple(rid[:-2])
            if root not in out:
                out.append(root)
                if len(out) == GAMES:
                    break
    assert len(out) == GAMES, (B, len(out))
    return out


def seeds_of(G=GAMES):
    return [100 + k for k in range(G)]


def stub_of(oracle, B):
    """the plain evaluator E(moves, planes, sim) of board B: the oracle's exact-arithmetic stub B % 3"""
    return lambda moves, planes, sim: oracle.stub_eval(planes, B % 3)


def counting_evaluator(evaluator, B, tally):
    """utils.leaf_tactics_evaluator around `evaluator`, counting into tally [4] what the device counts: the non-terminal
    leaves searched, those proven, those whose search ran out of nodes, and the solver's nodes (the oracle also evaluates
    terminal leaves; the device does not search those)."""
    from alpha_omok_amd import utils
    wm = MARK[B]
    inner = utils.leaf_tactics_evaluator(evaluator, B, wm, DEPTH, NODES)

    def f(moves, planes, sim):
        r = utils.forced_win(moves, B, wm, DEPTH, NODES)
        if r["status"] == 0:
            tally[:] += np.array([1, r["result"] == utils.FW_WIN, r["result"] == utils.FW_UNKNOWN, r["nodes"]], np.int64)
        return inner(moves, planes, sim)
    return f


def oracle_agent(oracle, B, seed, evaluator):
    ag = oracle.Agent(B, SIMS, PLANES, noise=True, evaluator=evaluator)
    ag.seed(seed)
    ag.set_win_mark(MARK[B])
    return ag


# ---------------------------------------------------------------------------------------------------------------------
# the two utils functions
# ---------------------------------------------------------------------------------------------------------------------
def test_a_proven_win_is_exactly_one_and_everything_else_is_left_alone():
    from alpha_omok_amd import utils
    hm = hand_made()
    v = np.float32(-0.4375)
    for name in ("open three", "four-four chain"):
        rid = hm[name][0]
        out = utils.leaf_tactics_value(rid[1:], 9, 5, v, 4, 2000)
        assert type(out) is np.float32 and out == np.float32(1.0) and out.tobytes() == np.float32(1).tobytes(), name
    # no forced win (FW_NONE), and a terminal position (white's five on the board): the value object itself comes back
    for name in ("the block makes a four", "the defender wins first", "two threats at the root", "terminal root"):
        rid = hm[name][0]
        assert utils.forced_win(rid[1:], 9, 5, 4, 2000)["result"] == utils.FW_NONE, name
        assert utils.leaf_tactics_value(rid[1:], 9, 5, v, 4, 2000) is v, name
    assert utils.forced_win(hm["terminal root"][0][1:], 9, 5, 4, 2000)["status"] != 0
    # the chain needs three attacker moves: invisible at depth 2; and one node short of its search it is FW_UNKNOWN -- the budget
    # ran out, the network's value stays
    chain = hm["four-four chain"][0]
    assert utils.leaf_tactics_value(chain[1:], 9, 5, v, 2, 2000) is v
    full = utils.forced_win(chain[1:], 9, 5, 4, 2000)["nodes"]
    assert utils.forced_win(chain[1:], 9, 5, 4, full - 1)["result"] == utils.FW_UNKNOWN
    assert utils.leaf_tactics_value(chain[1:], 9, 5, v, 4, full - 1) is v
    assert utils.leaf_tactics_value(chain[1:], 9, 5, v, 4, full) == np.float32(1.0)
    # a win is a win for whoever is to move: white to move with black's stones and white's exchanged
    rid = hm["open three"][0]
    black, white = list(rid[1::2]), list(rid[2::2])
    assert len(black) == len(white)                   # (black to move in the original)
    spare = [c for c in range(81) if c not in rid[1:]][-1]
    swapped = [x for pair in zip(white, black) for x in pair] + [spare]    # white's old stones are black's, one more black stone: white to move
    assert utils.leaf_tactics_value(swapped, 9, 5, v, 4, 2000) == np.float32(1.0)


def test_the_evaluator_wrapper_passes_the_policy_through():
    from alpha_omok_amd import utils
    hm = hand_made()
    calls = []
    pol = np.arange(81, dtype=np.float32)

    def plain(moves, planes, sim):
        calls.append((tuple(moves), sim))
        return pol, np.float32(0.25)

    f = utils.leaf_tactics_evaluator(plain, 9, 5, 4, 64)
    win, quiet = hm["open three"][0][1:], hm["the block makes a four"][0][1:]
    p, v = f(list(win), None, 3)
    assert p is pol and v == np.float32(1.0)
    p, v = f(list(quiet), None, 4)
    assert p is pol and v == np.float32(0.25)
    assert calls == [(tuple(win), 3), (tuple(quiet), 4)]


def test_limits_of_the_python_arguments():
    from alpha_omok_amd import utils
    assert utils.LEAF_MAX_NODES == 1024
    assert utils.leaf_tactics_limits(None) is None and utils.leaf_tactics_limits(False) is None
    assert utils.leaf_tactics_limits(True) == (2, 16)
    assert utils.leaf_tactics_limits(dict(max_depth=6)) == (6, 16)
    assert utils.leaf_tactics_limits(dict(max_depth=2, max_nodes=1024)) == (2, 1024)
    for bad in (dict(max_nodes=1025), dict(max_depth=17), dict(max_depth=0), dict(depth=3), 4, (4, 64), dict(max_nodes=True)):
        with pytest.raises(ValueError):
            utils.leaf_tactics_limits(bad)
    assert utils.parse_leaf_tactics(None) is None
    assert utils.parse_leaf_tactics("6,256") == dict(max_depth=6, max_nodes=256)
    with pytest.raises(ValueError):
        utils.parse_leaf_tactics("6")


# ---------------------------------------------------------------------------------------------------------------------
# declarations
# ---------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_both_entry_points():
    from alpha_omok_amd import _lib, build, engine
    hdr = open(os.path.join(REPO, "include", "omok_hip.h")).read()
    for name, nargs in NEW_SYMBOLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, "omok_hip.h does not declare %s" % name
        assert len(m.group(1).split(",")) == nargs
        assert name in _lib.SYMBOLS, "_lib.SYMBOLS lacks %s" % name
        assert len(_lib.SYMBOLS[name][1]) == nargs
    doc = hdr[:hdr.index("int ao_set_leaf_tactics")].rsplit("/*", 1)[1]
    for word in ("leaf_tactics_value", "FW_WIN", "FW_UNKNOWN", "1..1024", "AO_LEAF_TACTICS_SERIAL"):
        assert word in doc, word
    assert "leaf_tactics.hip" in build.SOURCES
    limits = open(os.path.join(build.CSRC, "tactics_limits.hpp")).read()
    assert re.search(r"kLeafMaxNodes\s*=\s*1024\b", limits)
    build.build()
    lib = _lib.load(build_if_missing=False)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), "libomok_hip.so does not export %s" % name
    assert lib.ao_abi_version() == 2          # additive change
    assert hasattr(engine.Engine, "set_leaf_tactics") and hasattr(engine.Engine, "leaf_tactics_stats")


# ---------------------------------------------------------------------------------------------------------------------
# the conditions of the device test, on the host
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BOARDS)
def test_the_roots_make_the_switch_visible(oracle, B):
    """One ply of the wrapped and of the plain reference search on the 8 roots: proven leaves are at least a quarter of the
    leaves searched; for at least half of the games the visit row differs from the plain search's; and at 9x9 at least one
    leaf runs out of its 64 nodes and keeps the network's value."""
    roots, seeds = roots_of(B), seeds_of()
    assert all(len(set(r[1:])) == len(r) - 1 for r in roots)
    tally = np.zeros((GAMES, 4), np.int64)
    differ = 0
    for g, root in enumerate(roots):
        assert oracle.check_win(oracle.get_board(list(root)[1:], B), MARK[B]) == 0
        plain = oracle_agent(oracle, B, seeds[g], stub_of(oracle, B))
        wrapped = oracle_agent(oracle, B, seeds[g], counting_evaluator(stub_of(oracle, B), B, tally[g]))
        _, vis_plain, _ = plain.get_pi(root, 1)
        _, vis, _ = wrapped.get_pi(root, 1)
        differ += not np.array_equal(vis, vis_plain)
    searched, proven, unknown, nodes = tally.sum(axis=0)
    print("board %d: %d leaves searched, %d proven, %d out of nodes, %.1f nodes per leaf, %d of %d visit rows differ"
          % (B, searched, proven, unknown, nodes / max(searched, 1), differ, GAMES))
    assert searched > 0 and 4 * proven >= searched, (searched, proven)
    assert 2 * differ >= GAMES, differ
    if B == 9:
        assert unknown >= 1, "no leaf ran out of %d nodes" % NODES
