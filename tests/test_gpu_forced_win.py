"""-m gpu: forced wins by continuous fours on the device (PositionBatch.forced_wins, k_forced_wins of csrc/positions.hip)
against the host definition, alpha_omok_amd.utils.forced_win. Integer results: every comparison is exact equality, `nodes`
and `line` included -- the order of visits is part of the contract.

The fixture and its host results are those of tests/test_forced_win_host.py, read from tests/golden/forced_win_fixture.npz
(that test holds the file to the live host definition): every prefix of seeded random games on 3/3, 5/4, 6/4, 8/5, 9/5, 12/5
and 15/5 (board / win_mark), max_depth 6, max_nodes 2000. In 64-cell mask words: 8x8 is exactly one full word, 9x9 has cells
on both sides of bit 63/64, 12x12 needs three words, 15x15 four with the last one partial."""
import functools

import numpy as np
import pytest

from test_forced_win_host import CASES, DEPTH, KEYS, MARK, NODES, SMALL_NODES, as_arrays, golden_fixture, hand_made

pytestmark = pytest.mark.gpu
OUT = KEYS + ("err",)


def _batch(B, **kw):
    from alpha_omok_amd.positions import PositionBatch
    return PositionBatch(B, win_mark=MARK[B], **kw)


@functools.lru_cache(maxsize=None)
def _golden():
    return golden_fixture()


def _same(d, want, rows=slice(None), what=""):
    for key in KEYS:
        bad = np.flatnonzero((d[key] != want[key][rows]).reshape(len(d[key]), -1).any(axis=1))
        assert bad.size == 0, "%s %s of %d positions, first row %d: device %s, host %s" % (
            what, key, bad.size, bad[0], d[key][bad[0]], want[key][rows][bad[0]])


@pytest.mark.parametrize("B", [B for B, _, _ in CASES])
def test_forced_wins_of_every_prefix(B):
    g = _golden()[B]
    with _batch(B) as pb:
        d = pb.forced_wins(g["ids"], DEPTH, NODES)
    n = len(g["ids"])
    assert d["moves"].dtype == np.uint8 and d["moves"].shape == (n, B * B)
    assert d["line"].dtype == np.int16 and d["line"].shape == (n, 2 * DEPTH - 1)
    assert all(d[key].dtype == np.int32 and d[key].shape == (n,) for key in OUT if key not in ("moves", "line"))
    assert not d["err"].any()
    _same(d, g, what="board %d" % B)
    # (what the outputs promise each other)
    win = d["result"] == 1
    assert (d["depth"][~win] == 0).all() and (d["move"][~win] == -1).all() and not d["moves"][~win].any()
    assert (d["line_len"][~win] == 0).all() and (d["line"][~win] == -1).all()
    assert (d["nodes"][d["result"] == 2] == NODES).all() and (d["result"][d["status"] != 0] == 0).all()
    assert (d["move"][win] == d["moves"][win].argmax(axis=1)).all() and (d["line"][win, 0] == d["move"][win]).all()


@pytest.mark.parametrize("B", [5, 9, 15])
def test_chunks_and_bare_move_lists_change_nothing(B):
    g = _golden()[B]
    rows = slice(0, len(g["ids"]), 3)
    ids = g["ids"][rows]
    with _batch(B, capacity=7) as pb:
        d = pb.forced_wins(ids, DEPTH, NODES)
        bare = pb.forced_wins([i[1:] for i in ids], DEPTH, NODES, leading_zero=False)
        none = pb.forced_wins([], DEPTH, NODES)
    _same(d, g, rows, "chunks of 7, board %d" % B)
    for key in OUT:
        np.testing.assert_array_equal(d[key], bare[key], err_msg=key)
    assert none["result"].shape == (0,) and none["moves"].shape == (0, B * B) and none["line"].shape == (0, 2 * DEPTH - 1)


def test_errors_stay_with_their_position():
    B, A = 9, 81
    g = _golden()[B]
    picks = [int(i) for i in np.flatnonzero(g["result"] == 1)[::40][:6]]
    good = [g["ids"][i] for i in picks]
    bad = [((0, 5, -1, 6), 1), ((0, 5, 6, A), 1), ((0, 3, 4, 3), 2), ((0,) + tuple(range(A)) + (0,), 3)]
    mixed, where_good = [], []
    for i, rid in enumerate(good):
        mixed.append(rid)
        where_good.append(len(mixed) - 1)
        if i < len(bad):
            mixed.append(bad[i][0])
    where_bad = [i for i in range(len(mixed)) if i not in where_good]
    with _batch(B, capacity=4) as pb:                                          # chunks that mix good and bad ids
        d = pb.forced_wins(mixed, DEPTH, NODES)
    assert d["err"][where_bad].tolist() == [c for _, c in bad] and not d["err"][where_good].any()
    for key in KEYS:
        np.testing.assert_array_equal(d[key][where_good], g[key][picks], err_msg=key)
        if key not in ("move", "line"):
            assert not d[key][where_bad].any(), key                            # a bad id's outputs are zero ...
    assert (d["move"][where_bad] == -1).all() and (d["line"][where_bad] == -1).all()    # ... or -1


@pytest.mark.parametrize("B", [6, 9, 15])
def test_depth_one_is_win_cells(B):
    g = _golden()[B]
    with _batch(B) as pb:
        d = pb.forced_wins(g["ids"], 1, NODES)
        w = pb.win_cells(g["ids"])
    assert d["line"].shape == (len(g["ids"]), 1)
    np.testing.assert_array_equal(d["moves"], w["mine"])
    np.testing.assert_array_equal(d["result"], w["mine"].any(axis=1).astype(np.int32))
    np.testing.assert_array_equal(d["depth"], d["result"])
    np.testing.assert_array_equal(d["nodes"], np.ones(len(g["ids"]), np.int32))
    np.testing.assert_array_equal(d["status"], w["status"])
    np.testing.assert_array_equal(d["turn"], w["turn"])
    np.testing.assert_array_equal(d["line"][:, 0], d["move"])


@pytest.mark.parametrize("B", [B for B, _, _ in CASES])
def test_small_budget(B):
    """max_nodes 50: a position the host gives up on is given up on, with nothing of the search left; every other position
    is what it was with 2000 nodes."""
    g = _golden()[B]
    with _batch(B) as pb:
        d = pb.forced_wins(g["ids"], DEPTH, SMALL_NODES)
    cut = g["small_unknown"].astype(bool)
    assert B < 8 or cut.any()
    np.testing.assert_array_equal(d["result"] == 2, cut)
    for key in KEYS:
        np.testing.assert_array_equal(d[key][~cut], g[key][~cut], err_msg=key)
    assert (d["nodes"][cut] == SMALL_NODES).all() and (d["move"][cut] == -1).all() and (d["line"][cut] == -1).all()
    for key in ("depth", "moves", "line_len"):
        assert not d[key][cut].any(), key
    np.testing.assert_array_equal(d["status"], g["status"])
    np.testing.assert_array_equal(d["turn"], g["turn"])


def test_hand_made_positions_and_the_deepest_search():
    """The host test's hand-made positions at max_depth 4, and one of them at the limits (max_depth 16, max_nodes 65536)
    against the host at the same limits: all 16 levels of the stack."""
    from alpha_omok_amd import utils
    cases = hand_made()
    names = sorted(cases)
    with _batch(9) as pb:
        d = pb.forced_wins([cases[n][0] for n in names], 4, 2000)
        deep = pb.forced_wins([cases["the block makes a four"][0]], 16, 65536)
    host = as_arrays([utils.forced_win(cases[n][0][1:], 9, 5, 4, 2000) for n in names], 81, 4)
    _same(d, host, what="hand-made")
    for i, n in enumerate(names):
        _, result, depth, moves, line, _ = cases[n]
        assert (d["result"][i], d["depth"][i], np.flatnonzero(d["moves"][i]).tolist(), d["line"][i, :d["line_len"][i]].tolist()) == \
            (result, depth, moves, line), n
    _same(deep, as_arrays([utils.forced_win(cases["the block makes a four"][0][1:], 9, 5, 16, 65536)], 81, 16), what="deep")
    assert deep["line"].shape == (1, 31)


def test_zero_agent_get_forced_win_is_the_position_batch_row():
    from alpha_omok_amd.agents import ZeroAgent
    B = 9
    g = _golden()[B]
    agent = ZeroAgent(B, 4, 5, noise=False)
    picks = [int(np.flatnonzero((g["result"] == 1) & (g["depth"] == k))[0]) for k in (1, 2, 3, 5)]
    picks += [int(np.flatnonzero(g["result"] == 2)[0]), 0]
    for i in picks:
        result, depth, moves, line = agent.get_forced_win(g["ids"][i], DEPTH, NODES)
        assert moves.dtype == bool and moves.shape == (B, B) and isinstance(line, list)
        assert (result, depth) == (g["result"][i], g["depth"][i])
        np.testing.assert_array_equal(moves.ravel(), g["moves"][i].astype(bool))
        assert line == g["line"][i, :g["line_len"][i]].tolist()
    with pytest.raises(ValueError):
        agent.get_forced_win((0, 3, 3))
    with pytest.raises(ValueError):
        agent.get_forced_win((0, 3), max_depth=17)


def test_forced_win_summary_is_the_sum_of_the_host_definition():
    from alpha_omok_amd import evaluate, utils
    from test_forced_win_host import games_of
    B = 9
    games = [(0, g) for g in games_of(B, 5, 32)[:10]]
    got = evaluate.forced_win_summary(games, B, DEPTH, NODES)
    want = {name: dict(plies=0, forced_wins=0, followed=0, missed=0, unknown=0) for name in ("black", "white")}
    g = _golden()[B]
    row = {rid: i for i, rid in enumerate(g["ids"])}
    for _, mv in games:
        for t in range(len(mv)):
            i, w = row[(0,) + tuple(mv[:t])], want["black" if t % 2 == 0 else "white"]
            assert g["status"][i] == 0
            w["plies"] += 1
            w["unknown"] += int(g["result"][i] == 2)
            if g["result"][i] == 1 and g["depth"][i] >= 2:
                w["forced_wins"] += 1
                w["followed" if g["moves"][i, mv[t]] else "missed"] += 1
    assert got == want
    assert sum(v["forced_wins"] for v in want.values()) > 0 and sum(v["missed"] for v in want.values()) > 0
