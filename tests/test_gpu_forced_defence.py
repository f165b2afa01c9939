"""-m gpu: which replies hold against a forced win by continuous fours, on the device (PositionBatch.forced_defences,
k_forced_defences / k_defence_rows of csrc/positions.hip) against the host definition, alpha_omok_amd.utils.forced_defences.
Integer results: every comparison is exact equality, `nodes` included.

The fixture and its host results are those of tests/test_forced_defence_host.py, read from
tests/golden/forced_defence_fixture.npz (that test holds the file to the live host definition): every prefix of seeded random
games on 3/3, 5/4, 6/4, 8/5, 9/5 and 15/5 (board / win_mark), max_depth 6, max_nodes 2000. In 64-cell mask words 8x8 is one
full word with the pass at index 64, 9x9 has cells on both sides of bit 63/64, 15x15 needs four, the last one partial."""
import functools

import numpy as np
import pytest

from test_forced_defence_host import (CASES, DEPTH, KEYS, MARK, NODES, SMALL_BOARD, SMALL_NODES, as_arrays, fixture_games, golden_fixture,
                                      open_three, summary_of)
from test_forced_win_host import hand_made

pytestmark = pytest.mark.gpu
OUT = KEYS + ("err",)
WIDE = ("threat_moves", "reply", "depth")


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


def _shapes(d, n, A):
    assert all(d[key].dtype == np.uint8 and d[key].shape == (n, A) for key in WIDE)
    assert d["counts"].dtype == np.int32 and d["counts"].shape == (n, 4)
    assert all(d[key].dtype == np.int32 and d[key].shape == (n,) for key in OUT if key not in WIDE + ("counts",))


@pytest.mark.parametrize("B", [B for B, _, _ in CASES])
def test_forced_defences_of_every_prefix(B):
    from alpha_omok_amd import positions as P
    g = _golden()[B]
    with _batch(B) as pb:
        d = pb.forced_defences(g["ids"], DEPTH, NODES)
    _shapes(d, len(g["ids"]), B * B)
    assert not d["err"].any()
    _same(d, g, what="board %d" % B)
    # (what the outputs promise each other)
    np.testing.assert_array_equal(d["counts"][:, 0], (d["reply"] != P.FD_NONE).sum(axis=1))
    for col, v in ((1, P.FD_SAFE), (2, P.FD_LOSES), (3, P.FD_UNKNOWN)):
        np.testing.assert_array_equal(d["counts"][:, col], (d["reply"] == v).sum(axis=1))
    assert not d["depth"][d["reply"] != P.FD_LOSES].any() and d["depth"][d["reply"] == P.FD_LOSES].all()
    term = d["status"] != 0
    assert term.any()
    for key in OUT:
        if key not in ("status", "turn"):
            assert not d[key][term].any(), key
    assert (d["threat_depth"][d["threat"] != P.FW_WIN] == 0).all() and not d["threat_moves"][d["threat"] != P.FW_WIN].any()
    assert d["threat_moves"][d["threat"] == P.FW_WIN].any(axis=1).all()


@pytest.mark.parametrize("B", [5, 9, 15])
def test_chunks_and_bare_move_lists_change_nothing(B):
    g = _golden()[B]
    rows = slice(0, len(g["ids"]), 5)
    ids = g["ids"][rows]
    with _batch(B, capacity=3) as pb:
        d = pb.forced_defences(ids, DEPTH, NODES)
        bare = pb.forced_defences([i[1:] for i in ids], DEPTH, NODES, leading_zero=False)
        none = pb.forced_defences([], DEPTH, NODES)
    assert len(ids) > 2 * 3                                                    # chunk edges inside the batch
    _same(d, g, rows, "chunks of 3, board %d" % B)
    for key in OUT:
        np.testing.assert_array_equal(d[key], bare[key], err_msg=key)
    _shapes(none, 0, B * B)


def test_errors_stay_with_their_position():
    B, A = 9, 81
    g = _golden()[B]
    picks = [int(i) for i in np.flatnonzero(g["threat"] == 1)[::12][:6]]
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
        d = pb.forced_defences(mixed, DEPTH, NODES)
    assert len(picks) == 6
    assert d["err"][where_bad].tolist() == [c for _, c in bad] and not d["err"][where_good].any()
    for key in KEYS:
        np.testing.assert_array_equal(d[key][where_good], g[key][picks], err_msg=key)
        assert not d[key][where_bad].any(), key                                # a bad id's outputs are zero


@pytest.mark.parametrize("B", [5, 8, 9, 15])
def test_two_kernels_one_search(B):
    """every reply of a sample of positions is what forced_wins says of the position after it"""
    g = _golden()[B]
    rows = [i for i in range(0, len(g["ids"]), 9) if g["status"][i] == 0]
    with _batch(B) as pb:
        d = pb.forced_defences([g["ids"][i] for i in rows], DEPTH, NODES)
        after, where = [], []
        for r, i in enumerate(rows):
            for c in np.flatnonzero(d["reply"][r]):
                after.append(g["ids"][i] + (int(c),))
                where.append((r, int(c)))
        w = pb.forced_wins(after, DEPTH, NODES)
    assert not w["err"].any() and len(after) == d["counts"][:, 0].sum()
    r, c = np.array(where).T
    np.testing.assert_array_equal(d["reply"][r, c].astype(np.int32) - 1, w["result"])
    np.testing.assert_array_equal(d["depth"][r, c].astype(np.int32), w["depth"])
    # (the pass has no id of its own: its nodes are what the replies' leave of the sum)
    of_pass = d["nodes"] - np.bincount(r, weights=w["nodes"], minlength=len(rows)).astype(np.int64)
    assert (of_pass >= 1).all() and (of_pass <= NODES).all()


@pytest.mark.parametrize("B", [6, 9, 15])
def test_depth_one_is_win_cells(B):
    from alpha_omok_amd import positions as P
    g = _golden()[B]
    with _batch(B) as pb:
        d = pb.forced_defences(g["ids"], 1, NODES)
        w = pb.win_cells(g["ids"])
    mine, theirs = w["mine"].astype(bool), w["theirs"].astype(bool)
    open_ = (w["status"] == 0)[:, None]
    np.testing.assert_array_equal(d["threat"], theirs.any(axis=1).astype(np.int32))
    np.testing.assert_array_equal(d["threat_depth"], d["threat"])
    np.testing.assert_array_equal(d["threat_moves"], w["theirs"])
    empty = np.ones_like(mine)
    for i, rid in enumerate(g["ids"]):
        empty[i, list(rid[1:])] = False
    # a reply loses at depth one where it neither wins nor leaves the opponent without a winning cell
    left = theirs.sum(axis=1)[:, None] - theirs
    loses = open_ & empty & ~mine & (left > 0)
    np.testing.assert_array_equal(d["reply"] == P.FD_LOSES, loses)
    np.testing.assert_array_equal(d["reply"] == P.FD_SAFE, open_ & empty & ~loses)
    assert not (d["reply"] == P.FD_UNKNOWN).any() and loses.any()
    np.testing.assert_array_equal(d["depth"], loses.astype(np.uint8))
    np.testing.assert_array_equal(d["nodes"], np.where(open_[:, 0], empty.sum(axis=1) + 1, 0))
    np.testing.assert_array_equal(d["status"], w["status"])
    np.testing.assert_array_equal(d["turn"], w["turn"])


def test_small_budget():
    """max_nodes 50 on 9x9: the searches the host gives up on are given up on, one by one"""
    from alpha_omok_amd import positions as P
    g = _golden()[SMALL_BOARD]
    with _batch(SMALL_BOARD) as pb:
        d = pb.forced_defences(g["ids"], DEPTH, SMALL_NODES)
    assert (g["small"]["threat"] == P.FW_UNKNOWN).any() and (g["small"]["reply"] == P.FD_UNKNOWN).any()
    _same(d, g["small"], what="budget %d" % SMALL_NODES)


def test_hand_made_positions_and_the_limits():
    """The open three of the host test at max_depth 4, and it and the four-four chain with white to move (a threat in three:
    four replies hold) at the limits, max_depth 16 and max_nodes 65536, against the host at the same limits."""
    from alpha_omok_amd import utils
    rid, ends = open_three()
    chain = hand_made()["four-four chain"][0] + (8 * 9 + 4,)
    with _batch(9) as pb:
        d = pb.forced_defences([rid], 4, 2000)
        deep = pb.forced_defences([rid, chain], 16, 65536)
    _same(d, as_arrays([utils.forced_defences(rid[1:], 9, 5, 4, 2000)], 81), what="hand-made")
    assert (d["threat"][0], d["threat_depth"][0], d["nodes"][0], d["counts"][0].tolist()) == (1, 2, 616, [76, 2, 74, 0])
    assert np.flatnonzero(d["reply"][0] == 1).tolist() == ends
    _same(deep, as_arrays([utils.forced_defences(i[1:], 9, 5, 16, 65536) for i in (rid, chain)], 81), what="limits")
    assert (deep["threat"][1], deep["threat_depth"][1], deep["counts"][1].tolist()) == (1, 3, [70, 4, 66, 0])


def test_zero_agent_get_forced_defences_is_the_position_batch_row():
    from alpha_omok_amd import positions as P
    from alpha_omok_amd.agents import ZeroAgent
    B = 9
    g = _golden()[B]
    agent = ZeroAgent(B, 4, 5, noise=False)
    mixed = (g["counts"][:, 1] > 0) & (g["counts"][:, 2] > 0)
    picks = [int(np.flatnonzero(mixed & (g["threat_depth"] == k))[0]) for k in (1, 2)]
    picks += [int(np.flatnonzero(g["counts"][:, 3] > 0)[0]), int(np.flatnonzero(g["status"] != 0)[0]), 0]
    for i in picks:
        threat, depth, safe, losing = agent.get_forced_defences(g["ids"][i], DEPTH, NODES)
        assert safe.dtype == bool and safe.shape == (B, B) and losing.dtype == bool and losing.shape == (B, B)
        assert (threat, depth) == (g["threat"][i], g["threat_depth"][i])
        np.testing.assert_array_equal(safe.ravel(), g["reply"][i] == P.FD_SAFE)
        np.testing.assert_array_equal(losing.ravel(), g["reply"][i] == P.FD_LOSES)
    with pytest.raises(ValueError):
        agent.get_forced_defences((0, 3, 3))
    with pytest.raises(ValueError):
        agent.get_forced_defences((0, 3), max_depth=17)


def test_forced_defence_summary_is_the_sum_of_the_host_definition():
    from alpha_omok_amd import evaluate
    B = SMALL_BOARD
    g = _golden()[B]
    games = [(0, mv) for mv in fixture_games(B)]
    got = evaluate.forced_defence_summary(games, B, DEPTH, NODES)
    want = summary_of(g, g["ids"], games)
    assert got == want
    assert sum(v["defended"] for v in want.values()) > 0 and sum(v["blundered"] for v in want.values()) > 0
    for v in want.values():
        assert v["threats"] == v["defended"] + v["blundered"] + v["hopeless"] + v["unknown"]
