"""-m gpu: the tactical audit on the device (PositionBatch.win_cells / audit, k_win_cells / k_audit_games of
csrc/positions.hip) against its host definition, alpha_omok_amd.utils.win_cells / audit_moves (try every empty cell with
check_win). Integer results: every comparison is exact equality.

Fixture: seeded uniformly random legal games -- np.random.RandomState(1000 + B), one permutation of the cells per game, cut
at the first terminal position, so a game is played on past missed wins until a win is taken or the board is full -- 64
games each for 3/3, 5/5, 6/4, 8/5, 9/5 and 32 each for 12/5 and 15/5 (board / win_mark). In 64-cell mask words: 8x8 is
exactly one full word, 9x9 has cells on both sides of bit 63/64, 12x12 needs three words, 15x15 four with the last one
partial. On the host these give, per board, positions with `mine` not empty / THREAT / LOST: 3x3 146 / 114 / 26, 5x5
84 / 111 / 8, 6x6 497 / 211 / 85, 8x8 641 / 343 / 137, 9x9 995 / 396 / 142, 12x12 833 / 239 / 112, 15x15 1139 / 333 / 157;
over the set 332 wins taken, 4003 missed, 142 single threats blocked and 1000 not (asserted below as "at least one")."""
import functools

import numpy as np
import pytest

from test_tactics_host import hand_made_positions, records_9x9

pytestmark = pytest.mark.gpu

CASES = ((3, 3, 64), (5, 5, 64), (6, 4, 64), (8, 5, 64), (9, 5, 64), (12, 5, 32), (15, 5, 32))   # board, win_mark, games
MARK = {B: k for B, k, _ in CASES}


def _batch(B, **kw):
    from alpha_omok_amd.positions import PositionBatch
    return PositionBatch(B, win_mark=kw.pop("win_mark", MARK.get(B)), **kw)


def _games(B, k, n):
    from alpha_omok_amd import utils
    rs = np.random.RandomState(1000 + B)
    games = []
    for _ in range(n):
        perm = rs.permutation(B * B).tolist()
        after = np.stack([utils.get_board([0] + perm[:t + 1], B) for t in range(B * B)])
        end = int(np.flatnonzero(utils.check_win_boards(after, k))[0])       # (the full board is terminal at the latest)
        games.append(perm[:end + 1])
    return games


@functools.lru_cache(maxsize=None)
def _references():
    """Per board: the games, every prefix of every game with utils.win_cells of it, and utils.audit_moves of every game --
    computed once on the host and shared; the fixture conditions are asserted here, before any device comparison."""
    from alpha_omok_amd import utils
    real = utils.win_cells
    memo = {}

    def remembered(board, turn, win_mark):     # audit_moves asks for the sets of the prefixes again: the same answers
        key = (np.asarray(board, np.int8).tobytes(), turn, win_mark)
        if key not in memo:
            memo[key] = real(board, turn, win_mark)
        return memo[key]

    refs = {}
    total = dict(taken=0, missed=0, blocked=0, unblocked=0)
    utils.win_cells = remembered
    try:
        for B, k, n in CASES:
            memo.clear()
            games = _games(B, k, n)
            ids, mine, theirs, status = [], [], [], []
            for g in games:
                after = np.stack([utils.get_board([0] + g[:t], B) for t in range(len(g) + 1)])
                status += utils.check_win_boards(after, k).tolist()
                for t in range(len(g) + 1):                                   # every prefix, the terminal one included
                    rid = (0,) + tuple(g[:t])
                    board = utils.get_board(rid, B)
                    a, b = utils.win_cells(board, t % 2, k)
                    ids.append(rid)
                    mine.append(a)
                    theirs.append(b)
            audits = [utils.audit_moves(g, B, k) for g in games]
            flags = np.stack([f for f, _ in audits])
            counts = np.stack([c for _, c in audits])
            refs[B] = dict(games=games, ids=ids, mine=np.array(mine, np.uint8), theirs=np.array(theirs, np.uint8),
                           status=np.array(status, np.int32), flags=flags, counts=counts)
            # a degenerate fixture must not pass silently
            assert (flags & utils.WIN_AVAILABLE).astype(bool).sum() >= 1 and refs[B]["mine"].any(), B
            assert (flags & utils.THREAT).astype(bool).sum() >= 1 and (flags & utils.LOST).astype(bool).sum() >= 1, B
            assert status[len(games[0])] != 0, B                              # (the last prefix of a game is terminal)
            total["taken"] += int((flags & utils.WIN_TAKEN).astype(bool).sum())
            total["missed"] += int(counts[:, 2].sum())
            total["blocked"] += int(((flags & utils.BLOCKED) != 0)[(flags & utils.LOST) == 0].sum())
            total["unblocked"] += int(counts[:, 4].sum())
    finally:
        utils.win_cells = real
    assert min(total.values()) >= 1, total
    return refs


@pytest.mark.parametrize("B", [B for B, _, _ in CASES])
def test_win_cells_of_every_prefix(B):
    r = _references()[B]
    with _batch(B) as pb:
        d = pb.win_cells(r["ids"])
    n = len(r["ids"])
    assert d["mine"].dtype == np.uint8 and d["mine"].shape == (n, B * B) and d["theirs"].shape == (n, B * B)
    assert not d["err"].any()
    np.testing.assert_array_equal(d["status"], r["status"])
    np.testing.assert_array_equal(d["turn"], np.array([(len(i) - 1) % 2 for i in r["ids"]], np.int32))
    for key in ("mine", "theirs"):
        bad = np.flatnonzero((d[key] != r[key]).any(axis=1))
        assert bad.size == 0, "%s of %d positions, first id %r: device %s, host %s" % (
            key, bad.size, r["ids"][bad[0]], np.flatnonzero(d[key][bad[0]]), np.flatnonzero(r[key][bad[0]]))
    assert not d["mine"][r["status"] != 0].any() and not d["theirs"][r["status"] != 0].any()


@pytest.mark.parametrize("B", [B for B, _, _ in CASES])
def test_audit_of_every_game(B):
    from alpha_omok_amd import positions as P
    r = _references()[B]
    with _batch(B) as pb:
        d = pb.audit(r["games"], leading_zero=False)
        d1 = pb.audit([(0,) + tuple(g) for g in r["games"]])
        desc = pb.describe(r["games"], leading_zero=False)
    assert d["flags"].dtype == np.uint8 and d["counts"].dtype == np.int32 and d["counts"].shape == (len(r["games"]), 8)
    assert not d["err"].any()
    np.testing.assert_array_equal(d["flags"], r["flags"])
    np.testing.assert_array_equal(d["counts"], r["counts"])
    for key in d:                                                              # leading_zero True and False agree
        np.testing.assert_array_equal(d[key], d1[key], err_msg=key)
    # the counters are what the flags sum to
    f = d["flags"]
    avail, taken = (f & P.WIN_AVAILABLE) != 0, (f & P.WIN_TAKEN) != 0
    threat, blocked, lost = (f & P.THREAT) != 0, (f & P.BLOCKED) != 0, (f & P.LOST) != 0
    np.testing.assert_array_equal(d["counts"][:, 1], avail.sum(axis=1))
    np.testing.assert_array_equal(d["counts"][:, 2], (avail & ~taken).sum(axis=1))
    np.testing.assert_array_equal(d["counts"][:, 3], (threat & ~lost).sum(axis=1))
    np.testing.assert_array_equal(d["counts"][:, 4], (threat & ~lost & ~blocked).sum(axis=1))
    np.testing.assert_array_equal(d["counts"][:, 5], lost.sum(axis=1))
    np.testing.assert_array_equal(d["counts"][:, 0], [len(g) for g in r["games"]])      # (the games stop at their end)
    np.testing.assert_array_equal(d["counts"][:, 6], desc["end_ply"])
    np.testing.assert_array_equal(d["counts"][:, 7], desc["status"])
    assert not (taken & ~avail).any() and not (blocked & ~threat).any() and not (lost & ~threat).any() and not (avail & threat).any()


@pytest.mark.parametrize("B", [9, 15])
def test_hand_made_positions(B):
    """The cases of the host test -- a gap, a six, runs that reach the edge and "go on" in the next row by bit index (row
    and both diagonals), both colours, a terminal board -- through the device."""
    pos = hand_made_positions(B)
    with _batch(B) as pb:
        d = pb.win_cells([rid for _, rid, _, _, _ in pos])
    assert not d["err"].any()
    for i, (name, rid, turn, mine, theirs) in enumerate(pos):
        assert int(d["turn"][i]) == turn, name
        np.testing.assert_array_equal(d["mine"][i].astype(bool), mine, err_msg="mine: %s" % name)
        np.testing.assert_array_equal(d["theirs"][i].astype(bool), theirs, err_msg="theirs: %s" % name)
    assert d["status"][[n == "terminal" for n, _, _, _, _ in pos]].tolist() == [1]


@pytest.mark.parametrize("B", [9, 15])
def test_hand_made_records(B):
    """A missed win followed by a taken one, a single threat blocked and not blocked, a double threat, moves after the end
    (the 9x9 records, moved cell by cell onto the 15x15 board)."""
    from alpha_omok_amd import utils
    recs = records_9x9()
    names = sorted(recs)
    games = [[(m // 9) * B + m % 9 for m in recs[n][0]] for n in names]
    with _batch(B) as pb:
        d = pb.audit(games, leading_zero=False)
    for i, name in enumerate(names):
        mv, fl, cn = recs[name]
        host_f, host_c = utils.audit_moves(games[i], B, 5)
        np.testing.assert_array_equal(d["flags"][i], host_f, err_msg=name)
        np.testing.assert_array_equal(d["counts"][i], host_c, err_msg=name)
        if B == 9:
            assert d["flags"][i, :len(mv)].tolist() == fl and d["counts"][i].tolist() == cn, name


def test_errors_stay_with_their_record():
    B, A = 9, 81
    r = _references()[B]
    good = r["games"][:6]
    bad = [([5, -1, 6], 1), ([5, 6, A], 1), ([3, 4, 3], 2), (list(range(A)) + [0], 3)]
    mixed, where_good = [], []
    for i, g in enumerate(good):
        mixed.append(g)
        where_good.append(len(mixed) - 1)
        if i < len(bad):
            mixed.append(bad[i][0])
    where_bad = [i for i in range(len(mixed)) if i not in where_good]
    with _batch(B, capacity=4) as pb:                                          # chunks that mix good and bad records
        a = pb.audit(mixed, leading_zero=False)
        w = pb.win_cells(mixed, leading_zero=False)
    with _batch(B) as pb:
        a0 = pb.audit(good, leading_zero=False)
        w0 = pb.win_cells(good, leading_zero=False)
    for d, d0 in ((a, a0), (w, w0)):
        assert d["err"][where_bad].tolist() == [c for _, c in bad]
        assert not d["err"][where_good].any() and not d0["err"].any()
        for key in d0:
            np.testing.assert_array_equal(d[key][where_good], d0[key], err_msg=key)
            if key != "err":
                assert not d[key][where_bad].any(), key                        # a bad record's outputs are zero
    np.testing.assert_array_equal(a0["flags"], r["flags"][:6])
    np.testing.assert_array_equal(a0["counts"], r["counts"][:6])


def test_chunks_empty_calls_empty_id_and_full_draw():
    r = _references()[9]
    ten = r["ids"][20:30]
    where = slice(20, 30)
    with _batch(9, capacity=3) as pb:                                          # 10 positions through chunks of 3, 3, 3, 1
        d = pb.win_cells(ten)
        a = pb.audit(r["games"][:10], leading_zero=False)
        e = pb.win_cells([])                                                   # n = 0
        ea = pb.audit([])
        one = pb.win_cells([(0,)])                                             # the empty id
        onea = pb.audit([(0,)])
    np.testing.assert_array_equal(d["mine"], r["mine"][where])
    np.testing.assert_array_equal(d["theirs"], r["theirs"][where])
    np.testing.assert_array_equal(d["status"], r["status"][where])
    np.testing.assert_array_equal(a["flags"], r["flags"][:10])
    np.testing.assert_array_equal(a["counts"], r["counts"][:10])
    assert e["mine"].shape == (0, 81) and e["err"].shape == (0,) and ea["flags"].shape == (0, 81) and ea["counts"].shape == (0, 8)
    assert not one["mine"].any() and not one["theirs"].any() and one["status"].tolist() == [0] and one["turn"].tolist() == [0]
    assert not one["err"].any() and not onea["err"].any()
    assert not onea["flags"].any() and onea["counts"].tolist() == [[0, 0, 0, 0, 0, 0, -1, 0]]
    from alpha_omok_amd import utils
    draw = [0, 1, 2, 4, 3, 5, 7, 6, 8]                                         # X O X / X O O / O X X: all nine cells
    with _batch(3) as pb:
        a = pb.audit([draw], leading_zero=False)
        w = pb.win_cells([draw, draw[:8]], leading_zero=False)
    host_f, host_c = utils.audit_moves(draw, 3, 3)
    np.testing.assert_array_equal(a["flags"][0], host_f)
    np.testing.assert_array_equal(a["counts"][0], host_c)
    assert a["counts"][0, 0] == 9 and a["counts"][0, 6] == 8 and a["counts"][0, 7] == 3
    assert w["status"].tolist() == [3, 0] and not w["mine"].any() and not w["theirs"][0].any()
    mine, theirs = utils.win_cells(utils.get_board([0] + draw[:8], 3), 0, 3)
    np.testing.assert_array_equal(w["theirs"][1].astype(bool), theirs)
    assert not mine.any()                                                      # the last cell only fills the board


def test_zero_agent_get_win_cells_is_the_position_batch_row():
    from alpha_omok_amd.agents import ZeroAgent
    B = 9
    r = _references()[B]
    agent = ZeroAgent(B, 4, 5, noise=False)
    picks = [i for i in np.flatnonzero(r["mine"].any(axis=1) | r["theirs"].any(axis=1))[:3]] + [0]
    with _batch(B) as pb:
        d = pb.win_cells([r["ids"][i] for i in picks])
    for row, i in enumerate(picks):
        mine, theirs = agent.get_win_cells(r["ids"][i])
        assert mine.dtype == bool and mine.shape == (B, B) and theirs.shape == (B, B)
        np.testing.assert_array_equal(mine.ravel(), d["mine"][row].astype(bool))
        np.testing.assert_array_equal(theirs.ravel(), d["theirs"][row].astype(bool))
        np.testing.assert_array_equal(mine.ravel(), r["mine"][i].astype(bool))
    with pytest.raises(ValueError):
        agent.get_win_cells((0, 3, 3))


def test_tactical_summary_is_the_sum_by_parity_of_audit_moves():
    from alpha_omok_amd import evaluate, utils
    B = 9
    r = _references()[B]
    games = [(int(c[7]), list(g)) for g, c in zip(r["games"][:12], r["counts"][:12])]
    got = evaluate.tactical_summary(games, B)
    want = {name: dict(plies=0, wins_available=0, wins_missed=0, single_threats=0, blocks_missed=0, lost_positions=0)
            for name in ("black", "white")}
    for _, g in games:
        flags, counts = utils.audit_moves(g, B, 5)
        for t in range(int(counts[0])):
            f, w = int(flags[t]), want["black" if t % 2 == 0 else "white"]
            w["plies"] += 1
            w["wins_available"] += bool(f & utils.WIN_AVAILABLE)
            w["wins_missed"] += bool(f & utils.WIN_AVAILABLE) and not f & utils.WIN_TAKEN
            w["single_threats"] += bool(f & utils.THREAT) and not f & utils.LOST
            w["blocks_missed"] += bool(f & utils.THREAT) and not f & (utils.LOST | utils.BLOCKED)
            w["lost_positions"] += bool(f & utils.LOST)
    assert got == want
    assert sum(v["wins_available"] for v in want.values()) > 0 and sum(v["single_threats"] for v in want.values()) > 0
