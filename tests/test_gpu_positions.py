"""-m gpu: the position batch (alpha_omok_amd.positions.PositionBatch, csrc/positions.hip) against the reference's own
answers (gv1: utils.check_win, gv3: utils.get_state_pt / get_board / get_turn) and against the host mirror of the
reference's scan (alpha_omok_amd.utils.check_win). Every comparison is exact: integers, or float32 bit for bit."""
import functools

import numpy as np
import pytest

import net_reference
from conftest import load_golden

pytestmark = pytest.mark.gpu

GV1_SIZES = ((3, 3), (9, 5), (15, 5))
# the hand-made lines of gv1 (tools/gen_golden.py, gv1): per colour, per placement, the full line, the line with its last
# stone missing, the line with its third stone of the other colour
def _gv1_placements(B, k):
    return ((0, 0, 0, 1), (B - 1, B - k, 0, 1), (0, B - 1, 1, 0), (B - k, 0, 1, 0), (0, 0, 1, 1), (B - k, B - k, 1, 1),
            (k - 1, 0, -1, 1), (B - 1, B - k, -1, 1))


def _batch(B, **kw):
    from alpha_omok_amd.positions import PositionBatch
    return PositionBatch(B, **kw)


def _host_win(board, k):
    from alpha_omok_amd import utils
    return utils.check_win(np.asarray(board, np.float64), k)


# ---------------------------------------------------------------------------------------------------------------------
# 1. gv1 on the device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", [4096, 64])
def test_check_win_gv1(capacity):
    """Every board of gv1 (the reference's check_win on hand-made lines, full boards and random boards; 3x3 mark 3, 9x9
    and 15x15 mark 5), one call per board size; capacity 64 makes the call loop over chunks."""
    g = load_golden("gv1_check_win")
    seen = 0
    for B, k in GV1_SIZES:
        sel = np.flatnonzero((g["size_mark"][:, 0] == B) & (g["size_mark"][:, 1] == k))
        assert sel.size > 300
        with _batch(B, win_mark=k, capacity=capacity) as pb:
            got = pb.check_win(g["boards"][sel][:, :B, :B])
        assert got.dtype == np.int32
        np.testing.assert_array_equal(got, g["win"][sel], err_msg="B=%d" % B)
        seen += sel.size
    assert seen == g["win"].size


# ---------------------------------------------------------------------------------------------------------------------
# 2. scan order
# ---------------------------------------------------------------------------------------------------------------------
SCAN_SIZES = ((5, 5), (6, 5), (9, 5), (12, 5), (13, 5), (15, 5), (3, 3), (4, 3))


@functools.lru_cache(maxsize=None)
def _dense_boards(B, k, count=160, seed=5):
    """Random dense boards (fixed seed; the last eighth full) and the host's answers. Returns (boards int8 [n, B, B],
    win int32 [n], both bool [n]: black AND white have a complete line somewhere)."""
    rs = np.random.RandomState(seed * 100 + B)
    boards = np.zeros((count, B, B), np.int8)
    for i in range(count):
        dens = 1.0 if i >= count - count // 8 else rs.uniform(0.75, 1.0)
        boards[i] = rs.choice([0, 1, -1], p=[1 - dens, dens / 2, dens / 2], size=(B, B))
    win = np.array([_host_win(b, k) for b in boards], np.int32)
    both = np.array([_host_win(b == 1, k) == 1 and _host_win(-(b == -1).astype(np.int8), k) == 2 for b in boards])
    return boards, win, both


def test_check_win_scan_order_on_dense_boards():
    """Boards on which BOTH colours have lines: only the reference's scan order (windows row-major, black before white
    inside a window) decides. Sizes: one window (5), four (6), exactly 64 = one pass of the wave (12), a second pass (13,
    15), bitboards of 2 / 3 / 4 words (9 / 12 / 15); mark 3 on 3x3 and 4x4."""
    n_both = {1: 0, 2: 0}
    full_draws = 0
    for B, k in SCAN_SIZES:
        boards, win, both = _dense_boards(B, k)
        with _batch(B, win_mark=k) as pb:
            got = pb.check_win(boards)
        bad = np.flatnonzero(got != win)
        assert bad.size == 0, "B=%d mark %d: boards %s: device %s, host %s" % (B, k, bad[:5], got[bad[:5]], win[bad[:5]])
        for w in (1, 2):
            n_both[w] += int((both & (win == w)).sum())
        full_draws += int(((win == 3) & (boards != 0).all(axis=(1, 2))).sum())
    # the generator did produce what the test is about
    assert n_both[1] >= 10 and n_both[2] >= 10, n_both
    assert full_draws >= 1


# ---------------------------------------------------------------------------------------------------------------------
# 3. gv1 through move lists
# ---------------------------------------------------------------------------------------------------------------------
def _playable(board, last, want, k, rs):
    """Filler stones of the short colour on empty cells of `board` until the stone counts are those of a game whose LAST
    move is the stone on `last`; the fillers leave the fixture's answer `want` alone and nobody has a line before the last
    move. Returns (filled board, move list: colours alternate, black first, `last` is the final move)."""
    B = board.shape[0]
    colour = int(board[last])
    nb, nw = int((board == 1).sum()), int((board == -1).sum())
    need_b, need_w = (nw + 1 - nb, 0) if colour == 1 and nb <= nw else (0, nb - 1 - nw) if colour == 1 else \
        (nw - nb, 0) if nb <= nw else (0, nb - nw)
    assert need_b >= 0 and need_w >= 0
    empty = np.flatnonzero(board.ravel() == 0)
    for _ in range(200):
        f = board.copy().ravel()
        pick = rs.permutation(empty)[:need_b + need_w]
        f[pick] = 1 if need_b else -1
        f = f.reshape(B, B)
        before = f.copy()
        before[last] = 0
        if _host_win(f, k) == want and _host_win(before, k) == 0:
            break
    else:
        raise AssertionError("no filler placement keeps the fixture's answer")
    lastc = last[0] * B + last[1]
    own = [c for c in np.flatnonzero(f.ravel() == colour).tolist() if c != lastc] + [lastc]
    other = np.flatnonzero(f.ravel() == -colour).tolist()
    blacks, whites = (own, other) if colour == 1 else (other, own)
    assert len(blacks) - len(whites) == (1 if colour == 1 else 0)
    moves = []
    for i in range(len(blacks)):
        moves.append(blacks[i])
        if i < len(whites):
            moves.append(whites[i])
    assert moves[-1] == lastc
    return f, moves


def test_move_lists_of_gv1_lines():
    """Every hand-made line of gv1 as a GAME: filler stones make the counts playable, the line's last stone is the final
    move. status is the fixture's answer; the win is found on the final move (end_ply: the incremental five-in-a-row test
    of the tree kernels, win_after_move, against a fixture); broken and blocked lines end nowhere. Plus the two overlines,
    a full-board draw and a win on the last empty cell."""
    g = load_golden("gv1_check_win")
    rs = np.random.RandomState(3)
    checked = 0
    for B, k in GV1_SIZES:
        sel = np.flatnonzero((g["size_mark"][:, 0] == B) & (g["size_mark"][:, 1] == k))
        fb, fw = g["boards"][sel][:, :B, :B], g["win"][sel]
        ids, boards, expect = [], [], []
        j = 0
        for colour in (1, -1):
            for r0, c0, dr, dc in _gv1_placements(B, k):
                cells = [(r0 + i * dr, c0 + i * dc) for i in range(k)]
                for variant in ("full", "broken", "blocked"):
                    b = fb[j].astype(np.int8)
                    want = int(fw[j])
                    j += 1
                    line = [c for c in cells if b[c] == colour]
                    assert len(line) == (k if variant == "full" else k - 1)        # this IS the fixture's case
                    assert want == ((1 if colour == 1 else 2) if variant == "full" else 0)
                    f, moves = _playable(b, line[-1], want, k, rs)
                    ids.append((0,) + tuple(moves))
                    boards.append(f)
                    expect.append((want, len(moves) - 1 if want else -1))
        if B > 5:
            for colour in (1, -1):       # the two six-in-a-row boards: the stone that makes the six is the third of the line
                b = fb[j].astype(np.int8)
                want = int(fw[j])
                j += 1
                line = list(zip(*np.nonzero(b == colour)))
                assert len(line) == 6 and want == (1 if colour == 1 else 2)
                f, moves = _playable(b, line[2], want, k, rs)
                ids.append((0,) + tuple(moves))
                boards.append(f)
                expect.append((want, len(moves) - 1))
        if B == 3:
            draw = (0, 0, 1, 2, 4, 3, 5, 7, 6, 8)            # X O X / X O O / O X X
            last_cell = (0, 0, 3, 1, 4, 5, 7, 6, 8, 2)       # black completes the top row on the last empty cell
            from alpha_omok_amd import utils
            assert _host_win(utils.get_board(draw, 3), 3) == 3 and _host_win(utils.get_board(draw[:-1], 3), 3) == 0
            assert _host_win(utils.get_board(last_cell, 3), 3) == 1 and _host_win(utils.get_board(last_cell[:-1], 3), 3) == 0
            for rid, want in ((draw, 3), (last_cell, 1)):
                ids.append(rid)
                boards.append(utils.get_board(rid, 3).astype(np.int8))
                expect.append((want, 8))
        with _batch(B, win_mark=k) as pb:
            d = pb.describe(ids)
        assert (d["err"] == 0).all()
        for i, (want, end) in enumerate(expect):
            assert int(d["status"][i]) == want, (B, i, ids[i])
            assert int(d["end_ply"][i]) == end, (B, i, ids[i])
            np.testing.assert_array_equal(d["board"][i], boards[i])
            checked += 1
    assert checked == 3 * 48 + 4 + 2


# ---------------------------------------------------------------------------------------------------------------------
# 4. gv3
# ---------------------------------------------------------------------------------------------------------------------
def test_planes_board_turn_legal_gv3():
    """Every id of gv3 (C in 3 / 5 / 7, B in 3 / 9 / 15): planes() is the reference's get_state_pt bit for bit -- finished
    games included, which the search never encodes --, board its get_board, turn its get_turn, legal the empty cells."""
    g = load_golden("gv3_state_planes")
    groups = {}
    for i in range(int(g["count"])):
        m = g["m%d" % i]
        groups.setdefault((int(m[0]), int(m[1])), []).append(((0,) + tuple(int(x) for x in m[2:]), i))
    assert sorted(groups) == [(B, C) for B in (3, 9, 15) for C in (3, 5, 7)]
    checked = 0
    for (B, C), items in sorted(groups.items()):
        ids = [nid for nid, _ in items]
        with _batch(B, inplanes=C, capacity=8) as pb:        # (every group is longer than a chunk: the planes land at their offsets)
            planes = pb.planes(ids)
            d = pb.describe(ids)
        assert planes.is_cuda and planes.dtype.is_floating_point and tuple(planes.shape) == (len(ids), C, B, B)
        got = planes.cpu().numpy()
        assert got.dtype == np.float32
        assert (d["err"] == 0).all()
        for k, (nid, i) in enumerate(items):
            np.testing.assert_array_equal(got[k], g["s%d" % i], err_msg="B=%d C=%d id=%r" % (B, C, nid))
            np.testing.assert_array_equal(d["board"][k], g["b%d" % i])
            assert int(d["turn"][k]) == int(g["t%d" % i])
            checked += 1
        np.testing.assert_array_equal(d["legal"].reshape(len(ids), B, B), (d["board"] == 0).astype(np.uint8))
        # bare move lists are the same positions
        with _batch(B, inplanes=C) as pb:
            d2 = pb.describe([nid[1:] for nid in ids], leading_zero=False)
        for key in d:
            np.testing.assert_array_equal(d[key], d2[key])
    assert checked == int(g["count"])


@pytest.mark.parametrize("B", [12, 13])
def test_planes_board_turn_legal_on_three_word_boards(B):
    """12x12 and 13x13 (bitboards of three 64-cell words, which gv3 does not hold): planes / board / turn / legal of random
    legal move lists whose lengths sit on the word seams (0, 1, 64, 65, 128, 129, A - 1) against the host's
    utils.get_state_pt / get_board / get_turn, C = 5 and C = 7, exactly. Finished games are encoded like any other."""
    from alpha_omok_amd import utils
    A = B * B
    rs = np.random.RandomState(40 + B)
    ids = [(0,) + tuple(rs.permutation(A)[:n].tolist()) for n in (0, 1, 64, 65, 128, 129, A - 1) for _ in range(2)]
    for C in (5, 7):
        with _batch(B, inplanes=C, capacity=8) as pb:        # (two chunks)
            got = pb.planes(ids).cpu().numpy()
            d = pb.describe(ids)
        assert got.dtype == np.float32 and got.shape == (len(ids), C, B, B) and (d["err"] == 0).all()
        for k, nid in enumerate(ids):
            np.testing.assert_array_equal(got[k], utils.get_state_pt(nid, B, C).astype(np.float32), err_msg="B=%d C=%d n=%d" % (B, C, len(nid) - 1))
            board = utils.get_board(nid, B)
            np.testing.assert_array_equal(d["board"][k], board.astype(np.int8))
            assert int(d["turn"][k]) == int(utils.get_turn(nid))
            np.testing.assert_array_equal(d["legal"][k].reshape(B, B), (board == 0).astype(np.uint8))


# ---------------------------------------------------------------------------------------------------------------------
# 5. errors are per position
# ---------------------------------------------------------------------------------------------------------------------
def test_errors_stay_with_their_position():
    B, A = 9, 81
    rs = np.random.RandomState(8)
    good = [(0,) + tuple(rs.permutation(A)[:n].tolist()) for n in (0, 1, 7, 30, 64, 65, 81)]
    bad = [((0, 3, 4, 3), 2),                                   # a repeated cell
           ((0, 5, -1, 6), 1),
           ((0, 5, 6, A), 1),
           ((0,) + tuple(range(A)) + (0,), 3),                  # longer than the board has cells
           ((0, 7, 7, -1), 2)]                                  # the first mistake is the one reported
    mixed, where_good = [], []
    for i, gid in enumerate(good):
        mixed.append(gid)
        where_good.append(len(mixed) - 1)
        if i < len(bad):
            mixed.append(bad[i][0])
    mixed += [b for b, _ in bad[len(good):]]
    where_bad = [i for i in range(len(mixed)) if i not in where_good]
    with _batch(B, capacity=4) as pb:                            # chunks that mix good and bad positions
        d = pb.describe(mixed)
        pl = pb.planes(mixed).cpu().numpy()
    with _batch(B) as pb:
        d0 = pb.describe(good)
        pl0 = pb.planes(good).cpu().numpy()
    assert d["err"][where_bad].tolist() == [c for _, c in bad]
    assert (d["err"][where_good] == 0).all() and (d0["err"] == 0).all()
    for key in d0:
        np.testing.assert_array_equal(d[key][where_good], d0[key], err_msg=key)
        if key != "err":
            assert not d[key][where_bad].any(), key            # a bad position's outputs are zeroed
    np.testing.assert_array_equal(pl[where_good], pl0)
    assert not pl[where_bad].any()
    assert d0["status"][-1] != 0 and d0["end_ply"][-1] >= 8     # (the 81-move game is over, and was before its last move)


# ---------------------------------------------------------------------------------------------------------------------
# 6. evaluate
# ---------------------------------------------------------------------------------------------------------------------
def _game_ids(B, n, seed, with_terminal=True):
    """n ids of random play of every length, among them finished games (a line of five, played on past it)."""
    rs = np.random.RandomState(seed)
    A = B * B
    ids = [(0,)]
    while len(ids) < n:
        ids.append((0,) + tuple(rs.permutation(A)[:rs.randint(1, A + 1)].tolist()))
    if with_terminal and n >= 4:
        five = [0, B, 1, B + 1, 2, B + 2, 3, B + 3, 4]                   # black's top row
        ids[1] = (0,) + tuple(five)
        ids[n // 2] = (0,) + tuple(five) + (B + 5, 40)                    # moves past the win
    return ids


@functools.lru_cache(maxsize=None)
def _model(nb, B):
    import torch
    from alpha_omok_amd import pvnet
    m = pvnet.PVNet(nb, 5, 128, B)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in net_reference.case_network(nb, B, 128).items()})
    return m.eval()


def _native_on_host_planes(net, ids, B, chunk):
    """The native forward fed get_state_pt planes built on the host, in chunks of `chunk` (the batch composition evaluate uses)."""
    import torch
    from alpha_omok_amd import utils
    x = torch.from_numpy(np.stack([utils.get_state_pt(i, B, 5) for i in ids]).astype(np.float32)).cuda()
    pol, val = [], []
    for a in range(0, len(ids), chunk):
        p, v = net(x[a:a + chunk])
        pol.append(p.cpu().numpy())
        val.append(v.cpu().numpy())
    return np.concatenate(pol), np.concatenate(val)


@pytest.mark.parametrize("nb,B", [(2, 9), (1, 15)])
def test_evaluate_is_the_native_forward_on_device_planes(nb, B):
    """evaluate(model, ids) == the native forward on the host-built planes of the same ids in the same batches, bit for
    bit: n = 1, 17, 200 in one chunk, 150 in chunks of 64 / 64 / 22. Finished games are evaluated like any other and
    reported by status; ZeroAgent.get_pv_batch is the same call."""
    from alpha_omok_amd import utils
    from alpha_omok_amd.agents import ZeroAgent
    model = _model(nb, B)
    agent = ZeroAgent(B, 4, 5, noise=False)
    agent.model = model
    net = agent._evaluator.native_net(model, B, 5)
    assert net is not None
    for n, cap in ((1, 4096), (17, 4096), (200, 4096), (150, 64)):
        ids = _game_ids(B, n, seed=n)
        want_p, want_v = _native_on_host_planes(net, ids, B, cap)
        with _batch(B, capacity=cap) as pb:
            pol, val, status, err = pb.evaluate(model if n == 17 else net, ids)   # (a module is exported once more: once is enough)
        assert pol.dtype == np.float32 and val.dtype == np.float32 and pol.shape == (n, B * B) and val.shape == (n,)
        assert (err == 0).all()
        np.testing.assert_array_equal(pol.view(np.uint32), want_p.view(np.uint32), err_msg="n=%d" % n)
        np.testing.assert_array_equal(val.view(np.uint32), want_v.view(np.uint32), err_msg="n=%d" % n)
        host_status = [utils.check_win(utils.get_board(i, B), 5) for i in ids]
        assert status.tolist() == host_status
        if n >= 4:
            assert status[1] == 1 and status[n // 2] == 1 and np.isfinite(pol[[1, n // 2]]).all()
        if cap == 4096:
            got = agent.get_pv_batch(ids)
            for a, b in zip(got, (pol, val, status, err)):
                np.testing.assert_array_equal(a, b)


def test_evaluate_bad_positions_do_not_disturb_their_chunk():
    """Positions with an error sit in the batch as empty boards and come back as zeros; the good ones next to them get
    what they get when the bad ones ARE empty boards (same batch composition, so the same kernels)."""
    B = 9
    model = _model(2, B)
    ids = _game_ids(B, 40, seed=40)
    bad_at = {5: (0, 3, 3), 22: (0, -1), 39: (0, 81)}
    mixed = [bad_at.get(i, rid) for i, rid in enumerate(ids)]
    empty = [(0,) if i in bad_at else rid for i, rid in enumerate(ids)]
    with _batch(B) as pb:
        pol, val, status, err = pb.evaluate(model, mixed)
        pol0, val0, status0, err0 = pb.evaluate(model, empty)
    assert err.tolist() == [{5: 2, 22: 1, 39: 1}.get(i, 0) for i in range(40)] and not err0.any()
    good = [i for i in range(40) if i not in bad_at]
    np.testing.assert_array_equal(pol[good].view(np.uint32), pol0[good].view(np.uint32))
    np.testing.assert_array_equal(val[good].view(np.uint32), val0[good].view(np.uint32))
    np.testing.assert_array_equal(status[good], status0[good])
    for i in bad_at:
        assert not pol[i].any() and val[i] == 0 and status[i] == 0
        assert pol0[i].sum() > 0.99                              # (the empty board itself has a policy)


def test_evaluate_refuses_a_network_of_another_shape():
    from alpha_omok_amd.engine import EngineError
    model = _model(2, 9)
    with _batch(9, inplanes=3) as pb:
        with pytest.raises(ValueError):
            pb.evaluate(model, [(0,)])                           # a 5-plane net for 3-plane positions
        net = model.to_native()
        with pytest.raises(EngineError, match="board/inplanes"):
            pb.evaluate(net, [(0,)])
        net.close()
