"""-m gpu: Engine.root_tactics (k_root_tactics_a / _b / k_root_tactics_rows on the engine's own root positions) against the
host definition utils.root_tactics, entry for entry, `nodes` and `unknown` included.

The positions are the fixture of test_forced_defence_host, set with set_roots on engines of 8 games and worked through in
rounds: boards 3, 5, 6, 8, 9 and 15 (NCH = 1, 2 and 4) at depth 6 / 2000 nodes, 9x9 also at 50 nodes where searches run
out; the expected rows are test_root_tactics_host.expected (the recorded forced_defences rows + two live searches per
position, itself held to the live host there). NCH = 3: six prefixes of a hand-made 12x12 game against the live host."""
import numpy as np
import pytest

from test_forced_defence_host import CASES, DEPTH, MARK, NODES, SMALL_BOARD, SMALL_NODES, STEP
from test_root_tactics_host import KEYS, NCH3_BOARD, NCH3_MARK, expected, host_rows, nch3_ids

pytestmark = pytest.mark.gpu

G = 8


def device_rows(B, mark, ids, max_nodes, max_depth=DEPTH, sims=4):
    """Engine.root_tactics of the positions `ids`, eight at a time on one engine"""
    from alpha_omok_amd.engine import Engine
    eng = Engine(B, sims, 5, games=G, noise=False, win_mark=mark)
    out = {key: [] for key in KEYS}
    for first in range(0, len(ids), G):
        chunk = list(ids[first:first + G])
        n = len(chunk)
        assert (eng.set_roots(chunk + [(0,)] * (G - n)) >= 0).all()
        r = eng.root_tactics(max_depth=max_depth, max_nodes=max_nodes)
        for key in KEYS:
            out[key].append(r[key][:n])
    eng.close()
    return {key: np.concatenate(v) for key, v in out.items()}


def _rows_of(B, n):
    return list(range(n)) if B < SMALL_BOARD else list(range(0, n, STEP))


@pytest.mark.parametrize("B", [b for b, _, _ in CASES])
def test_fixture_positions_equal_the_host(B):
    ids, want = expected(B)
    rows = _rows_of(B, len(ids))
    got = device_rows(B, MARK[B], [ids[i] for i in rows], NODES)
    for key in KEYS:
        np.testing.assert_array_equal(got[key], want[key][rows], err_msg="board %d: %s" % (B, key))


def test_small_budget_equals_the_host():
    """9x9 at 50 nodes: every unknown bit occurs among the compared positions"""
    B = SMALL_BOARD
    ids, want = expected(B, small=True)
    rows = sorted(set(_rows_of(B, len(ids))) | set(np.flatnonzero(want["unknown"] & 4)[:4].tolist()))
    got = device_rows(B, MARK[B], [ids[i] for i in rows], SMALL_NODES)
    for key in KEYS:
        np.testing.assert_array_equal(got[key], want[key][rows], err_msg="9x9 at %d nodes: %s" % (SMALL_NODES, key))
    for bit in (1, 2, 4):
        assert (got["unknown"] & bit).any()


def test_nch3_prefixes_equal_the_live_host():
    ids = nch3_ids()
    want = host_rows(NCH3_BOARD, ids, 512, 6, NCH3_MARK)
    got = device_rows(NCH3_BOARD, NCH3_MARK, ids, 512, 6)
    for key in KEYS:
        np.testing.assert_array_equal(got[key], want[key], err_msg="12x12: %s" % key)


def _verdict_roots(B, count=G):
    """the fixture's first open positions of every verdict on board B, WIN / DEFEND / LOST / NONE in turn"""
    from alpha_omok_amd import utils
    ids, want = expected(B)
    open_ = np.array([want["nodes"][i] > 0 for i in range(len(ids))])
    per = [np.flatnonzero((want["verdict"] == v) & open_) for v in (utils.RT_WIN, utils.RT_DEFEND, utils.RT_LOST, utils.RT_NONE)]
    pick = [int(per[k % 4][k // 4]) for k in range(count)]
    return [ids[i] for i in pick], {key: want[key][pick] for key in KEYS}


def test_inactive_games_get_zeros_and_cost_nothing():
    from alpha_omok_amd.engine import Engine
    B = 9
    roots, want = _verdict_roots(B)
    eng = Engine(B, 4, 5, games=G, noise=False, win_mark=MARK[B])
    eng.set_roots(roots)
    active = np.array([1, 0, 1, 0, 0, 1, 1, 0], np.uint8)
    r = eng.root_tactics(active=active, max_depth=DEPTH, max_nodes=NODES)
    on = active != 0
    for key in KEYS:
        np.testing.assert_array_equal(r[key][on], want[key][on], err_msg=key)
        assert not r[key][~on].any(), key
    with pytest.raises(ValueError):
        eng.root_tactics(max_depth=17)
    with pytest.raises(ValueError):
        eng.root_tactics(max_nodes=0)
    eng.close()


@pytest.mark.parametrize("B", (6, 9))
def test_apply_leaves_the_bar_of_begin_move_allowed(B):
    """root_tactics(apply=True) then begin_move() against begin_move(allowed=result["allowed"]) on a twin, on EXPANDED roots:
    the same root_children, sentinels included; and with a caller's bar pending the two intersect, a game whose intersection
    is empty keeping the caller's."""
    from alpha_omok_amd import utils
    from alpha_omok_amd.engine import BAR_Q, Engine
    from gpu_helpers import HostEvalRunner
    A, S = B * B, 8
    roots, want = _verdict_roots(B)
    flat = np.full(A, np.float32(1.0 / A), np.float32)
    ev = lambda g, sim, planes: (flat, np.float32(0.0))
    engines = []
    for _ in range(4):
        eng = Engine(B, S, 5, games=G, noise=False, win_mark=MARK[B])
        eng.set_roots(roots)
        run = HostEvalRunner(eng)
        run.move(ev, tau=np.ones(G, np.int8))                   # the roots are expanded and hold visits
        engines.append((eng, run))
    (ea, ra), (eb, rb), (ec, rc), (ed, rd) = engines
    rt = ea.root_tactics(max_depth=DEPTH, max_nodes=NODES, apply=True)
    for key in KEYS:
        np.testing.assert_array_equal(rt[key], want[key], err_msg=key)
    ea.begin_move()
    eb.begin_move(allowed=rt["allowed"])
    bar = utils.root_bar(rt["allowed"], roots, B)
    assert bar.any()
    for g in range(G):
        ca, cb = ea.root_children(g), eb.root_children(g)
        for key in ca:
            np.testing.assert_array_equal(ca[key], cb[key], err_msg="game %d: %s" % (g, key))
        np.testing.assert_array_equal(ca["q"] == BAR_Q, bar[g][ca["action"]])
    # a caller's bar on top: the lower half of the board only, except game 1 whose row is the complement of what the solver allows
    mine = np.zeros((G, A), np.uint8)
    mine[:, :A // 2 + B] = 1
    defend = int(np.flatnonzero(want["verdict"] == utils.RT_DEFEND)[0])
    mine[defend] = ~rt["allowed"][defend]
    both = mine.astype(bool) & rt["allowed"]
    empty = np.array([~np.isin(np.arange(A), r[1:]) for r in roots])
    keep = ~(both & empty).any(axis=1)                           # nothing left: the caller's row stands
    assert keep[defend] and not keep.all() and (mine.astype(bool) & empty).any(axis=1).all()
    both[keep] = mine[keep].astype(bool)
    ec.set_root_bar(mine)
    ec.root_tactics(max_depth=DEPTH, max_nodes=NODES, apply=True)
    ec.begin_move()
    ed.begin_move(allowed=both)
    for g in range(G):
        cc, cd = ec.root_children(g), ed.root_children(g)
        for key in cc:
            np.testing.assert_array_equal(cc[key], cd[key], err_msg="intersection, game %d: %s" % (g, key))
    for eng, _ in engines:
        eng.close()
