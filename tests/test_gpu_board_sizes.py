"""-m gpu: the tree kernels on EVERY board size 3 .. 15 against the CPU oracle, from mid-game roots.

Every tree kernel is a template on NCH = ceil(B * B / 64) 64-cell chunks, and the child order of a node is CPython's set
difference, emulated on the device (tree_device.hpp, legal_order): ascending until the result's hash table is smaller than
its largest key. At which stone counts that happens depends on the board size (test_oracle_golden.NONASC_RANGE, measured
with the live CPython set): on 12x12 from 68 stones on -- 47 % of the board --, on 6x6 from 18. The other parity tests start
from the empty board or from 9x9 / 15x15 endgames; here every board size is searched from roots inside its range, the first
stone count of the range (where the emulation's table-size thresholds L <= 4 / 18 / 76 sit) among them.

Roots are five-free by construction: both colours' stones are drawn from the colouring ((c // 2) + r) % 2 (runs of two along
rows, alternating along columns; no three in a line in any direction), black on 0, white on 1, the moves interleaved.

4x4: Engine takes its default mark 5 there (above the board size: no line wins), PositionBatch refuses mark 5 on a 4x4 board
(a mark has to fit the board). The two layers disagree on the default, so 4x4 is searched with mark 4, which both accept."""
import numpy as np
import pytest

from conftest import load_golden
from gpu_helpers import HostEvalRunner, children_by_action
from test_gpu_tree_parity import _run_golden_cases
from test_oracle_golden import NONASC_RANGE

pytestmark = pytest.mark.gpu

# stones of the four mid-game roots per board: the first count of the board's non-ascending range, then counts inside it
ROOT_STONES = {3: (5, 5, 6, 6), 4: (12, 12, 13, 13), 5: (21, 21, 22, 22), 6: (18, 24, 28, 32), 7: (31, 33, 40, 45), 8: (46, 48, 55, 60),
               9: (63, 66, 70, 76), 10: (82, 84, 90, 96), 11: (103, 104, 110, 118), 12: (68, 70, 100, 130), 13: (93, 95, 130, 160),
               14: (120, 122, 150, 190), 15: (149, 152, 180, 220)}


def _win_mark(B):
    """(mark handed to Engine: 0 = its default, the mark that default is -- what the oracle is told)."""
    if B == 4:
        return 4, 4
    return 0, (3 if B == 3 else 5)


def _mid_game_root(oracle, B, n_stones, wm, rs):
    """A root id of n_stones stones from the line-free colouring, black first; drawn again (up to 300 times) until the
    oracle lists its free cells in non-ascending order -- the oracle equals the live CPython order at every size and count
    (test_oracle_golden.test_legal_order_matches_live_cpython)."""
    cells = [(r * B + c, ((c // 2) + r) % 2) for r in range(B) for c in range(B)]
    black = [a for a, col in cells if col == 0]
    white = [a for a, col in cells if col == 1]
    nid = None
    for _ in range(300):
        bsel = rs.permutation(black)[:(n_stones + 1) // 2].tolist()
        wsel = rs.permutation(white)[:n_stones // 2].tolist()
        mv = [x for pair in zip(bsel, wsel) for x in pair] + bsel[len(wsel):]
        assert len(mv) == n_stones and oracle.check_win(oracle.get_board(mv, B), wm) == 0
        nid = (0,) + tuple(int(a) for a in mv)
        order = oracle.legal_actions(mv, B).tolist()
        if order != sorted(order):
            break
    return nid


@pytest.mark.parametrize("B", list(range(3, 16)))
def test_search_from_mid_game_roots_vs_oracle(oracle, B):
    """6 games, noise on, stub evaluator B % 3, 40 simulations, 3 plies (tau 1, 1, 0): two games from the empty board, four
    from mid-game roots (set_roots) inside the board's non-ascending range. After every move, against the oracle bit for bit:
    visits, post-noise priors, pi; the root's children -- order, w, q; the chosen action and win; the MT19937 position and its
    624 state words. At least one compared root per board lists its children in non-ascending order."""
    from alpha_omok_amd.engine import Engine
    G, S, PLIES, mode = 6, 40, 3, B % 3
    A = B * B
    mark, wm = _win_mark(B)
    first, last = NONASC_RANGE[B]
    assert len(ROOT_STONES[B]) == 4 and ROOT_STONES[B][0] == first and all(first <= n <= last for n in ROOT_STONES[B])
    rs = np.random.RandomState(900 + B)
    roots = [(0,), (0,)] + [_mid_game_root(oracle, B, n, wm, rs) for n in ROOT_STONES[B]]
    eng = Engine(B, S, 5, games=G, noise=True, win_mark=mark)
    run = HostEvalRunner(eng)
    seeds = [3000 + 100 * B + 7 * g for g in range(G)]
    eng.seed_all(seeds)
    assert (eng.set_roots(roots) == 0).all()                     # nothing was known: fresh roots
    agents = [oracle.Agent(B, S, 5, noise=True, evaluator="stub%d" % mode) for _ in range(G)]
    for g in range(G):
        agents[g].seed(seeds[g])
        agents[g].set_win_mark(wm)
    alive = np.ones(G, np.uint8)
    nonasc = compared = 0
    for t in range(PLIES):
        if not alive.any():
            break
        tau = np.full(G, 1 if t < 2 else 0, np.int8)
        pi, vis, pol = run.move(lambda g, sim, planes: oracle.stub_eval(planes, mode), tau=tau, active=alive)
        kids = [children_by_action(eng.root_children(g), A) if alive[g] else None for g in range(G)]
        act, win = eng.play()
        for g in range(G):
            if not alive[g]:
                continue
            tag = "board %d game %d ply %d (%d stones)" % (B, g, t, len(roots[g]) - 1)
            opi, ovis, opol = agents[g].get_pi(roots[g], int(tau[g]))
            np.testing.assert_array_equal(vis[g], ovis, err_msg="visit " + tag)
            np.testing.assert_array_equal(pol[g], opol, err_msg="policy " + tag)
            np.testing.assert_array_equal(pi[g], opi, err_msg="pi " + tag)
            och = agents[g].children(roots[g])
            assert kids[g]["order"].tolist() == och["order"].tolist(), "child order " + tag
            np.testing.assert_array_equal(kids[g]["w"], och["w"], err_msg="w " + tag)
            np.testing.assert_array_equal(kids[g]["q"], och["q"], err_msg="q " + tag)
            nonasc += int(och["order"].tolist() != sorted(och["order"].tolist()))
            compared += 1
            oa = agents[g].rng.choice_p(opi)
            assert act[g] == oa, "action " + tag
            roots[g] = roots[g] + (int(oa),)
            mt, pos, _, _ = eng.get_rng_state(g)
            assert pos == agents[g].rng.pos, "mt position " + tag
            np.testing.assert_array_equal(mt, agents[g].rng.state_words(), err_msg="mt " + tag)
            ow = oracle.check_win(oracle.get_board(list(roots[g])[1:], B), wm)
            assert win[g] == ow, "win " + tag
            if ow != 0:
                alive[g] = 0
    eng.close()
    assert compared >= G and nonasc >= 1, (compared, nonasc)


def test_golden_mid_sizes(oracle):
    """The reference's own searches from a 6x6 root with 24 stones, 12x12 roots with 70 and 100 and a 13x13 root with 95
    (tests/golden/gv5_tree_stub_midsizes.npz): every root lists its children in non-ascending order."""
    g = load_golden("gv5_tree_stub_midsizes")
    assert sorted(set(g["meta"][:, 0].tolist())) == [6, 12, 13]
    _run_golden_cases(oracle, g, lambda ci, mode: (lambda gi, sim, pl: oracle.stub_eval(pl, mode)))
