"""-m gpu: the switch that joins the solver and the bar -- Engine.search / Evaluator.search(tactics=...), ZeroAgent.get_pi and
evaluate_batched -- with an evaluator that knows nothing: uniform policy, value 0, S = 16. Whatever such a search gets
right about forced wins, it was told by root_tactics.

Roots: the fixture's first open positions of every verdict (RT_WIN, RT_DEFEND, RT_LOST, RT_NONE, two of each: 8 games) on
boards 6 and 9, at the fixture's own limits (depth 6, 2000 nodes), with test_root_tactics_host.expected as the yardstick."""
import numpy as np
import pytest

from test_forced_defence_host import DEPTH, MARK, NODES
from test_gpu_root_tactics import G, _verdict_roots

pytestmark = pytest.mark.gpu

S = 16
LIMITS = dict(max_depth=DEPTH, max_nodes=NODES)


class FlatModel:
    """Agent.model stand-in: every cell as likely as any other, every position worth nothing"""

    def __init__(self, A):
        self.A = A

    def eval(self):
        return self

    def __call__(self, x):
        import torch
        n = x.shape[0]
        return torch.full((n, self.A), 1.0 / self.A, dtype=torch.float32), torch.zeros(n, dtype=torch.float32)


def _search(B, roots, tactics, tau=0, seed0=40):
    from alpha_omok_amd.engine import Engine
    from alpha_omok_amd.evaluator import Evaluator
    eng = Engine(B, S, 5, games=G, noise=True, win_mark=MARK[B])
    eng.seed_all(np.arange(seed0, seed0 + G, dtype=np.uint32))
    eng.set_roots(roots)
    out = Evaluator(0).search(eng, FlatModel(B * B), tau, tactics=tactics)
    return eng, out


@pytest.mark.parametrize("B", (6, 9))
def test_tactics_restrict_what_is_proven_and_nothing_else(B):
    from alpha_omok_amd import utils
    roots, want = _verdict_roots(B)
    plain, (ppi, pvis, ppol) = _search(B, roots, None)
    assert plain.last_tactics() is None
    eng, (pi, vis, pol) = _search(B, roots, dict(LIMITS))
    rt = eng.last_tactics()
    for key in want:
        np.testing.assert_array_equal(rt[key], want[key], err_msg=key)
    np.testing.assert_array_equal(pol, ppol)                      # the priors are the network's, bar or no bar
    played = pi.argmax(axis=1)
    for g in range(G):
        v, tag = want["verdict"][g], "board %d game %d verdict %d" % (B, g, want["verdict"][g])
        if v in (utils.RT_WIN, utils.RT_DEFEND):
            assert want["allowed"][g][played[g]], tag
            assert not pi[g][~want["allowed"][g]].any() and not vis[g][~want["allowed"][g]].any(), tag
            assert vis[g].sum() == S, tag
        else:                                                     # RT_LOST and RT_NONE: the plain search, bit for bit
            np.testing.assert_array_equal(pi[g], ppi[g], err_msg=tag)
            np.testing.assert_array_equal(vis[g], pvis[g], err_msg=tag)
            a, b = eng.get_rng_state(g), plain.get_rng_state(g)
            assert a[1] == b[1] and np.array_equal(a[0], b[0]), tag
    ran = eng.sims_run()["sims"]
    assert (ran == S).all()
    eng.close()
    plain.close()


def test_solved_sims_cut_a_proven_win_to_one_simulation():
    from alpha_omok_amd import utils
    B = 9
    roots, want = _verdict_roots(B)
    eng, (pi, vis, _) = _search(B, roots, dict(LIMITS, solved_sims=1))
    ran = eng.sims_run()["sims"]
    won = want["verdict"] == utils.RT_WIN
    assert won.any() and (ran[won] == 1).all() and (ran[~won] == S).all()
    for g in np.flatnonzero(won):                                 # one visit among the winning first moves: a one-hot pi
        assert vis[g].sum() == 1 and pi[g].max() == 1 and want["allowed"][g][pi[g].argmax()]
    with pytest.raises(ValueError):
        eng.search(None, tactics=dict(solved_sims=0))
    with pytest.raises(ValueError):
        eng.search(None, tactics=dict(depth=3))
    eng.close()


def test_allowed_and_tactics_intersect():
    """the caller allows only what the solver forbids in a DEFEND game and one winning move in a WIN game"""
    from alpha_omok_amd import utils
    from alpha_omok_amd.engine import Engine
    from alpha_omok_amd.evaluator import Evaluator
    B = 9
    A = B * B
    roots, want = _verdict_roots(B)
    empty = np.array([~np.isin(np.arange(A), r[1:]) for r in roots])
    mine = np.ones((G, A), bool)
    d = int(np.flatnonzero(want["verdict"] == utils.RT_DEFEND)[0])
    w = int(np.flatnonzero(want["verdict"] == utils.RT_WIN)[0])
    mine[d] = ~want["allowed"][d]
    assert (mine[d] & empty[d]).any()
    first = int(np.flatnonzero(want["allowed"][w])[0])
    mine[w] = empty[w] & ~want["allowed"][w]
    mine[w, first] = True
    eng = Engine(B, S, 5, games=G, noise=False, win_mark=MARK[B])
    eng.set_roots(roots)
    pi, vis, _ = Evaluator(0).search(eng, FlatModel(A), 0, allowed=mine, tactics=dict(LIMITS))
    assert not vis[d][~mine[d]].any() and vis[d].sum() == S       # an empty intersection: the caller's row stands
    assert vis[w][first] == S                                     # the one winning move the caller allows
    eng.close()


@pytest.mark.parametrize("B", (6, 9))
def test_zero_agent_get_pi_and_get_root_tactics(B):
    from alpha_omok_amd import utils
    from alpha_omok_amd.agents import ZeroAgent
    roots, want = _verdict_roots(B, 4)
    ag = ZeroAgent(B, S, 5, noise=False)
    ag.win_mark = MARK[B]
    ag.model = FlatModel(B * B)
    for g, root in enumerate(roots):
        verdict, depth, allowed, nodes, unknown = ag.get_root_tactics(root, **LIMITS)
        assert (verdict, depth, nodes, unknown) == tuple(int(want[k][g]) for k in ("verdict", "depth", "nodes", "unknown"))
        np.testing.assert_array_equal(allowed.ravel(), want["allowed"][g])
        pi = ag.get_pi(root, 0, tactics=dict(LIMITS))
        assert ag.last_tactics["verdict"][0] == verdict
        if verdict in (utils.RT_WIN, utils.RT_DEFEND):
            assert want["allowed"][g][pi.argmax()] and not ag.visit[~want["allowed"][g]].any()
        pi = ag.get_pi(root, 0, allowed=np.flatnonzero(want["allowed"][g])[:1].tolist())     # a list of cells
        assert pi.argmax() == np.flatnonzero(want["allowed"][g])[0] and ag.last_tactics is None


def test_evaluate_batched_with_tactics_never_walks_into_a_proven_loss():
    """Two matches of a know-nothing network against itself, the player's side with the switch, 40 plies at the most. Every
    position is put to utils.forced_defences afterwards at the same limits: where the opponent threatened a forced win and
    a reply that is not proven to lose existed, the side with the switch did not play one that is."""
    from alpha_omok_amd import utils
    from alpha_omok_amd.evaluate import evaluate_batched
    B, limits = 9, dict(max_depth=6, max_nodes=512)
    model = FlatModel(B * B)
    _, _, games = evaluate_batched(model, model, B, S, n_match=2, seed=5, max_plies=40, tactics=(dict(limits), None))
    assert len(games) == 2
    checked = threats = 0
    for i, (_, moves) in enumerate(games):
        for t in range(len(moves)):
            if (t % 2 == 0) != (i % 2 == 0):                      # match 0: the player (the side with the switch) is black
                continue
            d = utils.forced_defences(moves[:t], B, 5, **limits)
            checked += 1
            if d["status"] != 0 or d["threat"] != utils.FW_WIN:
                continue
            threats += 1
            holds = (d["reply"] == utils.FD_SAFE) | (d["reply"] == utils.FD_UNKNOWN)
            if holds.any():
                assert d["reply"][moves[t]] != utils.FD_LOSES, "match %d ply %d: %d loses although %s hold" % (
                    i, t, moves[t], np.flatnonzero(holds).tolist())
    print("positions of the side with the switch: %d, under a proven threat: %d" % (checked, threats))
    assert checked > 0
