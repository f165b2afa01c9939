"""-m gpu: per-game simulation budgets, per-game noise and settling (k_settle) on the STEP-WISE protocol, against the CPU oracle.

A game's search is strictly sequential, so a budget-k search is the first k simulations of the budget-S search from the same
stream: oracle.Agent(B, k, ...) is the yardstick for every budget and for every search that settling or a stop ended after k
simulations. Boards 5, 9, 12 and 15 give NCH = 1, 2, 3 and 4 64-cell chunks: every instantiation of k_settle. S = 40, 8 games."""
import numpy as np
import pytest

from gpu_helpers import HostEvalRunner, children_by_action
from test_gpu_board_sizes import ROOT_STONES, _mid_game_root, _win_mark

pytestmark = pytest.mark.gpu

S, G = 40, 8
BOARDS = (5, 9, 12, 15)
BUDGETS = (1, 2, 3, 7, 16, 23, 39, 40)


class Runner(HostEvalRunner):
    """HostEvalRunner.move with the arguments of begin_move, a settle call after every apply_evals (settle_mask) and a stop after
    a given number of launches (stop_after)."""

    def move_opts(self, eval_fn, tau=None, active=None, sims=None, noise=None, settle_mask=None, stop_after=None):
        e, torch = self.e, self.torch
        e.begin_move(active, sims=sims, noise=noise)
        sim = 0
        while e.sims_left() > 0:
            e.collect_leaves(self.planes.data_ptr())
            e.sync()
            pl = self.planes.cpu().numpy()
            for g in range(e.G):
                if active is not None and not active[g]:
                    continue
                p, v = eval_fn(g, sim, pl[g])
                self.h_policy[g] = p
                self.h_value[g] = v
            self.policy.copy_(torch.from_numpy(self.h_policy))
            self.value.copy_(torch.from_numpy(self.h_value))
            torch.cuda.synchronize()
            e.apply_evals(self.policy.data_ptr(), self.value.data_ptr())
            sim += 1
            if settle_mask is not None:
                e.settle(settle_mask)
            if stop_after is not None and sim == stop_after:
                assert e.settle(stop=True) == 0 and e.sims_left() == 0
        return e.end_move(tau)


def _roots(oracle, B, wm, rs, n_empty=2):
    stones = list(ROOT_STONES[B]) + [ROOT_STONES[B][1], ROOT_STONES[B][2]]
    return [(0,)] * n_empty + [_mid_game_root(oracle, B, n, wm, rs) for n in stones[:G - n_empty]]


def _check_game(oracle, eng, agent, g, root, tau, out, kids, act, win, wm, tag):
    """Everything a move hands out for game g against the oracle agent's search of `root`, bit for bit; returns the new root."""
    B, A = eng.board_size, eng.A
    pi, vis, pol = out
    opi, ovis, opol = agent.get_pi(root, int(tau))
    np.testing.assert_array_equal(vis[g], ovis, err_msg="visit " + tag)
    np.testing.assert_array_equal(pol[g], opol, err_msg="policy " + tag)
    np.testing.assert_array_equal(pi[g], opi, err_msg="pi " + tag)
    och = agent.children(root)
    assert kids["order"].tolist() == och["order"].tolist(), "child order " + tag
    np.testing.assert_array_equal(kids["w"], och["w"], err_msg="w " + tag)
    np.testing.assert_array_equal(kids["q"], och["q"], err_msg="q " + tag)
    oa = agent.rng.choice_p(opi)
    assert act[g] == oa, "action " + tag
    root = root + (int(oa),)
    mt, pos, _, _ = eng.get_rng_state(g)
    assert pos == agent.rng.pos, "mt position " + tag
    np.testing.assert_array_equal(mt, agent.rng.state_words(), err_msg="mt " + tag)
    ow = oracle.check_win(oracle.get_board(list(root)[1:], B), wm)
    assert win[g] == ow, "win " + tag
    return root, ow


def _play_vs_oracle(oracle, B, sims, noise_engine, noise_games, plies=3, seed0=0):
    """`plies` moves (tau 1, 1, 0) of 8 games on one engine, game g with sims[g] simulations (None: S) and noise_games[g]
    (None: the engine's), each against its own oracle agent created with exactly that budget and noise switch."""
    from alpha_omok_amd.engine import Engine
    A, mode = B * B, B % 3
    mark, wm = _win_mark(B)
    rs = np.random.RandomState(1700 + B + seed0)
    roots = _roots(oracle, B, wm, rs)
    eng = Engine(B, S, 5, games=G, noise=noise_engine, win_mark=mark)
    run = Runner(eng)
    seeds = [7000 + 100 * B + 11 * g + seed0 for g in range(G)]
    eng.seed_all(seeds)
    assert (eng.set_roots(roots) == 0).all()
    agents = []
    for g in range(G):
        ng = noise_engine if noise_games is None else bool(noise_games[g])
        a = oracle.Agent(B, S if sims is None else int(sims[g]), 5, noise=ng, evaluator="stub%d" % mode)
        a.seed(seeds[g])
        a.set_win_mark(wm)
        agents.append(a)
    alive = np.ones(G, np.uint8)
    compared = 0
    for t in range(plies):
        if not alive.any():
            break
        tau = np.full(G, 1 if t < 2 else 0, np.int8)
        out = run.move_opts(lambda g, sim, planes: oracle.stub_eval(planes, mode), tau=tau, active=alive, sims=sims, noise=noise_games)
        ran = eng.sims_run()
        kids = [children_by_action(eng.root_children(g), A) if alive[g] else None for g in range(G)]
        act, win = eng.play()
        for g in range(G):
            if not alive[g]:
                assert ran["sims"][g] == 0
                continue
            tag = "board %d game %d ply %d (%d stones, budget %s)" % (B, g, t, len(roots[g]) - 1, "S" if sims is None else sims[g])
            assert ran["sims"][g] == (S if sims is None else sims[g]) and not ran["settled"][g], tag
            roots[g], ow = _check_game(oracle, eng, agents[g], g, roots[g], tau[g], out, kids[g], act, win, wm, tag)
            compared += 1
            if ow != 0:
                alive[g] = 0
    eng.close()
    assert compared >= G


@pytest.mark.parametrize("B", BOARDS)
def test_per_game_budgets_vs_oracle(oracle, B):
    """Budgets {1, 2, 3, 7, 16, 23, 39, 40} side by side in one launch sequence, noise on; two games from the empty board, six
    from mid-game roots; three plies. Visits, post-noise priors, pi, the root children's order, w, q, action, win and the
    MT19937 stream after every move equal oracle.Agent(B, budget)."""
    _play_vs_oracle(oracle, B, np.array(BUDGETS, np.int32), True, None)


@pytest.mark.parametrize("B", (9, 15))
def test_per_game_noise_vs_oracle(oracle, B):
    """On a noise=True engine the games with noise[g] = 0 equal oracle.Agent(noise=False) -- no draw, no re-noise at the inherited
    roots of plies 2 and 3, stream untouched by either -- while their neighbours in the same launches equal noise=True agents;
    with budgets of their own on top."""
    noise = np.array([1, 0, 0, 1, 0, 1, 1, 0], np.uint8)
    _play_vs_oracle(oracle, B, None, True, noise, seed0=1)
    _play_vs_oracle(oracle, B, np.array(BUDGETS[::-1], np.int32), True, noise, seed0=2)


def test_full_budgets_equal_the_plain_call(oracle):
    """sims = num_mcts and noise = 1 everywhere: the same bits as begin_move without them, over two plies."""
    from alpha_omok_amd.engine import Engine
    B, mode = 9, 0
    mark, wm = _win_mark(B)
    roots = _roots(oracle, B, wm, np.random.RandomState(31))
    res = []
    for opts in (False, True):
        eng = Engine(B, S, 5, games=G, noise=True, win_mark=mark)
        run = Runner(eng)
        eng.seed_all(np.arange(400, 400 + G))
        eng.set_roots(roots)
        got = []
        for t in range(2):
            ev = lambda g, sim, planes: oracle.stub_eval(planes, mode)
            if opts:
                out = run.move_opts(ev, tau=np.ones(G, np.int8), sims=np.full(G, S, np.int32), noise=np.ones(G, np.uint8))
            else:
                out = run.move(ev, tau=np.ones(G, np.int8))
            got.append(out + eng.play() + tuple(eng.get_rng_state(g)[0] for g in range(G)))
        res.append(got)
        eng.close()
    for a, b in zip(res[0], res[1]):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)


def _peaked(A, cell):
    p = np.full(A, np.float32(0.1) / np.float32(A - 1), np.float32)
    p[cell] = np.float32(0.9)
    return p


def _settle_plan(oracle, B):
    """The games of the settling test and what the oracle ALONE says about them: game g is peaked (policy 0.9 on one legal cell
    of its root, flat elsewhere, value 0) for g < 4 and the stub otherwise; games 2, 3, 6, 7 search without noise; even games
    start from the empty board, odd ones from mid-game roots. Returns roots, evaluators, noise switches, seeds, and per game the
    smallest k in 1..S at which utils.move_decided holds for the budget-k visits (S if none) with that budget's agent."""
    from alpha_omok_amd.utils import move_decided
    A, mode = B * B, B % 3
    mark, wm = _win_mark(B)
    rs = np.random.RandomState(2300 + B)
    stones = ROOT_STONES[B]
    roots = [(0,) if g % 2 == 0 else _mid_game_root(oracle, B, stones[g // 2], wm, rs) for g in range(G)]
    noise = np.array([1, 1, 0, 0, 1, 1, 0, 0], np.uint8)
    seeds = [9100 + 10 * B + g for g in range(G)]
    evals = []
    for g in range(G):
        if g < 4:
            free = [a for a in range(A) if a not in roots[g][1:]]
            pol = _peaked(A, free[(3 * g + 1) % len(free)])
            evals.append(lambda planes, pol=pol: (pol, np.float32(0.0)))
        else:
            evals.append(lambda planes: oracle.stub_eval(planes, mode))
    first_k, agents, full_vis = [], [], []
    for g in range(G):
        found = None
        for k in range(1, S + 1):
            a = oracle.Agent(B, k, 5, noise=bool(noise[g]), evaluator=lambda mv, pl, sim, f=evals[g]: f(pl))
            a.seed(seeds[g])
            a.set_win_mark(wm)
            rng0 = (a.rng.state_words(), a.rng.pos)
            _, vis, _ = a.get_pi(roots[g], 0)
            if k == S:
                full_vis.append(vis.copy())
            if found is None and (move_decided(vis, S - k) or k == S):
                found = k
                # a fresh agent of that budget, its search not yet run: the test runs it through _check_game
                b = oracle.Agent(B, k, 5, noise=bool(noise[g]), evaluator=lambda mv, pl, sim, f=evals[g]: f(pl))
                b.rng.set_state(*rng0)
                b.set_win_mark(wm)
                agents.append(b)
        first_k.append(found)
    return roots, evals, noise, seeds, first_k, agents, full_vis


@pytest.mark.parametrize("B", BOARDS)
def test_settling_stepwise_vs_oracle(oracle, B):
    """settle(mask) after every apply_evals, tau 0: every masked game stops at the first k at which its move is decided
    (sims_run == the oracle's first k, the full budget if there is none) and hands out exactly the budget-k oracle search --
    visits, pi, children, stream, action. Game 3 is not in the mask and runs all S simulations although its move was decided
    long before. The move a settled game returns is the argmax of the full-budget oracle visits."""
    from alpha_omok_amd.engine import Engine
    A = B * B
    mark, wm = _win_mark(B)
    roots, evals, noise, seeds, first_k, agents, full_vis = _settle_plan(oracle, B)
    mask = np.ones(G, np.uint8)
    mask[3] = 0
    want = [first_k[g] if mask[g] else S for g in range(G)]
    print("board %d: first decided k per game %s, run %s" % (B, first_k, want))
    # what the inputs must be for the test to mean anything (the oracle alone says so)
    assert sum(1 for g in range(G) if mask[g] and first_k[g] < S) >= G // 4
    assert any(mask[g] and first_k[g] == S for g in range(G))                # a game that runs to its end
    assert first_k[3] < S
    if not mask[3]:   # the unmasked game is compared with the full-budget agent
        b = oracle.Agent(B, S, 5, noise=bool(noise[3]), evaluator=lambda mv, pl, sim, f=evals[3]: f(pl))
        b.seed(seeds[3])
        b.set_win_mark(wm)
        agents[3] = b
    eng = Engine(B, S, 5, games=G, noise=True, win_mark=mark)
    run = Runner(eng)
    eng.seed_all(seeds)
    assert (eng.set_roots(roots) == 0).all()
    tau = np.zeros(G, np.int8)
    out = run.move_opts(lambda g, sim, planes: evals[g](planes), tau=tau, noise=noise, settle_mask=mask)
    ran = eng.sims_run()
    kids = [children_by_action(eng.root_children(g), A) for g in range(G)]
    act, win = eng.play()
    assert ran["sims"].tolist() == want
    assert ran["settled"].tolist() == [bool(mask[g]) and first_k[g] < S for g in range(G)]
    assert ran["settled_total"] == int(ran["settled"].sum()) and ran["saved_total"] == sum(S - w for w in want)
    for g in range(G):
        tag = "board %d game %d (settled after %d)" % (B, g, want[g])
        _check_game(oracle, eng, agents[g], g, roots[g], 0, out, kids[g], act, win, wm, tag)
        if ran["settled"][g]:
            assert int(np.argmax(out[0][g])) == int(np.argmax(full_vis[g])), "move of the full search " + tag
            assert int((full_vis[g] == full_vis[g].max()).sum()) == 1
    eng.close()


@pytest.mark.parametrize("B", (9, 12))
def test_stop_now_stepwise_vs_oracle(oracle, B):
    """After k = 13 of 40 launches settle(stop=True) ends the move: end_move hands out the budget-k oracle search (a fresh root
    has run its own expansion and k - 1 simulations by then: budget k - 1) without ERR_SHORT. A plain short end_move still
    raises, and the engine searches correctly afterwards."""
    from alpha_omok_amd.engine import Engine, EngineError
    A, mode, K = B * B, B % 3, 13
    mark, wm = _win_mark(B)
    rs = np.random.RandomState(77 + B)
    roots = _roots(oracle, B, wm, rs)
    eng = Engine(B, S, 5, games=G, noise=True, win_mark=mark)
    run = Runner(eng)
    seeds = [5100 + g for g in range(G)]
    ev = lambda g, sim, planes: oracle.stub_eval(planes, mode)

    def agents_for(budgets):
        out = []
        for g in range(G):
            a = oracle.Agent(B, budgets[g], 5, noise=True, evaluator="stub%d" % mode)
            a.seed(seeds[g])
            a.set_win_mark(wm)
            out.append(a)
        return out

    eng.seed_all(seeds)
    assert (eng.set_roots(roots) == 0).all()                     # all fresh: the first launch is the root's expansion
    tau = np.array([1, 0] * (G // 2), np.int8)
    out = run.move_opts(ev, tau=tau, stop_after=K)
    ran = eng.sims_run()
    assert ran["sims"].tolist() == [K - 1] * G and ran["settled"].all()
    kids = [children_by_action(eng.root_children(g), A) for g in range(G)]
    act, win = eng.play()
    ag = agents_for([K - 1] * G)
    for g in range(G):
        _check_game(oracle, eng, ag[g], g, roots[g], tau[g], out, kids[g], act, win, wm, "stop board %d game %d" % (B, g))
    # a pending leaf: stop between collect_leaves and apply_evals -- the leaf is still backed up, then the move ends
    eng.reset()
    eng.seed_all(seeds)
    eng.set_roots(roots)
    eng.begin_move()
    for i in range(5):
        eng.collect_leaves(run.planes.data_ptr())
        eng.sync()
        pl = run.planes.cpu().numpy()
        for g in range(G):
            run.h_policy[g], run.h_value[g] = ev(g, i, pl[g])
        run.policy.copy_(run.torch.from_numpy(run.h_policy))
        run.value.copy_(run.torch.from_numpy(run.h_value))
        run.torch.cuda.synchronize()
        if i == 4:
            assert eng.settle(stop=True) == G and eng.sims_left() == 1
        eng.apply_evals(run.policy.data_ptr(), run.value.data_ptr())
    assert eng.sims_left() == 0
    out = eng.end_move(tau)
    assert eng.sims_run()["sims"].tolist() == [4] * G
    kids = [children_by_action(eng.root_children(g), A) for g in range(G)]
    act, win = eng.play()
    ag = agents_for([4] * G)
    for g in range(G):
        _check_game(oracle, eng, ag[g], g, roots[g], tau[g], out, kids[g], act, win, wm, "pending stop board %d game %d" % (B, g))
    # a plain short end_move is still an error ...
    eng.reset()
    eng.seed_all(seeds)
    eng.set_roots(roots)
    eng.begin_move()
    eng.collect_leaves(run.planes.data_ptr())
    eng.apply_evals(run.policy.data_ptr(), run.value.data_ptr())
    with pytest.raises(EngineError, match="search ended after 1 of 41 simulations"):
        eng.end_move(tau)
    # ... and the engine is usable afterwards
    eng.reset()
    eng.seed_all(seeds)
    eng.set_roots(roots)
    out = run.move(ev, tau=tau)
    kids = [children_by_action(eng.root_children(g), A) for g in range(G)]
    act, win = eng.play()
    ag = agents_for([S] * G)
    for g in range(G):
        _check_game(oracle, eng, ag[g], g, roots[g], tau[g], out, kids[g], act, win, wm, "after ERR_SHORT board %d game %d" % (B, g))
    eng.close()


def test_bad_arguments_are_errors_that_name_the_cause(oracle):
    """Budgets 0 and num_mcts + 1, noise switched on for a game of a noise=False engine, settle outside a move: each an
    EngineError that names the game / the cause, nothing changed -- the next search on the same engine equals the oracle's."""
    from alpha_omok_amd.engine import Engine, EngineError
    B, mode = 9, 0
    A = B * B
    mark, wm = _win_mark(B)
    roots = _roots(oracle, B, wm, np.random.RandomState(5))
    ev = lambda g, sim, planes: oracle.stub_eval(planes, mode)
    for noise_engine in (True, False):
        eng = Engine(B, S, 5, games=G, noise=noise_engine, win_mark=mark)
        run = Runner(eng)
        seeds = [640 + g for g in range(G)]
        eng.seed_all(seeds)
        eng.set_roots(roots)
        sims = np.full(G, S, np.int32)
        sims[5] = 0
        with pytest.raises(EngineError, match=r"game 5: sims 0 is outside 1\.\.40"):
            eng.begin_move(sims=sims)
        sims[5], sims[2] = 3, S + 1
        with pytest.raises(EngineError, match=r"game 2: sims 41 is outside 1\.\.40"):
            eng.begin_move(sims=sims)
        with pytest.raises(EngineError, match="ao_settle outside"):
            eng.settle()
        if not noise_engine:
            with pytest.raises(EngineError, match="game 6: noise asked for on an engine created without noise"):
                eng.begin_move(noise=np.array([0, 0, 0, 0, 0, 0, 1, 0], np.uint8))
            eng.begin_move(noise=np.zeros(G, np.uint8))           # (switching it off where it is off is no error)
            eng.settle(stop=True)
            eng.end_move()
            eng.reset()
            eng.seed_all(seeds)
            eng.set_roots(roots)
        sims[2] = 0                                              # an inactive game's values are not looked at
        active = np.ones(G, np.uint8)
        active[2] = 0
        sims_ok = np.where(active != 0, sims, S)
        tau = np.ones(G, np.int8)
        out = run.move_opts(ev, tau=tau, active=active, sims=sims)
        kids = [children_by_action(eng.root_children(g), A) for g in range(G)]
        act, win = eng.play()
        for g in np.flatnonzero(active):
            a = oracle.Agent(B, int(sims_ok[g]), 5, noise=noise_engine, evaluator="stub%d" % mode)
            a.seed(seeds[g])
            a.set_win_mark(wm)
            _check_game(oracle, eng, a, g, roots[g], 1, out, kids[g], act, win, wm, "after errors, noise %s game %d" % (noise_engine, g))
        eng.close()
