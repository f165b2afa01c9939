"""-m gpu: leaf tactics (Engine.set_leaf_tactics, ao_set_leaf_tactics): the forced-win solver runs on every leaf the search
expands and its proof overrides the value -- exactly +1 for the leaf's mover. The definition is utils.leaf_tactics_value; a
search with the switch on is the reference search (oracle.Agent) under utils.leaf_tactics_evaluator, and everything is compared
bit for bit. The engine itself is driven with the PLAIN evaluator (step-wise protocol), or runs a network (ao_search, the rolling
search) whose logged evaluations -- what the network said, not the override -- the oracle replays through the wrapper.

The roots, seeds and settings are tests/test_leaf_tactics_host.py's, which asserts on the host that they make the switch
visible: at least a quarter of the leaves proven, most visit rows other than the plain search's, leaves out of budget at 9x9."""
import numpy as np
import pytest

import pvnet_weights
from gpu_helpers import HostEvalRunner, children_by_action
from test_forced_win_host import MARK, hand_made
from test_gpu_fused_parity import _trained_state_dict
from test_gpu_leaf_symmetry import KEY, _records_of, _sym_evaluator
from test_leaf_tactics_host import (DEPTH, GAMES, NODES, PLANES, SIMS, counting_evaluator, oracle_agent, roots_of, seeds_of,
                                    stub_of)

from alpha_omok_amd import utils

pytestmark = pytest.mark.gpu

B9, A9 = 9, 81
PLIES = 3


def _engine(B, roots=None, seeds=None, switch=True, games=GAMES, sims=SIMS):
    from alpha_omok_amd.engine import Engine
    e = Engine(B, sims, PLANES, games=games, noise=True, win_mark=MARK[B])
    e.seed_all(seeds_of(games) if seeds is None else seeds)
    if switch:
        e.set_leaf_tactics(DEPTH, NODES)
    assert (e.set_roots(roots_of(B) if roots is None else roots) >= 0).all()
    return e


def _stepwise_vs_oracle(oracle, B, plain_of, key=None):
    """Three plies (tau 1, 1, 0) with play() between -- inherited roots from the second on -- of the engine under the plain
    evaluator plain_of(g)(moves, planes, sim) against the oracle under the wrapper around it: pi, visit, the post-noise priors,
    the root's children, the moves and the streams; then the counters against the host's over the non-terminal leaves."""
    G, A = GAMES, B * B
    roots, seeds = list(roots_of(B)), seeds_of()
    eng = _engine(B)
    if key is not None:
        eng.set_leaf_symmetry(key)
    run = HostEvalRunner(eng)
    tally = np.zeros((G, 4), np.int64)
    agents = [oracle_agent(oracle, B, seeds[g], counting_evaluator(plain_of(g), B, tally[g])) for g in range(G)]
    plain = [plain_of(g) for g in range(G)]
    alive = np.ones(G, np.uint8)
    for t in range(PLIES):
        if not alive.any():
            break
        tau = np.full(G, 1 if t < 2 else 0, np.int8)
        if key is None:
            ev = lambda g, sim, planes: plain[g](None, planes, sim)
        else:       # (the engine hands out the planes already transformed: the device side evaluates them as they are)
            ev = lambda g, sim, planes: oracle.stub_eval(planes, B % 3)
        pi, vis, pol = run.move(ev, tau=tau, active=alive)
        kids = [children_by_action(eng.root_children(g), A) if alive[g] else None for g in range(G)]
        act, win = eng.play()
        for g in range(G):
            if not alive[g]:
                continue
            tag = "board %d game %d ply %d" % (B, g, t)
            opi, ovis, opol = agents[g].get_pi(roots[g], int(tau[g]))
            np.testing.assert_array_equal(vis[g], ovis, err_msg="visit " + tag)
            np.testing.assert_array_equal(pol[g], opol, err_msg="policy " + tag)
            np.testing.assert_array_equal(pi[g], opi, err_msg="pi " + tag)
            och = agents[g].children(roots[g])
            assert kids[g]["order"].tolist() == och["order"].tolist(), "child order " + tag
            for k in ("n", "w", "q", "p"):
                np.testing.assert_array_equal(kids[g][k], och[k], err_msg=k + " " + tag)
            oa = agents[g].rng.choice_p(opi)
            assert act[g] == oa, "action " + tag
            roots[g] = roots[g] + (int(oa),)
            mt, pos, _, _ = eng.get_rng_state(g)
            assert pos == agents[g].rng.pos, "mt position " + tag
            np.testing.assert_array_equal(mt, agents[g].rng.state_words(), err_msg="mt " + tag)
            ow = oracle.check_win(oracle.get_board(list(roots[g])[1:], B), MARK[B])
            assert win[g] == ow, "win " + tag
            if ow != 0:
                alive[g] = 0
    st = eng.leaf_tactics_stats(per_game=True)
    print("board %d: device counters %r" % (B, {k: st[k] for k in ("searched", "proven", "unknown", "nodes")}))
    np.testing.assert_array_equal(st["per_game"], tally, err_msg="per-game counters, board %d" % B)
    assert [st[k] for k in ("searched", "proven", "unknown", "nodes")] == tally.sum(axis=0).tolist()
    assert st["proven"] > 0 and 4 * st["proven"] >= st["searched"]
    if B == 9:
        assert st["unknown"] >= 1
    again = eng.leaf_tactics_stats(per_game=True, reset=True)
    np.testing.assert_array_equal(again["per_game"], tally)
    zero = eng.leaf_tactics_stats(per_game=True)
    assert not zero["per_game"].any() and (zero["searched"], zero["proven"], zero["unknown"], zero["nodes"]) == (0, 0, 0, 0)
    eng.close()


# ---- 1. the step-wise protocol against the oracle ----------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (6, 9, 12, 15))
def test_stepwise_search_with_leaf_tactics_vs_oracle(oracle, B):
    """One to four mask words. The device side sees the plain stub's values: ao_apply_evals copies them, searches the leaves and
    overrides the proven ones in the copy."""
    _stepwise_vs_oracle(oracle, B, lambda g: stub_of(oracle, B))


# ---- 4. with leaf symmetries on ----------------------------------------------------------------------------------------------------
def test_stepwise_search_with_leaf_tactics_and_leaf_symmetries_vs_oracle(oracle):
    """9x9: the oracle under the wrapper around the symmetry evaluator of tests/test_gpu_leaf_symmetry.py."""
    keys = [utils.leaf_key(KEY, s) for s in seeds_of()]
    _stepwise_vs_oracle(oracle, B9, lambda g: _sym_evaluator(lambda planes: oracle.stub_eval(planes, B9 % 3), keys[g]), key=KEY)


# ---- 2. ao_search with a real network -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_net():
    """one block, random weights, mode 6: one arithmetic whatever the batch, so that a game's evaluations do not depend on how
    the rows are handed out"""
    from alpha_omok_amd.engine import Net
    n = Net(1, PLANES, 128, B9, 0)
    n.load_state_dict(pvnet_weights.make_state_dict(1, PLANES, 128, B9, 4242))
    n.set_mode(6)
    try:
        yield n
    finally:
        n.close()


def _two_plies(eng, net, log=None):
    """tau 1 then 0 with play() between, a game that ends at the first sitting out the second: [(pi, visit, policy, action,
    win, the games searched, log records of the move or None)]"""
    out = []
    alive = np.ones(eng.G, np.uint8)
    for t in range(2):
        tau = np.full(eng.G, 1 if t == 0 else 0, np.int8)
        if log is not None:
            eng.set_eval_log(list(range(eng.G)), log.data_ptr(), log.numel())
        pi, vis, pol = eng.search(net, tau=tau, active=alive)
        rec = None
        if log is not None:
            n = eng.eval_log_count()
            rec = log[:n * eng.G * (A9 + 3)].cpu().numpy().reshape(n, eng.G, A9 + 3)
        act, win = eng.play()
        out.append((pi, vis, pol, act.copy(), win.copy(), alive.copy(), rec))
        alive = alive & (win == 0).astype(np.uint8)
    return out


def test_search_with_a_network_replayed_through_the_wrapped_oracle(oracle, small_net, monkeypatch):
    """ao_search, 8 games from the 9x9 roots: the evaluation log holds what the NETWORK said; replayed through the wrapper in the
    oracle it gives the engine's records. With 5 rows for the 8 games (rows per simulation, waiting leaves -- searched in the launch
    that gives them their row) the records are those without the cap, and so they are with AO_LEAF_TACTICS_SERIAL set."""
    import torch
    G = GAMES
    monkeypatch.delenv("AO_LEAF_TACTICS_SERIAL", raising=False)
    log = torch.zeros((2 * (SIMS + 8) * G * (A9 + 3),), dtype=torch.float32, device="cuda")
    base = _engine(B9)
    got = _two_plies(base, small_net, log)
    st = base.leaf_tactics_stats()
    assert st["proven"] > 0 and st["searched"] > st["proven"]
    base.close()
    roots, seeds = list(roots_of(B9)), seeds_of()
    recs, cursor = {}, {g: 0 for g in range(G)}
    overridden = [0]

    def replay_of(g):
        def replay(moves, planes, sim):
            p, v, done, status = recs[g][cursor[g]]
            cursor[g] += 1
            assert done == sim
            return p, v
        return replay

    def spying(g):
        inner = utils.leaf_tactics_evaluator(replay_of(g), B9, MARK[B9], DEPTH, NODES)

        def f(moves, planes, sim):
            before = recs[g][cursor[g]][1]
            p, v = inner(moves, planes, sim)
            overridden[0] += (v == np.float32(1.0)) and (before != np.float32(1.0))
            return p, v
        return f

    agents = [oracle_agent(oracle, B9, seeds[g], spying(g)) for g in range(G)]
    for t, (pi, vis, pol, act, win, alive, rec) in enumerate(got):
        for g in np.flatnonzero(alive):
            tag = "game %d ply %d" % (g, t)
            recs[g] = _records_of(rec, g)
            cursor[g] = 0
            assert len(recs[g]) == SIMS + (1 if t == 0 else 0), tag      # (a fresh root's expansion is one simulation more)
            opi, ovis, opol = agents[g].get_pi(roots[g], 1 if t == 0 else 0)
            np.testing.assert_array_equal(vis[g], ovis, err_msg=tag)
            np.testing.assert_array_equal(pol[g], opol, err_msg=tag)
            np.testing.assert_array_equal(pi[g], opi, err_msg=tag)
            oa = agents[g].rng.choice_p(opi)
            assert act[g] == oa, tag
            roots[g] = roots[g] + (int(oa),)
    assert overridden[0] > 0, "the log held no network value that the wrapper overrode"

    def same(other, what):
        for t in range(2):
            for x, y, name in zip(got[t][:6], other[t][:6], ("pi", "visit", "policy", "action", "win", "games searched")):
                np.testing.assert_array_equal(x, y, err_msg="%s, ply %d: %s" % (what, t, name))

    capped = _engine(B9)
    capped.set_row_cap(5)
    same(_two_plies(capped, small_net), "5 rows for 8 games")
    rows = capped.row_stats()
    print("5 rows for 8 games: %r" % (rows,))
    assert rows["launches"] > 2 * SIMS and rows["rows_launched"] == 5 * rows["launches"]
    assert capped.leaf_tactics_stats() == st          # every leaf searched once, whatever launch gave it its row
    capped.close()
    serial = _engine(B9)
    monkeypatch.setenv("AO_LEAF_TACTICS_SERIAL", "1")
    first = _two_plies(serial, small_net)
    monkeypatch.delenv("AO_LEAF_TACTICS_SERIAL")
    same(first, "AO_LEAF_TACTICS_SERIAL")
    assert serial.leaf_tactics_stats() == st
    serial.close()
    plain = _engine(B9, switch=False)
    other = _two_plies(plain, small_net)
    plain.close()
    assert any(not np.array_equal(got[0][1][g], other[0][1][g]) for g in range(G)), "the switch changes nothing: the test sees nothing"


# ---- 3. the rolling search -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net():
    from alpha_omok_amd.engine import Net
    n = Net(2, PLANES, 128, B9, 0)
    n.load_state_dict(_trained_state_dict())
    n.set_mode(6)
    try:
        yield n
    finally:
        n.set_mode(0)
        n.close()


@pytest.mark.parametrize("tactics,row_cap", ((None, 0), (True, 0), (None, 5)))
def test_rolling_search_equals_search_and_play(net, tactics, row_cap):
    """8 games from the 9x9 roots, three plies each (tau 1 at the first), turned two launches apart: every record of the roll is
    search + play of a twin engine with the switch on -- and, the second time, with the solver at the roots as well
    (roll_begin(tactics=True) against search(tactics=True)). The third time with 5 rows for the 8 games: the roll has no sit-out
    window, so leaves find the batch full, wait, and are searched in the launch that gives them their row."""
    G = GAMES
    nopen = np.array([len(r) - 1 for r in roots_of(B9)], np.int32)
    eng = _engine(B9)
    if row_cap:
        eng.set_row_cap(row_cap)
    eng.roll_begin(net, tau_plies=nopen + 1, visit=True, policy=True, turn_every=2, tactics=tactics)
    recs, played, over, drained = {}, np.zeros(G, int), np.zeros(G, bool), False
    for _ in range(100000):
        r = eng.roll_run()
        for b in range(len(r["game"])):
            g = int(r["game"][b])
            assert int(r["ply"][b]) - nopen[g] == played[g]
            recs[(g, int(played[g]))] = {k: r[k][b] for k in ("pi", "visit", "policy", "action", "win")}
            played[g] += 1
            over[g] = r["win"][b] != 0
        if not drained and ((played >= PLIES) | over).all():
            eng.roll_drain()
            drained = True
        if drained and len(r["game"]) == 0:
            break
    else:
        raise AssertionError("the roll did not run dry")
    eng.roll_end()
    st = eng.leaf_tactics_stats()
    if row_cap:
        assert eng.row_stats()["waits"] > 0, "no leaf waited for a row"
    eng.close()
    assert st["proven"] > 0
    twin = _engine(B9)
    compared = 0
    for k in range(int(played.max())):
        active = (played > k).astype(np.uint8)
        tau = np.full(G, 1 if k < 1 else 0, np.int8)
        pi, vis, pol = twin.search(net, tau=tau, active=active, tactics=tactics)
        act, win = twin.play()
        for g in np.flatnonzero(active):
            tag = "game %d ply %d (tactics %r, row cap %d)" % (g, k, tactics, row_cap)
            rec = recs[(int(g), k)]
            np.testing.assert_array_equal(rec["pi"], pi[g], err_msg=tag)
            np.testing.assert_array_equal(rec["visit"], vis[g], err_msg=tag)
            np.testing.assert_array_equal(rec["policy"], pol[g], err_msg=tag)
            assert (int(rec["action"]), int(rec["win"])) == (int(act[g]), int(win[g])), tag
            compared += 1
    assert compared == len(recs) and compared >= G
    assert twin.leaf_tactics_stats() == st
    twin.close()


# ---- 5. lifecycle ----------------------------------------------------------------------------------------------------------------------
def test_limits_are_refused_before_anything_else():
    from alpha_omok_amd.engine import Engine, EngineError
    eng = Engine(B9, SIMS, PLANES, games=2, noise=True)
    for depth, nodes, text in ((17, 64, "max_depth must be in 1..16"), (-1, 64, "max_depth must be in 1..16"),
                               (4, 1025, "max_nodes must be in 1..1024"), (4, 0, "max_nodes must be in 1..1024")):
        with pytest.raises(EngineError, match="ao_set_leaf_tactics: " + text):
            eng.set_leaf_tactics(depth, nodes)
    eng.begin_move()
    with pytest.raises(EngineError, match="max_nodes must be in 1..1024"):     # (the limits come first, inside a move too)
        eng.set_leaf_tactics(4, 1025)
    with pytest.raises(EngineError, match="ao_set_leaf_tactics inside a move"):
        eng.set_leaf_tactics(4, 64)
    with pytest.raises(EngineError, match="ao_set_leaf_tactics inside a move"):
        eng.set_leaf_tactics(None)
    eng.close()
    wide =Engine(6, SIMS, PLANES, games=2, noise=True, win_mark=10)          # no line wins: nothing for the solver
    with pytest.raises(EngineError, match="win_mark in 3..5"):
        wide.set_leaf_tactics(4, 64)
    wide.set_leaf_tactics(None)
    assert wide.leaf_tactics_stats(per_game=True)["per_game"].shape == (2, 4)
    wide.close()


def test_refused_for_a_roll_with_games_in_a_move(net):
    from alpha_omok_amd.engine import EngineError
    eng = _engine(B9, switch=False)
    mask = np.zeros(GAMES, np.uint8)
    mask[:3] = 1
    eng.roll_begin(net, active=mask, tau_plies=0)
    with pytest.raises(EngineError, match="ao_set_leaf_tactics: game 0 is in a move of the open roll"):
        eng.set_leaf_tactics(DEPTH, NODES)
    eng.roll_drain()
    while len(eng.roll_run()["game"]):
        pass
    eng.set_leaf_tactics(DEPTH, NODES)          # an open roll with nothing in a move takes it
    eng.set_leaf_tactics(None)
    eng.roll_end()
    eng.close()


def test_switched_off_again_is_an_engine_that_never_had_it(net, monkeypatch):
    """... under guarded allocations: the solver's buffers come from the engine's pool, and nothing writes outside a block."""
    from alpha_omok_amd.engine import guard_check
    monkeypatch.setenv("AO_POOL_GUARD", "4096")
    tau = np.ones(GAMES, np.int8)
    never, was = _engine(B9, switch=False), _engine(B9)
    first = was.search(net, tau=tau)
    assert guard_check()[1:] == (0, "")
    st = was.leaf_tactics_stats(reset=True)
    assert st["searched"] > 0 and st["proven"] > 0
    assert was.leaf_tactics_stats() == dict(searched=0, proven=0, unknown=0, nodes=0)
    plain = never.search(net, tau=tau)
    assert any(not np.array_equal(first[1][g], plain[1][g]) for g in range(GAMES))
    # the same position and streams again for both, the switch off: the same bits, and nothing is counted
    for e in (never, was):
        e.reset()
        e.seed_all(seeds_of())
        assert (e.set_roots(roots_of(B9)) >= 0).all()
    was.set_leaf_tactics(None)
    for t in range(2):
        x, y = never.search(net, tau=tau), was.search(net, tau=tau)
        for u, v in zip(x, y):
            np.testing.assert_array_equal(u, v)
        assert never.play()[0].tolist() == was.play()[0].tolist()
    assert was.leaf_tactics_stats()["searched"] == 0
    assert guard_check()[1:] == (0, "")
    never.close()
    was.close()


def test_zero_agent_takes_the_switch():
    """ZeroAgent(leaf_tactics=): a one-game engine without the fused per-game step; the counters move."""
    import torch
    from alpha_omok_amd.agents import ZeroAgent
    from alpha_omok_amd.pvnet import PVNet
    with pytest.raises(ValueError):
        ZeroAgent(B9, SIMS, PLANES, leaf_tactics=dict(max_nodes=1025))
    torch.manual_seed(5)
    ag = ZeroAgent(B9, SIMS, PLANES, noise=False, leaf_tactics=dict(max_depth=DEPTH, max_nodes=NODES))
    ag.model = PVNet(1, PLANES, 128, B9).cuda().eval()
    root = hand_made()["open three"][0]          # the mover wins in two: the fresh root's own expansion is a proven leaf
    pi = ag.get_pi(root, 0)
    assert pi.shape == (A9,) and abs(pi.sum() - 1.0) < 1e-12
    st = ag._engine.leaf_tactics_stats()
    assert st["searched"] > 0 and st["proven"] > 0


# ---- 6. through main: the switch composes with reproducible, strict, refills and rolling ------------------------------------------------
def test_self_play_with_leaf_tactics_rolling_equals_synchronous():
    """main.configure(leaf_tactics=..., reproducible=True, strict=True): ten episodes on four refilled slots are the same episodes
    -- moves, lengths, winners, recorded pi -- under rolling=True; the self-play engine carries the switch and its counters move;
    configure() without the argument switches it off again."""
    import alpha_omok_amd.main as main
    from test_gpu_rolling import _configure, _episodes, _restore
    keep = main.MAX_CONCURRENT
    lt = dict(max_depth=DEPTH, max_nodes=NODES)
    try:
        _configure(main, leaf_tactics=lt)
        assert main.LEAF_TACTICS == (DEPTH, NODES) and main.Agent.leaf_tactics == (DEPTH, NODES)
        sync = _episodes(main)
        st = main._engine.leaf_tactics_stats()
        assert st["searched"] > 0 and st["proven"] > 0, st
        _configure(main, leaf_tactics=lt, rolling=True, turn_every=3)
        roll = _episodes(main)
        for x, y, what in zip(sync, roll, ("moves", "lengths", "wins", "episode of sample", "ply of sample", "pi")):
            np.testing.assert_array_equal(x, y, err_msg=what)
        assert main._engine.leaf_tactics_stats()["proven"] > 0
    finally:
        _restore(main, keep)
    assert main.LEAF_TACTICS is None
