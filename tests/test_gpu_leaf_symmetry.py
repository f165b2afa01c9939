"""-m gpu: board symmetries where the network is evaluated.

Leaf symmetries (Engine.set_leaf_symmetry): every leaf goes through the network as sym_planes(planes, s) and its policy comes back
through sym_policy_back, s = utils.leaf_symmetry(key of the game, stones on the leaf, simulation index). The oracle is the CPU
reference search (oracle.Agent) whose evaluator applies exactly that around the plain evaluator; everything is compared bit for
bit. The engine itself is driven with the PLAIN evaluator on whatever planes it hands out (step-wise protocol), or runs the
trained 2-block 9x9 network (ao_search, the rolling search), whose recorded evaluations -- in the network's frame -- the oracle
replays through sym_policy_back.

The 8-fold mean (PositionBatch.evaluate(symmetries=8)): against the same fp32 sum worked out on the host from eight plain
evaluate calls on the ids mapped through each symmetry (mode 6: one arithmetic whatever the batch), and against the float64
reference forward in the default mode."""
import numpy as np
import pytest

import pvnet_weights
from gpu_helpers import HostEvalRunner, children_by_action
from test_gpu_fused_parity import _trained_state_dict
from test_leaf_symmetry_host import STUB_MODE

from alpha_omok_amd import utils

pytestmark = pytest.mark.gpu

KEY = 0x5EED1234


def _sym_evaluator(plain, key, seen=None):
    """The evaluator E' of a search with leaf symmetries, around the plain evaluator plain(planes) -> (policy, value)."""
    def ev(moves, planes, sim):
        s = utils.leaf_symmetry(key, len(moves), sim)
        if seen is not None:
            seen.append(s)
        p, v = plain(utils.sym_planes(planes, s))
        return utils.sym_policy_back(p, s), v
    return ev


def _openings(B, G, rs, stones=(0, 3, 4, 6)):
    """Fresh roots with a few scattered stones: the first simulation of a move expands the root itself, on a board that no
    symmetry maps onto itself."""
    ids = []
    for g in range(G):
        n = stones[g % len(stones)]
        while True:
            mv = [int(m) for m in rs.permutation(B * B)[:n]]
            pl = utils.get_state_pt((0,) + tuple(mv), B, 5)
            if n == 0 or all(not np.array_equal(utils.sym_planes(pl, s), pl) for s in range(1, 8)):
                break
        ids.append((0,) + tuple(mv))
    return ids


# ---- 1. the step-wise protocol against the oracle ----------------------------------------------------------------------------------
@pytest.mark.parametrize("B,G,C", [(4, 6, 5), (9, 8, 5), (15, 4, 5), (9, 4, 3)])
def test_stepwise_search_with_leaf_symmetries_vs_oracle(oracle, B, G, C):
    """24 simulations, 3 plies (tau 1, 1, 0), noise on, games from the empty board and from small openings; one, two and four
    64-lane chunks of cells, none of them full. pi, visits, post-noise priors, the root's children, the moves and the streams
    equal the oracle's under E'; what the engine hands out in simulation 0 of a fresh root is sym_planes of the root's planes;
    and an engine without the switch searches differently."""
    from alpha_omok_amd.engine import Engine
    S, PLIES, A = 24, 3, B * B
    mark, wm = (4, 4) if B == 4 else (0, 5)
    rs = np.random.RandomState(77 + B + C)
    roots = _openings(B, G, rs, stones=(0, 3, 4, 5) if B == 4 else (0, 3, 4, 6))
    seeds = [4100 + 13 * g + B for g in range(G)]
    keys = [utils.leaf_key(KEY, s) for s in seeds]

    def plain(planes):
        return oracle.stub_eval(planes, STUB_MODE)

    def engine(sym):
        e = Engine(B, S, C, games=G, noise=True, win_mark=mark)
        e.seed_all(seeds)
        if sym:
            e.set_leaf_symmetry(KEY)
        assert (e.set_roots(roots) == 0).all()
        return e

    eng, off = engine(True), engine(False)
    run, run_off = HostEvalRunner(eng), HostEvalRunner(off)
    seen = [[] for _ in range(G)]
    agents = []
    for g in range(G):
        ag = oracle.Agent(B, S, C, noise=True, evaluator=_sym_evaluator(plain, keys[g], seen[g]))
        ag.seed(seeds[g])
        ag.set_win_mark(wm)
        agents.append(ag)
    first = {}

    def ev(g, sim, planes):
        if sim == 0 and g not in first:
            first[g] = planes.copy()
        return plain(planes)

    alive = np.ones(G, np.uint8)
    roots = list(roots)
    for t in range(PLIES):
        if not alive.any():
            break
        tau = np.full(G, 1 if t < 2 else 0, np.int8)
        pi, vis, pol = run.move(ev, tau=tau, active=alive)
        if t == 0:
            for g in range(G):
                s0 = utils.leaf_symmetry(keys[g], len(roots[g]) - 1, 0)
                want = utils.sym_planes(oracle.get_state_pt(list(roots[g][1:]), B, C), s0)
                np.testing.assert_array_equal(first[g], want, err_msg="planes of simulation 0, game %d, symmetry %d" % (g, s0))
            _, vis_off, _ = run_off.move(lambda g, sim, planes: plain(planes), tau=tau, active=alive)
            assert any(not np.array_equal(vis[g], vis_off[g]) for g in range(G)), "the switch changes nothing: the test sees nothing"
        kids = [children_by_action(eng.root_children(g), A) if alive[g] else None for g in range(G)]
        act, win = eng.play()
        for g in range(G):
            if not alive[g]:
                continue
            tag = "board %d planes %d game %d ply %d" % (B, C, g, t)
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
            ow = oracle.check_win(oracle.get_board(list(roots[g])[1:], B), wm)
            assert win[g] == ow, "win " + tag
            if ow != 0:
                alive[g] = 0
    drawn = set(s for per in seen for s in per)
    assert drawn == set(range(8)), drawn     # every symmetry was exercised, the identity included
    eng.close()
    off.close()


# ---- 2. ao_search with the trained network ------------------------------------------------------------------------------------------
B9, A9 = 9, 81


@pytest.fixture(scope="module")
def net():
    from alpha_omok_amd.engine import Net
    n = Net(2, 5, 128, B9, 0)
    n.load_state_dict(_trained_state_dict())
    n.set_mode(6)
    try:
        yield n
    finally:
        n.set_mode(0)
        n.close()


def _records_of(rec, k):
    """The records of listed game k of one move (rows [launch, n, A + 3] of the evaluation log) that belong to a simulation:
    (policy, value, simulation index, leaf status), in order; the index counts up without gaps."""
    out = []
    for r in rec[:, k]:
        st, done = int(r[A9 + 2]), int(r[A9 + 1])
        if st not in (1, 2, 3):
            continue
        assert done == len(out), (done, len(out))
        out.append((r[:A9].copy(), np.float32(r[A9]), done, st))
    return out


@pytest.mark.parametrize("G,mode,row_cap", [(40, 6, 0), (40, 6, 28), (8, 0, 0)])
def test_fused_search_with_leaf_symmetries_replayed_through_the_oracle(oracle, net, G, mode, row_cap):
    """Engine.search, 9x9, 48 simulations, 3 plies, the trained network: 40 games on the per-layer kernels (mode 6), the same with
    28 rows for 40 games -- over-subscribed: rows handed out per simulation, a share of the games sitting out every launch (the
    window keeps leaves from waiting here; the rolling test below has the waiting leaves) --, and 8 games on the per-board path with the fused per-game step (k_step_board; the default mode plans it). Sampled games are
    replayed through the oracle from the evaluation log, which holds the rows in the network's frame: the replay brings the policy
    back. In mode 6 -- one arithmetic whatever the batch -- a separate forward of sym_planes(planes of the leaf, s) returns every
    logged row, bit for bit."""
    import torch
    from alpha_omok_amd.engine import Engine
    S, PLIES = 48, 3
    net.set_mode(mode)
    try:
        eng = Engine(B9, S, 5, games=G, noise=True)
        seeds = np.arange(61000, 61000 + G, dtype=np.uint32)
        eng.seed_all(seeds)
        eng.set_leaf_symmetry(KEY)
        if row_cap:
            eng.set_row_cap(row_cap)
        sample = [0, 3, G - 1]
        log = torch.zeros((4 * (S + 8) * len(sample) * (A9 + 3),), dtype=torch.float32, device="cuda")
        recs, cursors, fwd = {}, {g: [0] for g in sample}, []

        def make_agent(g):
            key = utils.leaf_key(KEY, int(seeds[g]))

            def replay(moves, pl, sim, g=g):
                i = cursors[g][0]
                cursors[g][0] += 1
                p, v, done, st = recs[g][i]
                assert done == sim
                s = utils.leaf_symmetry(key, len(moves), sim)
                if st != 3:     # (a terminal leaf takes no evaluation: its record holds whatever the row held)
                    fwd.append((utils.sym_planes(pl, s).copy(), p, v))
                return utils.sym_policy_back(p, s), v
            ag = oracle.Agent(B9, S, 5, noise=True, evaluator=replay)
            ag.seed(int(seeds[g]))
            return ag

        agents = {g: make_agent(g) for g in sample}
        roots = {g: (0,) for g in sample}
        for t in range(PLIES):
            tau = np.full(G, 1 if t < 2 else 0, np.int8)
            eng.set_eval_log(sample, log.data_ptr(), log.numel())
            pi, vis, pol = eng.search(net, tau=tau)
            n_rec = eng.eval_log_count()
            rec = log[:n_rec * len(sample) * (A9 + 3)].cpu().numpy().reshape(n_rec, len(sample), A9 + 3)
            act, win = eng.play()
            assert (win == 0).all()
            for k, g in enumerate(sample):
                tag = "game %d ply %d (%d games, mode %d, row cap %d)" % (g, t, G, mode, row_cap)
                recs[g] = _records_of(rec, k)
                cursors[g][0] = 0
                assert len(recs[g]) == S + (1 if t == 0 else 0), tag
                opi, ovis, opol = agents[g].get_pi(roots[g], int(tau[g]))
                np.testing.assert_array_equal(vis[g], ovis, err_msg=tag)
                np.testing.assert_array_equal(pol[g], opol, err_msg=tag)
                np.testing.assert_array_equal(pi[g], opi, err_msg=tag)
                oa = agents[g].rng.choice_p(opi)
                assert act[g] == oa, tag
                roots[g] = roots[g] + (int(oa),)
        if row_cap:
            rows = eng.row_stats()
            print("row cap %d for %d games: %r" % (row_cap, G, rows))
            assert rows["launches"] > 3 * S and rows["rows_launched"] == row_cap * rows["launches"]
        eng.close()
        # the logged rows are the network's answers on the transformed planes
        assert len(fwd) > 3 * len(sample) * S * 0.8
        for i in range(0, len(fwd) if mode == 6 else 0, 256):
            part = fwd[i:i + 256]
            x = torch.from_numpy(np.stack([f[0] for f in part])).cuda()
            p, v = net(x)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(p.cpu().numpy(), np.stack([f[1] for f in part]), err_msg="logged policy rows %d.." % i)
            np.testing.assert_array_equal(v.cpu().numpy().reshape(-1), np.array([f[2] for f in part], np.float32), err_msg="logged values %d.." % i)
    finally:
        net.set_mode(6)


# ---- 3. the rolling search ------------------------------------------------------------------------------------------------------------
# black: four in a row with both ends open, black to move; white's stones scattered
_OPEN_FOUR = (0, 37, 0, 38, 8, 39, 72, 40, 80)


@pytest.mark.parametrize("row_cap", (0, 4))
def test_rolling_search_with_refills_equals_search_and_play(net, row_cap):
    """9x9, 6 games, 16 simulations, tau 0: three games start one move from a win, end, and their slots are refilled (reset +
    seed_games + roll_join) while the others go on. Every record of every episode equals search + play of a one-game engine given
    the episode's seed and the same base key: an episode's symmetries follow its seed, in any slot. With 4 rows for the 6 games
    (the roll has no sit-out window) leaves find the batch full, wait, and are encoded a launch later -- under the symmetry they
    are then expanded with."""
    from alpha_omok_amd.engine import Engine
    G, S, PLIES = 6, 16, 3
    openings = [_OPEN_FOUR if g < 3 else (0,) for g in range(G)]
    eng = Engine(B9, S, 5, games=G, noise=True)
    seeds = [7300 + g for g in range(G)]
    eng.seed_all(seeds)
    eng.set_leaf_symmetry(KEY)
    assert (eng.set_roots(openings) == 0).all()
    if row_cap:
        eng.set_row_cap(row_cap)
    episode = [dict(seed=seeds[g], opening=openings[g], recs=[]) for g in range(G)]   # the episode in each slot
    done, refills, next_seed, drained = [], 0, 9100, False
    eng.roll_begin(net, tau_plies=0, visit=True, policy=True, turn_every=2)
    for _ in range(10000):
        r = eng.roll_run()
        refill = []
        for b in range(len(r["game"])):
            g = int(r["game"][b])
            episode[g]["recs"].append({k: r[k][b] for k in r})
            if r["win"][b] != 0 and not drained:
                refill.append(g)
        if refill:
            mask = np.zeros(G, np.uint8)
            mask[refill] = 1
            eng.reset(mask)
            eng.seed_games(refill, [next_seed + k for k in range(len(refill))])
            for k, g in enumerate(refill):
                done.append(episode[g])
                episode[g] = dict(seed=next_seed + k, opening=(0,), recs=[])
            next_seed += len(refill)
            refills += len(refill)
            eng.roll_join(active=mask, tau_plies=0)
        if not drained and all(len(ep["recs"]) >= PLIES for ep in episode):
            eng.roll_drain()
            drained = True
        if drained and len(r["game"]) == 0:
            break
    else:
        raise AssertionError("the roll did not run dry")
    eng.roll_end()
    rows = eng.row_stats()
    eng.close()
    print("row cap %d: %r, %d refills" % (row_cap, rows, refills))
    if row_cap:
        assert rows["waits"] > 0, "no leaf waited for a row"
    done += episode
    assert refills >= 1, "no game ended: nothing was refilled"
    one = Engine(B9, S, 5, games=1, noise=True)
    one.set_leaf_symmetry(KEY)
    compared = 0
    for ep in done:
        one.reset()
        one.seed(0, ep["seed"])
        if len(ep["opening"]) > 1:
            assert (one.set_roots([ep["opening"]]) == 0).all()
        for t, rec in enumerate(ep["recs"]):
            tag = "episode of seed %d, ply %d" % (ep["seed"], t)
            assert int(rec["ply"]) == len(ep["opening"]) - 1 + t, tag
            pi, vis, pol = one.search(net, tau=np.zeros(1, np.int8))
            act, win = one.play()
            np.testing.assert_array_equal(rec["pi"], pi[0], err_msg=tag)
            np.testing.assert_array_equal(rec["visit"], vis[0], err_msg=tag)
            np.testing.assert_array_equal(rec["policy"], pol[0], err_msg=tag)
            assert (int(rec["action"]), int(rec["win"])) == (int(act[0]), int(win[0])), tag
            compared += 1
    one.close()
    assert compared >= G * PLIES


# ---- 4. the seed alone ------------------------------------------------------------------------------------------------------------------
def _two_plies(net, games, slot, seed, key):
    from alpha_omok_amd.engine import Engine
    eng = Engine(B9, 32, 5, games=games, noise=True)
    eng.seed_all([500 + g for g in range(games)])
    eng.seed(slot, seed)
    eng.set_leaf_symmetry(key)
    out = []
    for t in range(2):
        pi, vis, pol = eng.search(net, tau=np.ones(games, np.int8))
        act, win = eng.play()
        out.append((pi[slot].copy(), vis[slot].copy(), pol[slot].copy(), int(act[slot]), int(win[slot])))
    eng.close()
    return out


def test_an_episode_depends_on_its_seed_and_the_base_key_alone(net):
    """Mode 6 (an evaluation does not depend on the batch): the same seed in slot 3 of a 5-game engine and in slot 0 of a 1-game
    engine plays the same two plies; another base key plays others."""
    a = _two_plies(net, 5, 3, 777, KEY)
    b = _two_plies(net, 1, 0, 777, KEY)
    c = _two_plies(net, 1, 0, 777, KEY ^ 0x01000000)
    for t in range(2):
        for x, y in zip(a[t][:3], b[t][:3]):
            np.testing.assert_array_equal(x, y, err_msg="ply %d" % t)
        assert a[t][3:] == b[t][3:]
    assert any(not np.array_equal(b[t][1], c[t][1]) for t in range(2)), "another base key, the same visits"


# ---- 5. snapshots ----------------------------------------------------------------------------------------------------------------------
def test_snapshot_resumes_bit_for_bit_given_the_key_and_the_seeds(net):
    """export_trees after the first move, import_trees into a fresh engine that was given the same base key and seeds: its next
    move is the uninterrupted one. The snapshot itself does not carry the keys: without them the next move is another."""
    from alpha_omok_amd.engine import Engine
    G, S = 4, 32
    seeds = [880 + g for g in range(G)]
    tau = np.ones(G, np.int8)

    def fresh(sym):
        e = Engine(B9, S, 5, games=G, noise=True)
        if sym:
            e.set_leaf_symmetry(KEY)
        e.seed_all(seeds)
        return e

    a = fresh(True)
    a.search(net, tau=tau)
    a.play()
    snap = a.export_trees()
    want = a.search(net, tau=tau)
    b, c = fresh(True), fresh(False)
    b.import_trees(snap)
    c.import_trees(snap)
    got, plain = b.search(net, tau=tau), c.search(net, tau=tau)
    for x, y in zip(want, got):
        np.testing.assert_array_equal(x, y)
    assert a.play()[0].tolist() == b.play()[0].tolist()
    assert not np.array_equal(want[1], plain[1]), "an importer without the keys searched the same: the test sees nothing"
    for e in (a, b, c):
        e.close()


# ---- 6. off is off ---------------------------------------------------------------------------------------------------------------------
def test_switched_off_again_is_an_engine_that_never_had_it(net):
    from alpha_omok_amd.engine import Engine, EngineError
    G, S = 4, 24
    tau = np.ones(G, np.int8)
    never, was = Engine(B9, S, 5, games=G, noise=True), Engine(B9, S, 5, games=G, noise=True)
    for e in (never, was):
        e.seed_all([40 + g for g in range(G)])
    was.set_leaf_symmetry(KEY)
    was.set_leaf_symmetry(None)
    for t in range(2):
        x, y = never.search(net, tau=tau), was.search(net, tau=tau)
        for u, v in zip(x, y):
            np.testing.assert_array_equal(u, v)
        assert never.play()[0].tolist() == was.play()[0].tolist()
    was.begin_move()
    with pytest.raises(EngineError, match="ao_set_leaf_symmetry inside a move"):
        was.set_leaf_symmetry(KEY)
    with pytest.raises(EngineError, match="ao_set_leaf_symmetry inside a move"):
        was.set_leaf_symmetry(None)
    with pytest.raises(EngineError, match="ao_set_leaf_symmetry_keys inside a move"):
        was.set_leaf_symmetry(keys=[1, 2, 3, 4])
    with pytest.raises(EngineError, match="ao_set_leaf_symmetry_keys: leaf symmetries are off"):
        never.set_leaf_symmetry(keys=[1, 2, 3, 4])
    never.close()
    was.close()


# ---- 7. the 8-fold mean --------------------------------------------------------------------------------------------------------------
def _positions(B, wm, rs):
    """Five ids: the empty board, a finished game (black's line on the top row), three scattered positions."""
    line = [x for k in range(wm) for x in (k, B * (B - 1) + k)][:2 * wm - 1]
    ids = [(0,), (0,) + tuple(line)]
    for n in (1, 6, 11):
        ids.append((0,) + tuple(int(m) for m in rs.permutation(B * B)[:n]))
    return ids


def _host_mean(pb, net, ids, B):
    """The fp32 reduction of ao_positions_evaluate_sym on the host, from eight plain evaluate calls: the ids mapped through each
    symmetry give the network's answers on sym_planes(planes, s)."""
    acc_p = acc_v = None
    for s in range(8):
        mapped = [(0,) + tuple(utils.sym_cell_inv(s, m, B) for m in i[1:]) for i in ids]
        p, v, _, err = pb.evaluate(net, mapped)
        assert (err == 0).all()
        p = utils.sym_policy_back(p, s).astype(np.float32)
        acc_p = p if s == 0 else (acc_p + p).astype(np.float32)
        acc_v = v if s == 0 else (acc_v + v).astype(np.float32)
    return np.float32(0.125) * acc_p, np.float32(0.125) * acc_v


@pytest.mark.parametrize("B,capacity", [(4, 16), (9, 16), (9, 64), (15, 16)])
def test_eight_fold_mean_bits(B, capacity):
    """Mode 6. capacity 16: two positions per chunk, the five ids go through three chunks; 64: one chunk."""
    from alpha_omok_amd.engine import Net
    from alpha_omok_amd.positions import PositionBatch
    wm = 4 if B == 4 else 5
    net = Net(1, 5, 128, B, 0)
    net.load_state_dict(pvnet_weights.make_state_dict(1, 5, 128, B, 300 + B))
    net.set_mode(6)
    ids = _positions(B, wm, np.random.RandomState(B))
    with PositionBatch(B, 5, wm, capacity=capacity) as pb:
        assert pb.describe(ids)["status"].tolist()[:2] == [0, 1]
        p1, v1, st1, e1 = pb.evaluate(net, ids)
        q1, w1, st2, e2 = pb.evaluate(net, ids, symmetries=1)
        for x, y in ((p1, q1), (v1, w1), (st1, st2), (e1, e2)):
            np.testing.assert_array_equal(x, y)
        p8, v8, st8, e8 = pb.evaluate(net, ids, symmetries=8)
        hp, hv = _host_mean(pb, net, ids, B)
        np.testing.assert_array_equal(p8, hp)
        np.testing.assert_array_equal(v8, hv)
        np.testing.assert_array_equal(st8, st1)
        assert (e8 == 0).all()
        assert not np.array_equal(p8[2:], p1[2:])       # the mean is not the single orientation
        bad, _, _, eb = pb.evaluate(net, [(0, 1, 1), (0, 2)], symmetries=8)   # an id with an error gets zeros
        assert eb.tolist() == [2, 0] and not bad[0].any() and bad[1].any()
    with PositionBatch(B, 5, wm, capacity=4) as small:
        with pytest.raises(Exception, match="capacity of at least 8"):
            small.evaluate(net, ids, symmetries=8)
    net.close()


def test_eight_fold_mean_default_mode_vs_float64_reference():
    """The default mode against tests/net_reference.forward in float64, for the 4-block 128-plane 9x9 network test_gpu_net.py holds
    to 1e-4 per evaluation: the mean of eight values each within 1e-4 is within 1e-4, plus 8 * 2^-24 for the fp32 sum of eight
    numbers in [0, 1]. ZeroAgent.get_pv(symmetries=8) is the batch call."""
    import net_reference
    import torch
    from alpha_omok_amd.agents import ZeroAgent
    from alpha_omok_amd.engine import Net
    from alpha_omok_amd.positions import PositionBatch
    B, nb = 9, 4
    sd = pvnet_weights.make_state_dict(nb, 5, 128, B, 100 + nb)
    net = Net(nb, 5, 128, B, 0)
    net.load_state_dict(sd)
    ids = _positions(B, 5, np.random.RandomState(21))
    x = np.stack([utils.get_state_pt(i, B, 5) for i in ids]).astype(np.float32)
    ref_p = np.zeros((len(ids), B * B))
    ref_v = np.zeros(len(ids))
    for s in range(8):
        r = net_reference.forward(sd, utils.sym_planes(x, s))
        ref_p += utils.sym_policy_back(torch.softmax(r["logits"], dim=1).numpy(), s)
        ref_v += torch.tanh(r["z"]).numpy()
    ref_p /= 8
    ref_v /= 8
    with PositionBatch(B, 5, 5, capacity=64) as pb:
        p8, v8, _, _ = pb.evaluate(net, ids, symmetries=8)
        p_one, v_one, _, _ = pb.evaluate(net, [ids[3]], symmetries=8)   # (a batch of its own: the rows get_pv's forward runs)
    dp, dv = np.abs(p8 - ref_p).max(), np.abs(v8 - ref_v).max()
    bound = 1e-4 + 8 * 2.0 ** -24
    print("8-fold mean against the float64 reference: policy %.3g, value %.3g (bound %.3g)" % (dp, dv, bound))
    assert dp < bound and dv < bound, (dp, dv)
    ag = ZeroAgent(B, 8, 5, noise=False)
    ag.model = net
    gp, gv = ag.get_pv(ids[3], symmetries=8)
    np.testing.assert_array_equal(gp, p_one[0])
    assert gv == v_one[0]
    net.close()


# ---- 8. through main: the switch composes with reproducible, strict, refills and rolling ------------------------------------------------
def test_self_play_with_leaf_symmetries_rolling_equals_synchronous():
    """main.configure(leaf_symmetry=KEY, reproducible=True, strict=True): ten episodes on four refilled slots are the same episodes
    -- moves, lengths, winners, recorded pi -- under rolling=True, because an episode's symmetries follow its seed through
    seed_games; and they are other episodes than without the switch."""
    import alpha_omok_amd.main as main
    from test_gpu_rolling import _configure, _episodes, _restore
    keep = main.MAX_CONCURRENT
    try:
        _configure(main)
        plain = _episodes(main)
        _configure(main, leaf_symmetry=KEY)
        sync = _episodes(main)
        _configure(main, leaf_symmetry=KEY, rolling=True, turn_every=3)
        roll = _episodes(main)
        for x, y, what in zip(sync, roll, ("moves", "lengths", "wins", "episode of sample", "ply of sample", "pi")):
            np.testing.assert_array_equal(x, y, err_msg=what)
        assert not (np.array_equal(plain[0], sync[0]) and np.array_equal(plain[5], sync[5])), "the switch changed no episode"
    finally:
        _restore(main, keep)
    assert main.LEAF_SYMMETRY is None
