"""-m gpu: the rolling search with the forced-win solver beside its loop (Engine.roll_begin(tactics=...), ao_roll_set_tactics).
Every move a game begins inside such a roll is begun as search(tactics=...) begins it: the solver's bar at the root, a proven
win capped at solved_sims simulations. The solver runs in batches on a stream of its own while the other games go on searching;
the games of a batch wait for its verdict.

The oracle is the synchronous path on a fresh twin engine, as in test_gpu_rolling: the same seeds and roots, per relative ply
search(sims=<the records' simulations>, tactics=dict(max_depth, max_nodes)) + play() for the games the roll played at that ply.
assert_array_equal everywhere: nothing of a record may depend on when its verdict arrived -- AO_ROLL_TACTICS_HOLD=k holds every
finished batch for k further turns, which reaches the "verdict arrives late" path without any timing.

Board 9x9, 8 games on the fixture's roots of test_gpu_root_tactics._verdict_roots(9) -- WIN / DEFEND / LOST / NONE twice --, at
the fixture's own limits (depth 6, 2000 nodes), the trained 2-block network on the per-layer kernels (mode 6)."""
import numpy as np
import pytest

from test_forced_defence_host import DEPTH, MARK, NODES
from test_gpu_fused_parity import _trained_state_dict
from test_gpu_root_tactics import _verdict_roots
from test_gpu_search_early_stop import SEEDS

pytestmark = pytest.mark.gpu

B, S, G = 9, 40, 8
A = B * B
LIMITS = dict(max_depth=DEPTH, max_nodes=NODES)
BUDGETS = np.array([4, 8, 12, 16, 20, 28, 36, 40], np.int32)
SOLVED = 6
WORDS = ("verdict", "depth", "nodes", "unknown")
RT_NONE, RT_WIN, RT_DEFEND, RT_LOST = 0, 1, 2, 3


def _roots():
    roots, want = _verdict_roots(B)
    return roots, want, np.array([len(r) - 1 for r in roots], np.int32)


@pytest.fixture(scope="module")
def net():
    from alpha_omok_amd.engine import Net
    n = Net(2, 5, 128, B, 0)
    n.load_state_dict(_trained_state_dict())
    n.set_mode(6)
    try:
        yield n
    finally:
        n.set_mode(0)
        n.close()


@pytest.fixture(scope="module")
def flat_net():
    """a network that knows nothing: every weight zero -- uniform priors, value 0"""
    from alpha_omok_amd.engine import Net
    n = Net(2, 5, 128, B, 0)
    n.load_state_dict({k: np.zeros_like(v) for k, v in _trained_state_dict().items()})
    n.set_mode(6)
    try:
        yield n
    finally:
        n.close()


def _engine(sims=S, noise=True, roots=None):
    from alpha_omok_amd.engine import Engine
    eng = Engine(B, sims, 5, games=G, noise=noise, win_mark=MARK[B])
    eng.seed_all(SEEDS)
    assert (eng.set_roots(_roots()[0] if roots is None else roots) >= 0).all()
    return eng


def _streams(eng):
    st = [eng.get_rng_state(g) for g in range(eng.G)]
    return np.stack([s[0] for s in st]), np.array([s[1] for s in st])


def _take(r, nopen, recs, played, over):
    for b in range(len(r["game"])):
        g = int(r["game"][b])
        one = {k: r[k][b] for k in r}
        one["rel"] = int(r["ply"][b]) - int(nopen[g])
        assert one["rel"] == played[g]
        recs.append(one)
        played[g] += 1
        over[g] = r["win"][b] != 0


def _roll(eng, net, plies, tau_rel, tactics, **kw):
    """Rolls until every game has played `plies` plies (or is over), drains, runs dry, ends: (records in return order, plies
    played per game, roll_tactics_stats)."""
    nopen = _roots()[2]
    eng.roll_begin(net, tau_plies=nopen + tau_rel, visit=True, policy=True, tactics=tactics, **kw)
    recs, played, over, drained = [], np.zeros(G, int), np.zeros(G, bool), False
    for _ in range(100000):
        r = eng.roll_run()
        _take(r, nopen, recs, played, over)
        if not drained and ((played >= plies) | over).all():
            eng.roll_drain()
            drained = True
        if drained and len(r["game"]) == 0:
            break
    else:
        raise AssertionError("the roll did not run dry")
    stats = eng.roll_tactics_stats()
    eng.roll_end()
    return recs, played, stats


def _oracle(net, recs, played, tau_rel, eng=None):
    """The synchronous twin: per relative ply the games the roll played at it, with the budgets its records report and the
    solver in front (no solved_sims: the cap is in the budgets). Returns {(game, rel): (pi, visit, policy, action, win, tactics
    row)}, the engine (open) and the number of compared moves in which a root child with inherited visits was barred."""
    eng = eng or _engine()
    sims = {(int(r["game"]), r["rel"]): int(r["sims"]) for r in recs}
    out, barred_inherited = {}, 0
    for k in range(int(played.max())):
        active = played > k
        budget = np.array([sims.get((g, k), 1) for g in range(G)], np.int32)
        tau = (np.ones(G) * (1 if k < tau_rel else 0)).astype(np.int8)
        before = {int(g): eng.root_children(int(g)) for g in np.flatnonzero(active)} if k > 0 else {}
        pi, vis, pol = eng.search(net, tau=tau, active=active.astype(np.uint8), sims=budget, tactics=dict(LIMITS))
        rt = eng.last_tactics()
        act, win = eng.play()
        for g in np.flatnonzero(active):
            g = int(g)
            out[(g, k)] = (pi[g], vis[g], pol[g], int(act[g]), int(win[g]), {key: rt[key][g] for key in WORDS + ("allowed",)})
            rc = before.get(g)
            if rc is not None and len(rc["action"]) and ((rc["n"] > 0) & ~rt["allowed"][g][rc["action"]]).any():
                barred_inherited += 1
    return out, eng, barred_inherited


def _compare(recs, oracle, tag, allowed=True):
    assert len(recs) == len(oracle)
    for r in recs:
        key = (int(r["game"]), r["rel"])
        pi, vis, pol, act, win, rt = oracle[key]
        np.testing.assert_array_equal(r["pi"], pi, err_msg="%s %r: pi" % (tag, key))
        np.testing.assert_array_equal(r["visit"], vis, err_msg="%s %r: visit" % (tag, key))
        np.testing.assert_array_equal(r["policy"], pol, err_msg="%s %r: policy" % (tag, key))
        assert (int(r["action"]), int(r["win"])) == (act, win), (tag, key)
        for w in WORDS:
            assert int(r[w]) == int(rt[w]), (tag, key, w, int(r[w]), int(rt[w]))
        if allowed:
            np.testing.assert_array_equal(r["allowed"], rt["allowed"], err_msg="%s %r: allowed" % (tag, key))


TACTICS = dict(LIMITS, solved_sims=SOLVED, allowed=True)


def _parity_roll(net, turn_every):
    eng = _engine()
    try:
        recs, played, stats = _roll(eng, net, 3, 2, TACTICS, sims=BUDGETS, turn_every=turn_every)
        mt, pos = _streams(eng)
        kids = [eng.root_children(g) for g in range(G)]
        # one synchronous ply behind the roll: a sentinel left in a root by the roll's last bars would be seen here
        after = eng.search(net, tau=0) + eng.play()
        return recs, played, stats, mt, pos, kids, after
    finally:
        eng.close()


@pytest.mark.parametrize("hold", (0, 2))
@pytest.mark.parametrize("turn_every", (1, 4))
def test_records_equal_the_synchronous_tactics_search(net, turn_every, hold, monkeypatch):
    """Budgets 4 .. 40, tau 1 for two plies, solved_sims 6, three plies per game: pi, visit, policy, action, win, the solver's
    words and allowed rows of every record, and every stream after the last ply, equal the twin's; a proven win searched
    min(budget, 6) simulations and nothing else was capped; some compared move barred a child with inherited visits; held
    batches made games wait; the synchronous ply behind roll_end equals the twin's next ply."""
    monkeypatch.setenv("AO_ROLL_TACTICS_HOLD", str(hold))
    tag = "turn_every %d, hold %d" % (turn_every, hold)
    recs, played, stats, mt, pos, kids, after = _parity_roll(net, turn_every)
    monkeypatch.delenv("AO_ROLL_TACTICS_HOLD")
    print("%s: plies %s, solver stats %s" % (tag, played.tolist(), stats))
    assert (played >= 3).all() or any(r["win"] != 0 for r in recs)
    oracle, ref, barred_inherited = _oracle(net, recs, played, 2)
    try:
        _compare(recs, oracle, tag)
        rmt, rpos = _streams(ref)
        rkids = [ref.root_children(g) for g in range(G)]
        rafter = ref.search(net, tau=0) + ref.play()
    finally:
        ref.close()
    np.testing.assert_array_equal(mt, rmt, err_msg="streams after the last ply")
    np.testing.assert_array_equal(pos, rpos, err_msg="stream positions after the last ply")
    for g in range(G):                                               # the roots handed on: the same children with the same statistics
        for key in ("action", "n", "w", "q", "p"):
            np.testing.assert_array_equal(kids[g][key], rkids[g][key], err_msg="%s: root of game %d after the roll: %s" % (tag, g, key))
    live = np.array([not any(int(r["game"]) == g and r["win"] != 0 for r in recs) for g in range(G)])   # (a game that is over is not searched: its rows are not results)
    assert live.any()
    for a, b, what in zip(after, rafter, ("pi", "visit", "policy", "action", "win")):
        bad = np.flatnonzero((np.asarray(a) != np.asarray(b)).reshape(G, -1).any(axis=1) & live)
        assert bad.size == 0, "%s: the synchronous ply behind roll_end: %s differs for games %s (plies played %s)" % (tag, what, bad.tolist(), played.tolist())
    want = _roots()[1]
    for r in recs:
        g, won = int(r["game"]), int(r["verdict"]) == RT_WIN
        assert int(r["sims"]) == (min(BUDGETS[g], SOLVED) if won else BUDGETS[g]), (tag, g, r["rel"])
        assert not r["settled"]
        if r["rel"] == 0:                                            # the fixture's verdicts at the roots themselves
            assert int(r["verdict"]) == int(want["verdict"][g])
    assert any(int(r["verdict"]) == RT_WIN and BUDGETS[r["game"]] > SOLVED for r in recs)
    assert barred_inherited > 0, "no compared move barred a root child that carried inherited visits"
    assert stats["batches"] > 0 and stats["games_solved"] == len(recs) and stats["bytes"] > 0
    assert stats["nodes"] == sum(int(r["nodes"]) for r in recs)
    if hold:
        assert stats["waited_turns"] > 0


@pytest.mark.parametrize("hold", (0, 2))
def test_early_stop(net, hold, monkeypatch):
    """early_stop, tau 0 from the first ply, three plies: the twin with sims = the recorded simulations and no early stop is
    bit-identical; no move ran more than its (capped) budget, and a settled move ran fewer."""
    monkeypatch.setenv("AO_ROLL_TACTICS_HOLD", str(hold))
    eng = _engine()
    try:
        recs, played, stats = _roll(eng, net, 3, 0, TACTICS, early_stop=True, turn_every=2)
        mt, pos = _streams(eng)
    finally:
        eng.close()
    monkeypatch.delenv("AO_ROLL_TACTICS_HOLD")
    print("hold %d: (game, ply, verdict, sims, settled) %s" % (hold, [(int(r["game"]), r["rel"], int(r["verdict"]), int(r["sims"]), int(r["settled"]))
                                                                     for r in recs]))
    for r in recs:
        cap = SOLVED if int(r["verdict"]) == RT_WIN else S
        assert 1 <= int(r["sims"]) <= cap and int(r["tau"]) == 0
        assert bool(r["settled"]) == (int(r["sims"]) < cap), (int(r["game"]), r["rel"])
    oracle, ref, _ = _oracle(net, recs, played, 0)
    try:
        _compare(recs, oracle, "early stop, hold %d" % hold)
        rmt, rpos = _streams(ref)
    finally:
        ref.close()
    np.testing.assert_array_equal(mt, rmt, err_msg="streams after the last ply")
    np.testing.assert_array_equal(pos, rpos, err_msg="stream positions after the last ply")


def test_wiring_on_a_network_that_knows_nothing(flat_net):
    """Uniform priors, value 0, no noise, tau 0, 8 simulations: what such a search gets right about forced wins it was told by
    the solver. On every ply pi and visit are zero outside the record's allowed row and the action lies inside it. A game
    begun on a fixture WIN root of depth d whose verdicts never carry an unknown bit ends in the mover's win within 2d - 1
    plies -- checked first on the host: utils.root_tactics along the lines played says what the records say, for the WIN
    roots' games (no root had to be left out). What the same roll does without the solver is printed."""
    from alpha_omok_amd import utils
    roots, want, nopen = _roots()
    sims = 8
    lines = {}
    for tactics in (dict(LIMITS, allowed=True), None):
        eng = _engine(sims=sims, noise=False)
        try:
            recs, played, _ = _roll(eng, flat_net, 2 * DEPTH - 1, 0, tactics, turn_every=1)
        finally:
            eng.close()
        lines[tactics is not None] = recs
    won_plain = {g: [int(r["win"]) for r in lines[False] if int(r["game"]) == g][-1] for g in range(G)}
    print("without the solver: last win word per game %s" % won_plain)
    recs = lines[True]
    for r in recs:
        assert not r["pi"][~r["allowed"]].any() and not r["visit"][~r["allowed"]].any(), (int(r["game"]), r["rel"])
        assert r["allowed"][int(r["action"])], (int(r["game"]), r["rel"])
    checked = 0
    for g in np.flatnonzero(want["verdict"] == RT_WIN):
        g = int(g)
        mine = sorted((r for r in recs if int(r["game"]) == g), key=lambda r: r["rel"])
        moves = list(roots[g][1:])
        for r in mine:                                               # the host definition along the line played
            h = utils.root_tactics(moves, B, MARK[B], DEPTH, NODES)
            assert (h["verdict"], h["depth"], h["nodes"], h["unknown"]) == tuple(int(r[w]) for w in WORDS), (g, r["rel"])
            np.testing.assert_array_equal(np.asarray(h["allowed"], bool).ravel(), r["allowed"])
            moves.append(int(r["action"]))
        if any(int(r["unknown"]) for r in mine):
            print("game %d: a verdict carried an unknown bit, the line is not held to the bound" % g)
            continue
        d = int(want["depth"][g])
        mover = 1 + (nopen[g] % 2)                                   # win word: 1 black, 2 white; black moves at even plies
        assert int(mine[-1]["win"]) == mover and len(mine) <= 2 * d - 1, (g, d, [int(r["win"]) for r in mine])
        checked += 1
    assert checked > 0


def test_refill_while_others_wait(net, monkeypatch):
    """hold 2, a turn after every launch, budgets that keep the games out of step: when a game ends its slot is reset, seeded and
    joined while others wait for a verdict or search. The joined game is listed in a batch that is held for two turns while the
    others search on, so it WAITS: its reset is refused by name -- and so is the reset of any game that turned in the same
    turn as the one that ended. Every record, the refilled game's second life included, equals the twin's."""
    from alpha_omok_amd.engine import EngineError
    monkeypatch.setenv("AO_ROLL_TACTICS_HOLD", "2")
    budgets = np.array([7, 7, 11, 13, 17, 19, 23, 40], np.int32)
    roots, want, nopen = _roots()
    tactics = dict(LIMITS)
    eng = _engine()
    first, second = [], []                                           # records of the first lives, and of the refilled slot's second life
    refilled, new_seed, refused = None, 4242, False
    try:
        eng.roll_begin(net, tau_plies=nopen + 2, sims=budgets, turn_every=1, visit=True, policy=True, tactics=tactics)
        played, over, drained = np.zeros(G, int), np.zeros(G, bool), False
        played2 = 0
        for _ in range(100000):
            r = eng.roll_run()
            for b in range(len(r["game"])):
                g = int(r["game"][b])
                one = {k: r[k][b] for k in r}
                if g == refilled:
                    one["rel"] = int(r["ply"][b])
                    assert one["rel"] == played2
                    second.append(one)
                    played2 += 1
                    continue
                one["rel"] = int(r["ply"][b]) - int(nopen[g])
                first.append(one)
                played[g] += 1
                over[g] = r["win"][b] != 0
            ended = [int(g) for g, w in zip(r["game"], r["win"]) if w != 0 and int(g) != refilled]
            if refilled is None and ended and not drained:
                refilled = ended[0]
                together = [int(g) for g, w in zip(r["game"], r["win"]) if w == 0]
                for h in together:                                   # turned in the same turn, not over: listed in a batch just now
                    with pytest.raises(EngineError, match="game %d is in a move" % h):
                        eng.reset(np.arange(G) == h)
                    refused = True
                mask = (np.arange(G) == refilled).astype(np.uint8)
                eng.reset(mask)
                eng.seed_games([refilled], [new_seed])
                eng.roll_join(active=mask, tau_plies=2, sims=budgets)
                with pytest.raises(EngineError, match="game %d is in a move" % refilled):
                    eng.reset(mask)                                  # listed just now, its batch is held: it waits for its verdict
            if not drained and refilled is not None and played2 >= 2 and ((played >= 3) | over).all():
                eng.roll_drain()
                drained = True
            if not drained and refilled is None and ((played >= 12) | over).all():
                eng.roll_drain()
                drained = True
            if drained and len(r["game"]) == 0:
                break
        stats = eng.roll_tactics_stats()
        eng.roll_end()
    finally:
        eng.close()
    monkeypatch.delenv("AO_ROLL_TACTICS_HOLD")
    print("refilled slot %s after %d plies, second life %d plies, refusal of a waiting game seen: %s, stats %s"
          % (refilled, 0 if refilled is None else played[refilled], len(second), refused, stats))
    assert refilled is not None, "no game ended within twelve plies"
    assert stats["waited_turns"] > 0 and len(second) >= 2
    # the twin: the first lives ply by ply, then the refilled slot's second life alone, from the empty board and the new seed
    sims1 = {(int(r["game"]), r["rel"]): int(r["sims"]) for r in first}
    ref = _engine()
    try:
        for k in range(int(played.max())):
            active = played > k
            budget = np.array([sims1.get((g, k), 1) for g in range(G)], np.int32)
            tau = (np.ones(G) * (1 if k < 2 else 0)).astype(np.int8)
            pi, vis, pol = ref.search(net, tau=tau, active=active.astype(np.uint8), sims=budget, tactics=dict(LIMITS))
            act, win = ref.play()
            for r in (r for r in first if r["rel"] == k):
                g = int(r["game"])
                np.testing.assert_array_equal(r["pi"], pi[g], err_msg="first life %r" % ((g, k),))
                np.testing.assert_array_equal(r["visit"], vis[g])
                assert (int(r["action"]), int(r["win"])) == (int(act[g]), int(win[g])) and int(r["sims"]) == budgets[g]
        mask = (np.arange(G) == refilled).astype(np.uint8)
        ref.reset(mask)
        ref.seed_games([refilled], [new_seed])
        for r in second:
            budget = np.full(G, int(r["sims"]), np.int32)
            tau = np.full(G, 1 if r["rel"] < 2 else 0, np.int8)
            pi, vis, pol = ref.search(net, tau=tau, active=mask, sims=budget, tactics=dict(LIMITS))
            rt = ref.last_tactics()
            act, win = ref.play()
            np.testing.assert_array_equal(r["pi"], pi[refilled], err_msg="second life, ply %d" % r["rel"])
            np.testing.assert_array_equal(r["visit"], vis[refilled])
            np.testing.assert_array_equal(r["policy"], pol[refilled])
            assert (int(r["action"]), int(r["win"])) == (int(act[refilled]), int(win[refilled]))
            assert int(r["verdict"]) == int(rt["verdict"][refilled]) and int(r["sims"]) == budgets[refilled]
    finally:
        ref.close()


def test_refusals(net):
    from alpha_omok_amd.engine import Engine, EngineError
    import alpha_omok_amd.main as main
    eng = _engine()
    try:
        L, h = eng._L, eng._h
        for depth, nodes in ((17, 512), (-1, 512), (6, 0), (6, 65537)):
            assert L.ao_roll_set_tactics(h, depth, nodes, 0, 0) != 0
            assert b"must be in 1.." in L.ao_last_error(h)
        assert L.ao_roll_set_tactics(h, 6, 512, S + 1, 0) != 0 and b"solved_sims" in L.ao_last_error(h)
        assert L.ao_roll_set_tactics(h, 6, 512, -1, 0) != 0
        assert L.ao_roll_set_tactics(h, 6, 512, S, 0) == 0 and L.ao_roll_set_tactics(h, 0, 0, 0, 0) == 0
        for bad in (dict(max_depth=17), dict(max_nodes=0), dict(solved_sims=S + 1), dict(solved_sims=0), dict(depth=3)):
            with pytest.raises(ValueError):
                eng.roll_begin(net, tactics=bad)
        eng.roll_begin(net, tactics=True)
        assert "verdict" in eng.roll_run(max_launches=1)
        with pytest.raises(EngineError, match="a roll is open"):
            eng.roll_begin(net, tactics=True)                        # ao_roll_set_tactics comes first, and is refused
        assert L.ao_roll_set_tactics(h, 6, 512, 0, 0) != 0 and b"a roll is open" in L.ao_last_error(h)
        with pytest.raises(EngineError, match="a roll is open"):
            eng.root_tactics()
        with pytest.raises(EngineError, match="a roll is open"):
            eng.set_root_bar(np.ones((G, A), np.uint8))
        eng.roll_drain()
        while len(eng.roll_run()["game"]):
            pass
        eng.roll_end()
        eng.set_root_bar(np.ones((G, A), np.uint8))                  # a pending bar still refuses a roll, armed or not
        with pytest.raises(EngineError, match="root bar is pending"):
            eng.roll_begin(net, tactics=True)
        eng.set_root_bar(None)
        eng.roll_begin(net)                                          # disarmed again: today's keys
        assert "verdict" not in eng.roll_run(max_launches=1)
        eng.roll_drain()
        while len(eng.roll_run()["game"]):
            pass
        eng.roll_end()
    finally:
        eng.close()
    # win_mark 6 on a 5x5 board (no line wins: the full board is the only end) is an engine the solver has no rules for
    import pvnet_weights
    from alpha_omok_amd.engine import Net
    small = Net(1, 5, 128, 5, 0)
    small.load_state_dict(pvnet_weights.make_state_dict(1, 5, 128, 5, 3))
    six = Engine(5, 8, 5, games=2, noise=False, win_mark=6)
    try:
        with pytest.raises(EngineError, match="win_mark in 3..5"):
            six.roll_begin(small, tactics=True)
        six.roll_begin(small)                                        # ... which the plain roll does not mind
        six.roll_drain()
        while len(six.roll_run()["game"]):
            pass
        six.roll_end()
    finally:
        six.close()
        small.close()
    keep = main.MAX_CONCURRENT
    try:
        with pytest.raises(ValueError, match="rolling=True"):
            main.configure(board_size=B, n_mcts=16, model=_model(), roll_tactics=True)
        with pytest.raises(ValueError, match="roll_tactics="):
            main.configure(board_size=B, n_mcts=16, model=_model(), rolling=True, tactics=True)
        with pytest.raises(ValueError, match="strict"):
            main.configure(board_size=B, n_mcts=16, model=_model(), rolling=True, roll_tactics=True, strict=True)
    finally:
        _restore(main, keep)


@pytest.mark.parametrize("turn_every", (1,))
def test_guarded_allocations(net, turn_every, monkeypatch):
    """The parity roll under AO_POOL_GUARD=4096 with both fills, hold 2: the batches' buffers are new allocations of ragged
    n x A sizes. No guard is damaged, and the records are identical between the fills and to the unguarded run."""
    from alpha_omok_amd.engine import guard_check
    monkeypatch.setenv("AO_ROLL_TACTICS_HOLD", "2")
    runs = []
    for guard, fill in ((None, None), (4096, 255), (4096, 0x5A)):
        if guard is None:
            monkeypatch.delenv("AO_POOL_GUARD", raising=False)
            monkeypatch.delenv("AO_POOL_FILL", raising=False)
        else:
            monkeypatch.setenv("AO_POOL_GUARD", str(guard))
            monkeypatch.setenv("AO_POOL_FILL", str(fill))
        eng = _engine()
        try:
            recs, played, stats = _roll(eng, net, 3, 2, TACTICS, sims=BUDGETS, turn_every=turn_every)
            mt, pos = _streams(eng)
            if guard is not None:
                blocks, damaged, msg = guard_check()
                assert blocks > 0 and damaged == 0, (fill, msg)
        finally:
            eng.close()
            monkeypatch.delenv("AO_POOL_GUARD", raising=False)
            monkeypatch.delenv("AO_POOL_FILL", raising=False)
        assert guard_check()[1] == 0, "found when the engine was freed (fill %r)" % fill
        runs.append((recs, mt, pos))
    # (how many plies a game plays before the drain depends on when verdicts arrive; a record of a (game, ply) does not)
    ref = {(int(r["game"]), r["rel"]): r for r in runs[0][0]}
    for (recs, mt, pos), tag in zip(runs[1:], ("fill 255", "fill 0x5A")):
        mine = {(int(r["game"]), r["rel"]): r for r in recs}
        common = sorted(set(ref) & set(mine))
        assert all((g, k) in common for g in range(G) for k in range(3) if (g, k) in ref), tag
        for key in common:
            a, b = ref[key], mine[key]
            assert sorted(a) == sorted(b)
            for k in a:
                np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg="%s: %s of %r" % (tag, k, key))
        for g in range(G):
            if sum(1 for key in ref if key[0] == g) == sum(1 for key in mine if key[0] == g):
                np.testing.assert_array_equal(runs[0][1][g], mt[g], err_msg="%s: stream of game %d" % (tag, g))
                assert runs[0][2][g] == pos[g], (tag, g)


# ---- whole games through main ----------------------------------------------------------------------------------------------------------
MS, MN, MSEED = 40, 6, 29
MT = dict(max_depth=6, max_nodes=512, solved_sims=8)


def _model():
    import torch
    from alpha_omok_amd.pvnet import PVNet
    model = PVNet(2, 5, 128, B)
    model.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in _trained_state_dict().items()})
    return model.cuda().eval()


def _configure(main, **kw):
    main.MAX_CONCURRENT = 4                                           # four slots for six episodes: finished slots are refilled
    main.configure(board_size=B, n_mcts=MS, model=_model(), seed=MSEED, strict=False, reproducible=True, **kw)
    main.cur_memory.clear()
    main.rep_memory.clear()


def _restore(main, keep):
    main.MAX_CONCURRENT = keep
    main.configure(board_size=B, n_mcts=16, model=_model(), seed=MSEED, strict=False)
    main.release_engine()


def test_self_play_roll_tactics_equals_synchronous_tactics():
    """reproducible=True: an episode is a function of its seed, so configure(rolling=True, roll_tactics=T) gives the episodes,
    moves and replay samples of configure(tactics=T), entry for entry, with four slots refilled for six episodes."""
    import alpha_omok_amd.main as main
    keep = main.MAX_CONCURRENT
    try:
        runs = []
        for kw in (dict(tactics=dict(MT)), dict(rolling=True, turn_every=3, roll_tactics=dict(MT))):
            _configure(main, **kw)
            eps = main._play_episodes(list(range(MN)), False, lambda ep: (MSEED + ep) & 0xFFFFFFFF, 0)
            _configure(main, **kw)
            out = main.self_play(MN)
            runs.append((eps, out["episodes"], out["moves"], [(np.asarray(s), np.asarray(pi), float(z)) for s, pi, z in main.cur_memory]))
        (e0, n0, m0, mem0), (e1, n1, m1, mem1) = runs
        for x, y, what in zip(e0, e1, ("moves", "lengths", "wins", "episode of sample", "ply of sample", "pi")):
            np.testing.assert_array_equal(x, y, err_msg=what)
        assert (n0, m0) == (n1, m1) == (MN, int(e0[1].sum())) and len(mem0) == len(mem1) > 0
        for (s0, p0, z0), (s1, p1, z1) in zip(mem0, mem1):
            np.testing.assert_array_equal(s0, s1)
            np.testing.assert_array_equal(p0, p1)
            assert z0 == z1
    finally:
        _restore(main, keep)
