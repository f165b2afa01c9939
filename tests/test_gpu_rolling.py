"""-m gpu: the rolling search (Engine.roll_*): every game ends its move, plays and begins the next one on its own clock inside
one launch loop, with the trained 2-block 9x9 network on the per-layer kernels (mode 6: a position's evaluation does not depend on
what else is in the batch -- under rolling the batch of a launch mixes games at different plies).

The oracle everywhere is the synchronous path on a fresh engine: the same seeds and openings, search(sims=, tau=) + play() ply by
ply, every game for as many plies as the roll played it, with the budgets the roll's records report. A game's search is strictly
sequential, so per game and ply pi, visit, policy, action and win are equal, and so is every game's stream after its last ply:
assert_array_equal, no tolerance.

`ply` in a record counts the moves on the board, the openings' included; tau_plies is given per game relative to its opening, so
that "tau_plies = k" below means tau 1 for the first k searched plies of every game."""
import numpy as np
import pytest

from test_gpu_fused_parity import _trained_state_dict
from test_gpu_search_early_stop import OPENINGS, SEEDS

pytestmark = pytest.mark.gpu

B, S, G = 9, 40, 8
A = B * B
NOPEN = np.array([len(o) - 1 for o in OPENINGS], np.int32)
BUDGETS = np.array([4, 8, 12, 16, 20, 28, 36, 40], np.int32)      # game 0 runs 4 simulations every ply, game 7 runs 40


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


def _engine(row_cap=0, games=G, seeds=SEEDS, openings=OPENINGS, sims=S):
    from alpha_omok_amd.engine import Engine
    eng = Engine(B, sims, 5, games=games, noise=True)
    eng.seed_all(seeds)
    if openings is not None:
        assert (eng.set_roots(openings) == 0).all()
    if row_cap:
        eng.set_row_cap(row_cap)
    return eng


def _streams(eng):
    st = [eng.get_rng_state(g) for g in range(eng.G)]
    return np.stack([s[0] for s in st]), np.array([s[1] for s in st])


def _roll(eng, net, plies, tau_rel, **kw):
    """Rolls until every game has played `plies` plies (or is over), drains, runs dry, ends. Returns the records in return
    order as a list of dicts (one per record, `rel` = the ply counted from the opening) and the runs' record counts."""
    eng.roll_begin(net, tau_plies=NOPEN[:eng.G] + tau_rel, visit=True, policy=True, **kw)
    recs, played, over, drained = [], np.zeros(eng.G, int), np.zeros(eng.G, bool), False
    for _ in range(100000):
        r = eng.roll_run()
        for b in range(len(r["game"])):
            g = int(r["game"][b])
            one = {k: r[k][b] for k in r}
            one["rel"] = int(r["ply"][b]) - int(NOPEN[g])
            assert one["rel"] == played[g]
            recs.append(one)
            played[g] += 1
            over[g] = r["win"][b] != 0
        if not drained and ((played >= plies) | over).all():
            eng.roll_drain()
            drained = True
        if drained and len(r["game"]) == 0:
            break
    else:
        raise AssertionError("the roll did not run dry")
    eng.roll_end()
    return recs, played


def _oracle(net, recs, played, tau_rel, row_cap=0, **engine_kw):
    """The synchronous run: per relative ply k the games that the roll played at k, with the budgets its records report.
    Returns {(game, rel ply): (pi, visit, policy, action, win)} and the engine (open: the caller reads streams and closes).
    engine_kw: what _engine was given for the roll beyond the row cap (games, seeds, openings, sims)."""
    eng = _engine(row_cap, **engine_kw)
    G = eng.G
    sims = {(int(r["game"]), r["rel"]): int(r["sims"]) for r in recs}
    out = {}
    for k in range(int(played.max())):
        active = played > k
        budget = np.array([sims.get((g, k), 1) for g in range(G)], np.int32)
        tau = np.where(k < tau_rel, 1, 0).astype(np.int8) * np.ones(G, np.int8)
        pi, vis, pol = eng.search(net, tau=tau, active=active.astype(np.uint8), sims=budget)
        act, win = eng.play()
        for g in np.flatnonzero(active):
            out[(int(g), k)] = (pi[g], vis[g], pol[g], int(act[g]), int(win[g]))
    return out, eng


def _compare(recs, oracle, tag):
    assert len(recs) == len(oracle)
    for r in recs:
        key = (int(r["game"]), r["rel"])
        pi, vis, pol, act, win = oracle[key]
        np.testing.assert_array_equal(r["pi"], pi, err_msg="%s %r: pi" % (tag, key))
        np.testing.assert_array_equal(r["visit"], vis, err_msg="%s %r: visit" % (tag, key))
        np.testing.assert_array_equal(r["policy"], pol, err_msg="%s %r: policy" % (tag, key))
        assert (int(r["action"]), int(r["win"])) == (act, win), (tag, key)


@pytest.mark.parametrize("row_cap", (0, 5))
@pytest.mark.parametrize("turn_every", (1, 4))
def test_full_budgets_games_out_of_step(net, turn_every, row_cap):
    """Per-game budgets 4 .. 40, tau 1 for two plies, noise on: every record equals the synchronous search + play of that game's
    ply, the streams end equal, and the games really were out of step."""
    eng = _engine(row_cap)
    try:
        recs, played = _roll(eng, net, 4, 2, sims=BUDGETS, turn_every=turn_every)
        mt, pos = _streams(eng)
        rows = eng.row_stats()
    finally:
        eng.close()
    assert (played >= 4).all() or any(r["win"] != 0 for r in recs)
    for r in recs:
        assert int(r["sims"]) == BUDGETS[r["game"]] and not r["settled"] and int(r["tau"]) == (1 if r["rel"] < 2 else 0)
        assert r["visit"].sum() >= r["sims"]
    print("turn_every %d, row_cap %d: plies played %s, row stats %s" % (turn_every, row_cap, played.tolist(), rows))
    oracle, ref = _oracle(net, recs, played, 2, row_cap)
    try:
        _compare(recs, oracle, "turn_every %d, row_cap %d" % (turn_every, row_cap))
        rmt, rpos = _streams(ref)
    finally:
        ref.close()
    np.testing.assert_array_equal(mt, rmt, err_msg="streams after the last ply")
    np.testing.assert_array_equal(pos, rpos, err_msg="stream positions after the last ply")
    # out of step: in return order game 0 is two plies ahead of a ply that game 7 has not returned yet
    order = [(int(r["game"]), r["rel"]) for r in recs]
    assert any(order.index((0, k + 2)) < order.index((7, k)) for k in range(2) if (0, k + 2) in order and (7, k) in order), order
    assert rows["launches"] > 0 and rows["rows_live"] <= rows["rows_launched"]
    if row_cap:
        assert rows["rows_launched"] == row_cap * rows["launches"]


@pytest.mark.parametrize("row_cap", (0, 5))
@pytest.mark.parametrize("turn_every", (1, 8))
def test_early_stop(net, turn_every, row_cap):
    """early_stop, tau 1 for the first ply only, three plies: the synchronous replay with sims = the recorded simulations of
    every (game, ply) and no early stop is bit-identical; settled <=> fewer simulations than the budget; tau == 1 moves are
    never settled; at least two games settle at their second ply; the engine's totals add up."""
    eng = _engine(row_cap)
    try:
        recs, played = _roll(eng, net, 3, 1, early_stop=True, turn_every=turn_every)
        mt, pos = _streams(eng)
        totals = eng.sims_run()
    finally:
        eng.close()
    print("turn_every %d, row_cap %d: (game, ply, sims, settled) %s" % (turn_every, row_cap, [(int(r["game"]), r["rel"], int(r["sims"]), int(r["settled"]))
                                                                                            for r in recs]))
    for r in recs:
        assert 1 <= int(r["sims"]) <= S
        assert bool(r["settled"]) == (int(r["sims"]) < S), (int(r["game"]), r["rel"])
        assert int(r["tau"]) == (1 if r["rel"] < 1 else 0)
        if r["tau"] == 1:
            assert not r["settled"]
    assert sum(1 for r in recs if r["rel"] == 1 and r["settled"]) >= 2, "the trained network decides at least two moves within 40 simulations"
    assert totals["settled_total"] == sum(1 for r in recs if r["settled"])
    assert totals["saved_total"] == sum(S - int(r["sims"]) for r in recs)
    oracle, ref = _oracle(net, recs, played, 1, row_cap)
    try:
        _compare(recs, oracle, "early stop, turn_every %d, row_cap %d" % (turn_every, row_cap))
        rmt, rpos = _streams(ref)
        assert ref.sims_run()["settled_total"] == 0
    finally:
        ref.close()
    np.testing.assert_array_equal(mt, rmt, err_msg="streams after the last ply")
    np.testing.assert_array_equal(pos, rpos, err_msg="stream positions after the last ply")


@pytest.mark.parametrize("row_cap", (0, 1))
def test_more_launches_than_the_row_counter_ring_has_slots(net, row_cap):
    """The rows of a launch are counted in a ring of 2048 device words, summed up at every turn and zeroed where it wraps. Two
    games on 300 simulations a move, a turn every 4 launches, 8 plies: about 2400 launches (twice that on one row), so the roll
    runs past the wrap. Every record and the final streams equal the synchronous run's, and the ledger counts every launch."""
    kw = dict(games=2, seeds=SEEDS[:2], openings=OPENINGS[:2], sims=300)
    eng = _engine(row_cap, **kw)
    try:
        recs, played = _roll(eng, net, 8, 2, turn_every=4)
        mt, pos = _streams(eng)
        rows = eng.row_stats()
    finally:
        eng.close()
    print("row_cap %d: plies played %s, row stats %s" % (row_cap, played.tolist(), rows))
    for r in recs:
        assert int(r["sims"]) == 300 and not r["settled"]
    oracle, ref = _oracle(net, recs, played, 2, row_cap, **kw)
    try:
        _compare(recs, oracle, "past the ring wrap, row_cap %d" % row_cap)
        rmt, rpos = _streams(ref)
    finally:
        ref.close()
    np.testing.assert_array_equal(mt, rmt, err_msg="streams after the last ply")
    np.testing.assert_array_equal(pos, rpos, err_msg="stream positions after the last ply")
    assert rows["launches"] > 2048, rows
    assert rows["rows_live"] <= rows["rows_launched"]
    if row_cap:
        assert rows["rows_launched"] == row_cap * rows["launches"]


def test_protocol(net):
    """Inside an open roll every call of the engine-wide move protocol raises EngineError naming the roll and leaves the roll
    usable; reset of a game in a move, roll_end with games in a move and roll_begin with a pending bar are refused; the tree
    read-outs agree with root_children between runs; after drain and end export_trees works and a plain search + play goes on
    bit for bit as in the all-synchronous run."""
    from alpha_omok_amd.engine import EngineError
    eng = _engine()
    try:
        snap = eng.export_trees()
        eng.set_root_bar(np.ones((G, A), np.uint8))
        with pytest.raises(EngineError, match="root bar is pending"):
            eng.roll_begin(net)
        eng.set_root_bar(None)
        eng.roll_begin(net, tau_plies=NOPEN + 2, sims=BUDGETS, turn_every=2, visit=True, policy=True)
        one = np.zeros(G, np.uint8)
        one[0] = 1
        refused = {
            "begin_move": lambda: eng.begin_move(), "begin_move_opts": lambda: eng.begin_move(sims=BUDGETS),
            "search": lambda: eng.search(net), "search_opts": lambda: eng.search(net, sims=BUDGETS), "end_move": lambda: eng.end_move(),
            "play": lambda: eng.play(), "settle": lambda: eng.settle(), "collect_leaves": lambda: eng.collect_leaves(),
            "apply_evals": lambda: eng.apply_evals(None, None), "set_root": lambda: eng.set_root(0, [40]),
            "set_roots": lambda: eng.set_roots(OPENINGS), "set_row_cap": lambda: eng.set_row_cap(4),
            "export_trees": lambda: eng.export_trees(), "import_trees": lambda: eng.import_trees(snap),
            "root_tactics": lambda: eng.root_tactics(), "roll_begin": lambda: eng.roll_begin(net),
        }
        recs, played = [], np.zeros(G, int)

        def take(r):
            for b in range(len(r["game"])):
                rec = {k: r[k][b] for k in r}
                rec["rel"] = int(r["ply"][b]) - int(NOPEN[r["game"][b]])
                recs.append(rec)
                played[r["game"][b]] += 1
        for name, call in refused.items():
            with pytest.raises(EngineError, match="a roll is open"):
                call()
            take(eng.roll_run(max_launches=1))                     # ... and the roll goes on
        with pytest.raises(EngineError, match="game 0 is in a move"):
            eng.reset(one)
        with pytest.raises(EngineError, match="game 0 is in a move"):
            eng.seed_games([0], [5])
        with pytest.raises(EngineError, match=r"ao_roll_end: \d+ game\(s\) are still in a move"):
            eng.roll_end()
        # tree read-outs between runs: the root of every game, as root_children shows it
        for _ in range(1000):
            if played.min() >= 2:
                break
            take(eng.roll_run())
        assert played.min() >= 2
        look = eng.tree_lookup([(0,) + tuple(eng.get_moves(g)) for g in range(G)])
        pv = eng.principal_variations(max_len=1)
        stats = eng.tree_stats()
        for g in range(G):
            rc = eng.root_children(g)
            k = len(rc["action"])
            assert look["nchild"][g] == k
            np.testing.assert_array_equal(look["child_action"][g, :k], rc["action"])
            np.testing.assert_array_equal(look["child_n"][g, :k], rc["n"].astype(np.int32))
            if k and rc["n"].max() > 0:
                assert pv["n"][g, 0] == rc["n"].max()
            assert stats["expanded"][g] >= (1 if k else 0)
        eng.roll_drain()
        for _ in range(100000):
            r = eng.roll_run()
            take(r)
            if len(r["game"]) == 0:
                break
        eng.roll_end()
        with pytest.raises(EngineError, match="no roll is open"):
            eng.roll_run()
        after = eng.export_trees()
        assert after.games == G
        pi, vis, pol = eng.search(net, tau=0)
        act, win = eng.play()
        mt, pos = _streams(eng)
    finally:
        eng.close()
    oracle, ref = _oracle(net, recs, played, 2)
    try:
        _compare(recs, oracle, "protocol")
        rpi, rvis, rpol = ref.search(net, tau=0)
        ract, rwin = ref.play()
        rmt, rpos = _streams(ref)
    finally:
        ref.close()
    for a, b, what in ((pi, rpi, "pi"), (vis, rvis, "visit"), (pol, rpol, "policy"), (act, ract, "action"), (win, rwin, "win"), (mt, rmt, "stream"),
                       (pos, rpos, "stream position")):
        np.testing.assert_array_equal(a, b, err_msg="the synchronous ply behind the roll: " + what)


def test_turn_traffic_is_per_turned_game(net):
    """64 games, one on budget 1 and the rest on 40, a turn after every launch: the turn that turns the one game moves less than
    a tenth of what the streams of all games weigh -- nothing [G]-wide but the sixteen bytes per game it decides from."""
    n = 64
    eng = _engine(games=n, seeds=np.arange(91000, 91000 + n, dtype=np.uint32), openings=None)
    try:
        budgets = np.full(n, S, np.int32)
        budgets[0] = 1
        eng.roll_begin(net, sims=budgets, turn_every=1)
        drained = False
        r = eng.roll_run()
        st = eng.roll_stats()
        assert r["game"].tolist() == [0] and st["last_games"] == 1 and int(r["sims"][0]) == 1
        print("one game of %d turned: %d bytes (all streams: %d)" % (n, st["last_bytes"], 624 * 4 * n))
        assert st["last_bytes"] < 624 * 4 * n // 10
        for _ in range(4):                                            # game 0 again, alone: one simulation per ply
            r = eng.roll_run()
            st = eng.roll_stats()
            assert r["game"].tolist() == [0] and st["last_games"] == 1 and st["last_bytes"] < 624 * 4 * n // 10
        # Turns of many games: bytes <= 16 G + c k for a turn of k games. 16 G: the four words per game the turn decides from.
        # c, per turned game: its index up (4) and its record down (32 + 8 A for pi; no visit / policy asked for here), its stream
        # down (624 words + the position) and, for its next move, stream and noise row up (+ 8 Ap) and the begin item (24).
        # 64 bytes of slack hold what does not grow with either: the row counter of the launch behind the last turn.
        c = 4 + 32 + 8 * A + (624 * 4 + 4) + (624 * 4 + 4 + 8 * 96) + 24
        most = 0
        while True:
            r = eng.roll_run()
            st = eng.roll_stats()
            k = int(r["game"].size)
            if k == 0:                                                # (a run without a launch bound comes back empty only when nothing is in a move)
                break
            assert st["last_games"] == k and st["last_bytes"] <= 16 * n + 64 + c * k, (k, st)
            most = max(most, k)
            if most >= n // 2 and not drained:
                eng.roll_drain()
                drained = True
        print("largest turn: %d of %d games" % (most, n))
        assert most >= n // 2                                         # the 63 games on 40 simulations come due together
        eng.roll_end()
        st = eng.roll_stats()
        assert st["games_turned"] >= n + 4 and st["bytes"] > 0
    finally:
        eng.close()


# ---- whole games through main: refill, early stop, playout cap, carry-over ------------------------------------------------------------
MS, MN, MSEED = 16, 10, 23                                            # simulations, episodes of a call, seed


def _model():
    import torch
    from alpha_omok_amd.pvnet import PVNet
    model = PVNet(2, 5, 128, B)
    model.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in _trained_state_dict().items()})
    return model.cuda().eval()


def _configure(main, **kw):
    main.MAX_CONCURRENT = 4                                           # G = 4 slots for 10 episodes: finished slots are refilled
    main.configure(board_size=B, n_mcts=MS, model=_model(), seed=MSEED, strict=True, reproducible=True, **kw)
    main.cur_memory.clear()
    main.rep_memory.clear()


def _episodes(main):
    out = main._play_episodes(list(range(MN)), False, lambda ep: (MSEED + ep) & 0xFFFFFFFF, 0)
    assert main._engine.G == 4
    return out


def _restore(main, keep):
    main.MAX_CONCURRENT = keep
    main.roll_sims_log = None
    main.configure(board_size=B, n_mcts=MS, model=_model(), seed=MSEED, strict=False)
    main.release_engine()


@pytest.mark.parametrize("variant", ("plain", "playout_cap"))
def test_self_play_rolling_equals_synchronous(variant):
    """reproducible=True: an episode is a function of its seed, so rolling=True gives the moves, lengths, winners and pi samples
    of rolling=False, episode by episode, with four slots refilled for ten episodes; with the playout cap the set of recorded
    plies is the same as well. Then the same through self_play: the samples in cur_memory."""
    import alpha_omok_amd.main as main
    keep = main.MAX_CONCURRENT
    kw = dict(fast_sims=4, full_prob=0.5) if variant == "playout_cap" else {}
    try:
        _configure(main, **kw)
        sync = _episodes(main)
        totals = dict(main.playout_totals)
        _configure(main, rolling=True, turn_every=3, **kw)
        roll = _episodes(main)
        for x, y, what in zip(sync, roll, ("moves", "lengths", "wins", "episode of sample", "ply of sample", "pi")):
            np.testing.assert_array_equal(x, y, err_msg=what)
        assert main.playout_totals == totals and totals["full"] == sync[3].shape[0]
        if variant == "playout_cap":
            assert 0 < totals["full"] < int(sync[1].sum())
        mem = []
        for rolling in (False, True):
            _configure(main, rolling=rolling, **kw)
            out = main.self_play(MN)
            mem.append((out["episodes"], out["moves"], [(np.asarray(s), np.asarray(pi), float(z)) for s, pi, z in main.cur_memory]))
        assert mem[0][:2] == mem[1][:2] == (MN, int(sync[1].sum())) and len(mem[0][2]) == len(mem[1][2]) == sync[3].shape[0]
        for (s0, p0, z0), (s1, p1, z1) in zip(mem[0][2], mem[1][2]):
            np.testing.assert_array_equal(s0, s1)
            np.testing.assert_array_equal(p0, p1)
            assert z0 == z1
    finally:
        _restore(main, keep)


def test_self_play_rolling_early_stop_equals_synchronous_with_its_budgets(monkeypatch):
    """early_stop=True: when a rolling search looks is not when the synchronous one does, so the simulations run differ. The
    comparison chosen here is the replay: the rolling call logs the simulations of every (episode, ply) (main.roll_sims_log), and
    a synchronous call WITHOUT early stop is given exactly those budgets (a wrapper around main._search_opts, in this test only):
    moves, lengths, winners and every pi are bit-identical. Searches did settle, only tau == 0 ones, never beyond the budget."""
    import alpha_omok_amd.main as main
    keep = main.MAX_CONCURRENT
    try:
        _configure(main, rolling=True, turn_every=2, early_stop=True)
        main.roll_sims_log = log = []
        roll = _episodes(main)
        main.roll_sims_log = None
        ran = {(e, p): k for e, p, k, _ in log}
        assert len(ran) == len(log) == int(roll[1].sum())
        settled = [(e, p, k) for e, p, k, s in log if s]
        print("rolling early-stop self-play: %d of %d searches settled" % (len(settled), len(log)))
        assert settled and all(p >= main.TAU_THRES and 1 <= k < MS for e, p, k in settled)
        assert all(k == MS for e, p, k, s in log if not s)
        _configure(main)
        plain_opts = main._search_opts

        def opts_with_budgets(eng, gids, ply, tau):
            opts, full = plain_opts(eng, gids, ply, tau)
            opts["sims"] = np.array([ran.get((int(e), int(p)), 1) for e, p in zip(gids, ply)], np.int32)
            return opts, full
        monkeypatch.setattr(main, "_search_opts", opts_with_budgets)
        sync = _episodes(main)
        for x, y, what in zip(sync, roll, ("moves", "lengths", "wins", "episode of sample", "ply of sample", "pi")):
            np.testing.assert_array_equal(x, y, err_msg=what)
    finally:
        monkeypatch.undo()
        _restore(main, keep)


def test_self_play_rolling_carry_over():
    """carry_over=True over two consecutive self_play calls: each call returns its own episodes' samples, the same under
    rolling=True as under rolling=False, while games of the next call stay in flight between moves across the call boundary."""
    import alpha_omok_amd.main as main
    keep = main.MAX_CONCURRENT
    try:
        mem = []
        for rolling in (False, True):
            _configure(main, rolling=rolling, turn_every=3, carry_over=True)
            calls = []
            for _ in range(2):
                main.cur_memory.clear()
                out = main.self_play(MN)
                calls.append((out["episodes"], out["moves"], [(np.asarray(s), np.asarray(pi), float(z)) for s, pi, z in main.cur_memory]))
            assert main._pool is not None
            mem.append(calls)
        for c0, c1 in zip(mem[0], mem[1]):
            assert c0[:2] == c1[:2] and c0[0] == MN and len(c0[2]) == len(c1[2]) == c0[1]
            for (s0, p0, z0), (s1, p1, z1) in zip(c0[2], c1[2]):
                np.testing.assert_array_equal(s0, s1)
                np.testing.assert_array_equal(p0, p1)
                assert z0 == z1
    finally:
        _restore(main, keep)


def test_rolling_configure_refusals():
    import alpha_omok_amd.main as main
    keep = main.MAX_CONCURRENT
    try:
        with pytest.raises(ValueError, match="tactics"):
            main.configure(board_size=B, n_mcts=MS, model=_model(), rolling=True, tactics=True)
        with pytest.raises(ValueError, match="native form"):
            main.configure(board_size=B, n_mcts=MS, model=lambda x: None, rolling=True)
        with pytest.raises(ValueError, match="turn_every"):
            main.configure(board_size=B, n_mcts=MS, model=_model(), rolling=True, turn_every=0)
    finally:
        _restore(main, keep)
