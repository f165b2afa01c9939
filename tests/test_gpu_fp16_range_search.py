"""-m gpu: what ao_search does when the network reports AO_NET_FP16_RANGE -- the move is searched again on the fp32-MFMA trunk
with the pre-move MT19937 streams and fresh trees (recover_fp16_range, engine.hip) -- IS the fresh search on that trunk, bit
for bit, under every option a search takes.

The overflowing network is the inner dead channel of tests/fp16_range_nets.py: it leaves the fp16 range without saturating, so
a game is played for some plies with ordinary weights and then searched with the overflowing weights loaded into the same Net
(as the evaluator re-exports). The reference of every case is a SECOND engine with the same seeds that takes the same earlier
plies on the same kernels; at the tested ply its net is put on mode 2, the games of the move are reset and set to their
current ids (fresh trees, streams untouched) and the same call with the same options follows. Equal must be: pi, visits and
priors, the MT19937 state of every game (has_gauss / gauss included), sims_run(), root_children of some games, the play()
that follows and the next ordinary ply on both engines.

Where a THIRD engine is used it repeats the first attempt alone: the dead network (the channel cut off, nothing scaled) on the
same kernels gives the bits of the clamped overflowing one -- a clamped activation and an ordinary one meet the same zero
weight -- without raising the flag. The counters that run over both attempts are its counts plus the reference's."""
import warnings

import numpy as np
import pytest

import fp16_range_nets as N
import net_reference as R

pytestmark = pytest.mark.gpu


def _same(a, b, what=""):
    for i, (x, y) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(x, y, err_msg="%s [%d]" % (what, i))


def _same_rng(a, b, G, what=""):
    for g in range(G):
        x, y = a.get_rng_state(g), b.get_rng_state(g)
        assert np.array_equal(x[0], y[0]) and x[1:] == y[1:], "%s: the stream of game %d differs (pos %r / %r, gauss %r / %r)" % (
            what, g, x[1], y[1], x[2:], y[2:])


def _make(B, G, S, nb, sd, mode, precision, win_mark, seed0, prepare, roots):
    from alpha_omok_amd.engine import Engine, Net
    net = Net(nb, 5, 128, B, 0)
    net.load_state_dict(sd)
    net.set_mode(mode)
    if precision != "fp32":
        assert net.precision(precision) == precision
    eng = Engine(B, S, 5, games=G, noise=True, win_mark=win_mark)
    eng.seed_all(np.arange(G, dtype=np.uint32) + seed0)
    if prepare:
        prepare(eng)
    if roots is not None:
        eng.set_roots(roots)
    return eng, net


def _warned_once(rec):
    return len([w for w in rec if issubclass(w.category, RuntimeWarning) and "fp16 range" in str(w.message)]) == 1


def check_recovery(B, G, S, nb=2, grid=False, precision="fp32", mode=0, plies=2, win_mark=0, seed0=700, prepare=None, roots=None,
                   options=None, third=False, need_over=False, kind="inner"):
    """The scheme of this module's docstring. options(engine, win) -> the keyword arguments of the tested search (built once,
    handed to every engine). Returns what the case may want to look at."""
    base, big = R.case_network(nb, B, 128, grid), N.big_network(nb, B, kind, grid)
    made = [_make(B, G, S, nb, base, mode, precision, win_mark, seed0, prepare, roots) for _ in range(3 if third else 2)]
    engs, nets = [m[0] for m in made], [m[1] for m in made]
    try:
        win = np.zeros(G, np.int32)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            for ply in range(plies):
                outs = [eng.search(net, tau=1) + eng.play() for eng, net in made]
                for o in outs[1:]:
                    _same(outs[0], o, "ply %d" % ply)
                win = np.where(win != 0, win, outs[0][4])
        if need_over:
            assert (win != 0).any() and (win == 0).sum() >= 8, "the case needs games that are over and games that are not"
        kw = dict(options(engs[0], win)) if options else {}
        kw.setdefault("tau", 1)
        active = (np.ones(G, bool) if kw.get("active") is None else np.asarray(kw["active"]).astype(bool)) & (win == 0)
        ids = [(0,) + tuple(engs[0].get_moves(g)) for g in range(G)]
        for eng in engs:
            eng.leaf_tactics_stats(reset=True)
        a, ref = engs[:2]
        na, nr = nets[:2]
        # the engine under test: the overflowing weights on the kernels it was playing on
        na.load_state_dict(big)
        with pytest.warns(RuntimeWarning, match="fp16 range") as rec:
            out_a = a.search(na, **kw)
        assert _warned_once(rec)
        assert a.fp16_range_events() == (1, int(active.sum()))
        assert na.get_mode() == mode and na.status() == 0
        # the reference: fresh trees for the games of the move, the fp32-MFMA trunk
        nr.load_state_dict(big)
        nr.set_mode(2)
        ref.reset(active.astype(np.uint8))
        ref.set_roots(ids, mask=active.astype(np.uint8))
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            out_r = ref.search(nr, **kw)
        assert ref.fp16_range_events() == (0, 0) and nr.status() == 0
        _same(out_a, out_r, "the repeated move")
        assert (out_a[1][active].sum(axis=1) > 0).all()
        _same_rng(a, ref, G, "after the repeated move")
        sa, sr = a.sims_run(), ref.sims_run()
        np.testing.assert_array_equal(sa["sims"], sr["sims"])
        np.testing.assert_array_equal(sa["settled"], sr["settled"])
        for g in sorted({int(x) for x in np.flatnonzero(active)[[0, -1]]} | {0, G // 2}):
            ca, cr = a.root_children(g), ref.root_children(g)
            assert set(ca) == set(cr)
            for key in ca:
                np.testing.assert_array_equal(ca[key], cr[key], err_msg="root_children(%d)[%s]" % (g, key))
        extra = dict(out=out_a, active=active, win=win, engs=engs, nets=nets, kw=kw, stats=None)
        if third:
            t, nt = engs[2], nets[2]
            nt.load_state_dict(N.dead_network(nb, B, kind, grid))
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                t.search(nt, **kw)
            assert t.fp16_range_events() == (0, 0)
            extra["stats"] = [e.leaf_tactics_stats(per_game=True) for e in (a, ref, t)]
        extra["tactics"] = (a.last_tactics(), ref.last_tactics())
        pa, pr = a.play(), ref.play()
        _same(pa, pr, "play() after the repeated move")
        _same_rng(a, ref, G, "after play()")
        # the next ordinary ply
        na.load_state_dict(base)
        nr.load_state_dict(base)
        nr.set_mode(mode)
        assert na.get_mode() == mode
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            nxt = [eng.search(net, tau=1) + eng.play() for eng, net in made[:2]]
        _same(nxt[0], nxt[1], "the ply after")
        _same_rng(a, ref, G, "after the ply after")
        assert a.fp16_range_events() == (1, int(active.sum()))
        return extra
    finally:
        for eng, net in made:
            eng.close()
            net.close()


def test_ply_three_with_inherited_trees_and_games_masked_out():
    """9 x 9, 64 games, the third ply: every game brings a tree along that the repeat must forget; a third of the games sits the
    move out (active=) and keeps its tree and its stream."""
    G = 64
    check_recovery(9, G, 16, plies=2, options=lambda eng, win: dict(active=(np.arange(G) % 3 != 0).astype(np.uint8)))


def test_games_that_are_over_take_no_part_in_the_repeat():
    """4 x 4 with three in a row winning: after six plies some of the 64 games are over (asserted), and a fifth of the others
    is masked out."""
    G = 64
    check_recovery(4, G, 12, plies=6, win_mark=3, need_over=True,
                   options=lambda eng, win: dict(active=(np.arange(G) % 5 != 1).astype(np.uint8)))


def test_per_game_budgets_and_noise_switches_hold_for_the_repeat():
    """sims= and noise= per game; a game with noise off draws nothing for its root: its stream must not move in either attempt"""
    G, S = 64, 16
    sims = 3 + (np.arange(G) * 5) % (S - 2)
    noise = np.arange(G) % 4 != 0
    x = check_recovery(9, G, S, plies=1, options=lambda eng, win: dict(sims=sims, noise=noise, tau=0))
    np.testing.assert_array_equal(x["out"][1].sum(axis=1), sims)            # (trees are fresh: the visits are the budget)
    assert not noise[0] and noise[1]


def test_allowed_masks_hold_for_the_repeat():
    G, B = 64, 9
    A = B * B

    def options(eng, win):
        rs = np.random.RandomState(5)
        allowed = rs.rand(G, A) < 0.4
        for g in range(G):
            mv = eng.get_moves(g)
            empty = np.ones(A, bool)
            empty[mv] = False
            allowed[g, np.flatnonzero(empty)[g % 7]] = True
        return dict(allowed=allowed.astype(np.uint8))

    x = check_recovery(B, G, 16, plies=2, options=options)
    assert not x["out"][1][x["kw"]["allowed"] == 0].any()


@pytest.mark.parametrize("B", (6, 9))
def test_the_bar_left_on_the_device_by_tactics_is_used_again(B):
    """search(tactics=dict(solved_sims=1)) on the forced-win fixture's positions: the solver's bar stays on the device and the
    repeat searches under it, with the budgets of the first attempt; last_tactics() is what the solver said once."""
    from alpha_omok_amd import utils
    from test_forced_defence_host import MARK
    from test_gpu_root_tactics import G, _verdict_roots
    roots, want = _verdict_roots(B)
    assert (want["verdict"] == utils.RT_WIN).any()
    x = check_recovery(B, G, 16, plies=0, win_mark=MARK[B], roots=roots,
                       options=lambda eng, win: dict(tactics=dict(max_depth=6, max_nodes=2000, solved_sims=1), tau=0))
    ta, tr = x["tactics"]
    for key in ta:
        np.testing.assert_array_equal(ta[key], tr[key], err_msg=key)
    np.testing.assert_array_equal(ta["verdict"], want["verdict"])
    won = want["verdict"] == utils.RT_WIN
    vis = x["out"][1]
    assert (vis[won].sum(axis=1) == 1).all() and not vis[~want["allowed"]].any()


def test_early_stop_holds_for_the_repeat():
    x = check_recovery(9, 64, 24, plies=2, options=lambda eng, win: dict(tau=0, early_stop=True, settle_every=4))
    assert x["out"][0].max(axis=1).min() == 1.0                               # tau == 0: one-hot pi


def test_leaf_symmetries_hold_for_the_repeat():
    check_recovery(9, 64, 16, plies=2, prepare=lambda eng: eng.set_leaf_symmetry(0x5eed))


def test_leaf_tactics_hold_for_the_repeat_and_count_both_attempts():
    """set_leaf_tactics(2, 16): the solver's second stream and its proofs belong to the search that is repeated. The counters of
    leaf_tactics_stats() run over BOTH attempts (nothing resets them but reset=True): they are the first attempt's -- the third
    engine's, on the dead network -- plus the reference's."""
    x = check_recovery(9, 64, 16, plies=2, prepare=lambda eng: eng.set_leaf_tactics(2, 16), third=True)
    sa, sr, st = x["stats"]
    assert sr["searched"] > 0 and st["searched"] > 0
    for key in ("searched", "proven", "unknown", "nodes"):
        assert sa[key] == sr[key] + st[key], (key, sa[key], sr[key], st[key])
    np.testing.assert_array_equal(sa["per_game"], sr["per_game"] + st["per_game"])


def test_the_eval_log_counts_both_attempts():
    """eval_log_count() after a repeated move: the rows of the first attempt stay in the log and the repeat's follow them"""
    import torch
    from alpha_omok_amd.engine import Engine, Net
    B, G, S = 9, 64, 8
    A = B * B
    counts = {}
    for name, sd, mode in (("big", N.big_network(2, B, "inner"), 0), ("dead", N.dead_network(2, B, "inner"), 0), ("mode 2", N.big_network(2, B, "inner"), 2)):
        net = Net(2, 5, 128, B, 0)
        net.load_state_dict(sd)
        net.set_mode(mode)
        eng = Engine(B, S, 5, games=G, noise=True)
        eng.seed_all(np.arange(G, dtype=np.uint32) + 31)
        log = torch.zeros(4 * (S + 2) * 2 * (A + 3), dtype=torch.float32, device="cuda:0")
        eng.set_eval_log([0, G - 1], log.data_ptr(), log.numel())
        with warnings.catch_warnings():
            warnings.simplefilter("ignore" if name == "big" else "error")
            eng.search(net, tau=1)
        counts[name] = eng.eval_log_count()
        assert eng.fp16_range_events()[0] == (1 if name == "big" else 0)
        eng.set_eval_log([])
        eng.close()
        net.close()
    assert counts["dead"] > 0 and counts["mode 2"] > 0
    assert counts["big"] == counts["dead"] + counts["mode 2"], counts


def test_a_row_cap_below_the_games_holds_for_the_repeat():
    check_recovery(9, 64, 16, plies=2, prepare=lambda eng: eng.set_row_cap(40))


@pytest.mark.parametrize("B,G,S", [(9, 5, 16), (9, 3072, 12), (15, 64, 8)], ids=["fused-step-G5", "trunk16hb-G3072", "boardh-15x15-G64"])
def test_the_other_regimes_of_the_search(B, G, S):
    check_recovery(B, G, S, plies=1)


def test_two_product_weights():
    check_recovery(9, 64, 16, plies=2, grid=True)


@pytest.mark.parametrize("precision,G,S", [("fp16", 3072, 12), ("fp16-all", 64, 16)])
def test_the_repeat_ignores_the_forward_precision(precision, G, S):
    """Net.precision("fp16") / ("fp16-all"): the one-product kernels report as the others do, and the repeat on mode 2 is the
    fp32-MFMA trunk whatever the precision -- the reference engine's net carries the same precision switch."""
    check_recovery(9, G, S, plies=1, grid=True, precision=precision)


def test_the_flag_may_rise_in_the_middle_of_a_move():
    """10 x 10, 64 games whose roots are one stone on the right edge: the root's own evaluation stays below 65504 / 2, every
    position one move on is beyond 2 x 65504 (float64 reference, asserted here), so the first launch of the move reports
    nothing and a later one does."""
    from alpha_omok_amd.utils import get_state_pt
    B, G = 10, 64
    A = B * B
    edge = [9 + 10 * k for k in range(9)]
    big = N.big_network(2, B, "inner")
    x = np.stack([get_state_pt((0, m), B, 5) for m in edge]).astype(np.float32)
    assert (N.stored_peaks(big, x) < N.LIMIT / 2).all()
    kids = np.stack([get_state_pt((0, m, k), B, 5) for m in edge for k in range(A) if k != m]).astype(np.float32)
    assert (N.stored_peaks(big, kids) > 2 * N.LIMIT).all()
    check_recovery(B, G, 8, plies=0, roots=[(0, edge[g % len(edge)]) for g in range(G)])


@pytest.mark.parametrize("mode", (0, 6))
def test_counters_warnings_and_modes_over_three_events(mode):
    """One warning and (1, active games) per event; the network is back on the mode that was asked for after events 1 and 2 and
    stays on mode 2 from the third on -- also when mode 6 was asked for --; ordinary weights bring it back, and raise nothing."""
    from alpha_omok_amd.engine import Engine, Net
    B, G, S = 9, 64, 8
    net = Net(2, 5, 128, B, 0)
    net.load_state_dict(N.big_network(2, B, "inner"))
    net.set_mode(mode)
    eng = Engine(B, S, 5, games=G, noise=True)
    eng.seed_all(np.arange(G, dtype=np.uint32) + 77)
    try:
        active = (np.arange(G) % 4 != 3).astype(np.uint8)
        n = int(active.sum())
        for k in (1, 2, 3):
            with pytest.warns(RuntimeWarning, match="fp16 range") as rec:
                eng.search(net, tau=1, active=active)
            assert _warned_once(rec)
            eng.play()
            assert eng.fp16_range_events() == (k, k * n)
            assert net.get_mode() == (mode if k < 3 else 2) and net.status() == 0
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            eng.search(net, tau=1, active=active)                  # on mode 2 now: no event, no warning
            eng.play()
            assert eng.fp16_range_events() == (3, 3 * n) and net.get_mode() == 2
            net.load_state_dict(R.case_network(2, B, 128))
            assert net.get_mode() == mode
            eng.search(net, tau=1)
            assert eng.fp16_range_events() == (3, 3 * n) and net.get_mode() == mode and net.status() == 0
    finally:
        eng.close()
        net.close()


def test_the_rolling_search_refuses_and_leaves_the_engine_usable():
    """roll_begin / roll_run on the overflowing network: EngineError naming AO_NET_FP16_RANGE, no game turned, the roll closed,
    the engine outside any move -- and after reset + set_roots an ordinary search on the same engine works, and recovers."""
    from alpha_omok_amd.engine import Engine, EngineError, Net
    B, G, S = 9, 64, 8
    net = Net(2, 5, 128, B, 0)
    net.load_state_dict(R.case_network(2, B, 128))
    eng = Engine(B, S, 5, games=G, noise=True)
    eng.seed_all(np.arange(G, dtype=np.uint32) + 5)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            eng.search(net, tau=1)
            eng.play()
        moves = [eng.get_moves(g) for g in range(G)]
        net.load_state_dict(N.big_network(2, B, "inner"))
        eng.roll_begin(net, tau_plies=4)
        with pytest.raises(EngineError, match="AO_NET_FP16_RANGE"):
            for _ in range(4 * S):
                eng.roll_run()
        assert [eng.get_moves(g) for g in range(G)] == moves
        with pytest.raises(EngineError):
            eng.roll_run()                                          # the roll is closed
        assert net.status() == 0 and eng.fp16_range_events() == (0, 0)
        eng.reset()
        eng.set_roots([(0,) + tuple(m) for m in moves])
        with pytest.warns(RuntimeWarning, match="fp16 range") as rec:
            pi, vis, pol = eng.search(net, tau=1)
        assert _warned_once(rec) and eng.fp16_range_events() == (1, G)
        assert (vis.sum(axis=1) == S).all()
        act, win = eng.play()
        assert [eng.get_moves(g) for g in range(G)] == [m + [int(a)] for m, a in zip(moves, act)]
    finally:
        eng.close()
        net.close()


def test_self_play_in_strict_mode_accounts_for_the_repeated_plies():
    """main.self_play with strict=True, carry_over=True, oversubscribe=1.25 and the overflowing network exported by the evaluator:
    the calls complete, _check_visits accepts the repeated plies (a repeated move starts from fresh trees: S visits, nothing
    inherited) and the events are counted -- three of them, after which the network stays on the fp32-MFMA trunk. The stronger
    statement -- the same games as a run on mode 2 from the start with the carried trees dropped at the plies of the events --
    cannot be arranged through main's public switches (nothing drops a carried tree at a chosen ply), so this test settles for
    completion, the counts and the visit sums that strict mode checks after every search."""
    import random
    from collections import deque
    import torch
    import alpha_omok_amd.main as main
    from alpha_omok_amd.pvnet import PVNet
    B, S, n = 6, 8, 3
    model = PVNet(2, 5, 128, B)
    model.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in N.big_network(2, B, "inner").items()})
    main.MAX_CONCURRENT = 4
    main.rep_memory = deque(maxlen=30000)
    try:
        main.configure(board_size=B, n_mcts=S, n_blocks=2, in_planes=5, out_planes=128, seed=3, model=model.cuda().eval(), node_cap=0,
                       strict=True, carry_over=True, oversubscribe=1.25, rows='auto', overlap_train=False, device_replay=False)
        main.result.update(Black=0, White=0, Draw=0)
        main.cur_memory.clear()
        random.seed(5)
        with pytest.warns(RuntimeWarning, match="fp16 range") as rec:
            rets = [main.self_play(n) for _ in range(2)]
        eng = main._engine
        ev, redone = eng.fp16_range_events()
        warned = len([w for w in rec if "fp16 range" in str(w.message)])
        print("FP16_RANGE self_play: events %d, games searched again %d, warnings %d, G %d, moves %s" % (
            ev, redone, warned, eng.G, [r['moves'] for r in rets]))
        assert eng.G == 5 and all(r['episodes'] == n for r in rets)
        assert ev == 3 and warned == 3 and redone == 3 * eng.G      # (the first three plies: every slot is in its first game)
        assert all(r['moves'] >= 5 * n for r in rets)
    finally:
        main.MAX_CONCURRENT = 4096
        main.rep_memory = deque(maxlen=30000)
        main.configure(board_size=B, n_mcts=S, n_blocks=2, out_planes=128, seed=0, reproducible=False, strict=False, carry_over=False,
                       oversubscribe=1.0, rows='auto', overlap_train=False, device_replay=False)
        main.release_engine()
