"""-m gpu: per-game budgets and settling inside the fused search (ao_search_opts) with the trained 2-block 9x9 network.

The regimes of the search loop: the fused few-game step (k_step_board; planned on the per-board network path only), rows
packed per move, rows handed out per simulation, and the same over-subscribed (5 rows for 8 games: games sit out, leaves
wait, the catch-up rounds run). A game's search is strictly sequential in all of them, so the same seeds and budgets give
the same visits and streams; and an early-stopped search is bit for bit the search with budgets equal to what it ran."""
import os

import numpy as np
import pytest

from test_gpu_fused_parity import _trained_state_dict

pytestmark = pytest.mark.gpu

B, S, G = 9, 40, 8
A = B * B
BUDGETS = np.array([1, 2, 3, 7, 16, 23, 39, 40], np.int32)
OPENINGS = [(0,), (0, 40), (0, 40, 41), (0, 30, 31, 39), (0,), (0, 20, 60), (0, 40, 31, 50, 22), (0, 44, 36)]
SEEDS = np.arange(81000, 81000 + G, dtype=np.uint32)


@pytest.fixture(scope="module")
def net():
    from alpha_omok_amd.engine import Net
    n = Net(2, 5, 128, B, 0)
    n.load_state_dict(_trained_state_dict())
    yield n
    n.close()


def _two_plies(net, row_cap=0, fused_step=True, ply1=None, ply2=None, tau2=None):
    """A fresh engine, the openings, SEEDS; ply 1 with tau 1 and ply 2 with tau2, each with its own Engine.search keywords.
    Returns per ply (pi, visits, priors, action, win, sims_run dict, streams [G, 624], stream positions)."""
    from alpha_omok_amd.engine import Engine
    eng = Engine(B, S, 5, games=G, noise=True)
    eng.seed_all(SEEDS)
    assert (eng.set_roots(OPENINGS) == 0).all()
    if row_cap:
        eng.set_row_cap(row_cap)
    old = os.environ.get("AO_FUSED_STEP")
    if not fused_step:
        os.environ["AO_FUSED_STEP"] = "0"                        # (read per search: the per-board path without the fused per-game step)
    res = []
    try:
        for tau, kw in ((np.ones(G, np.int8), ply1 or {}), (np.ones(G, np.int8) if tau2 is None else tau2, ply2 or {})):
            pi, vis, pol = eng.search(net, tau=tau, **kw)
            ran = eng.sims_run()
            act, win = eng.play()
            st = [eng.get_rng_state(g) for g in range(G)]
            res.append((pi, vis, pol, act, win, ran, np.stack([s[0] for s in st]), np.array([s[1] for s in st])))
            assert (win == 0).all()                              # (nobody wins within two plies of these openings)
    finally:
        if not fused_step:
            if old is None:
                del os.environ["AO_FUSED_STEP"]
            else:
                os.environ["AO_FUSED_STEP"] = old
        rows = eng.row_stats()
        eng.close()
    return res, rows


def _same(a, b, tag, what=(0, 1, 2, 3, 6, 7)):
    names = ("pi", "visits", "priors", "action", "win", "", "stream", "stream position")
    for ply in range(2):
        for i in what:
            np.testing.assert_array_equal(a[ply][i], b[ply][i], err_msg="%s, ply %d: %s" % (tag, ply + 1, names[i]))


def _check_visit_sums(res, budgets, tag):
    """sum(visits) == inherited + budget: a fresh root brings nothing, the root of ply 2 was expanded by the first of the n visits
    of the move played at ply 1 and brings n - 1."""
    p1, p2 = res
    np.testing.assert_array_equal(p1[1].sum(axis=1), budgets[0], err_msg=tag + " ply 1")
    inherited = np.maximum(p1[1][np.arange(G), p1[3]] - 1, 0)
    np.testing.assert_array_equal(p2[1].sum(axis=1), inherited + budgets[1], err_msg=tag + " ply 2")


@pytest.mark.parametrize("mode", (3, 6))
def test_budgets_hold_in_every_regime_of_the_search(net, mode):
    """Budgets {1, 2, 3, 7, 16, 23, 39, 40} (reversed at ply 2), the same seeds: identical visits, pi, priors, actions and
    streams in every regime of the loop, and sum(visits) == inherited + budget per game. One kernel family per mode, so that
    the batch size does not pick the arithmetic: mode 3 is the per-board path for every batch -- the only one on which the
    fused per-game step is planned (8 games: k_step_board; without it: rows packed per move; 5 rows: handed out per
    simulation, over-subscribed) --, mode 6 the per-layer kernels (rows packed per move; handed out per simulation, 8 rows;
    over-subscribed, 5 rows)."""
    net.set_mode(mode)
    try:
        kw1, kw2 = dict(sims=BUDGETS), dict(sims=BUDGETS[::-1].copy())
        tau2 = np.array([0, 1] * (G // 2), np.int8)
        if mode == 3:
            regimes = {"fused step": dict(), "packed rows": dict(fused_step=False), "over-subscribed": dict(row_cap=5)}
        else:
            regimes = {"packed rows": dict(), "rows per simulation": dict(row_cap=G), "over-subscribed": dict(row_cap=5)}
        got = {name: _two_plies(net, ply1=kw1, ply2=kw2, tau2=tau2, **r) for name, r in regimes.items()}
        first = next(iter(got))
        for name, (res, rows) in got.items():
            _check_visit_sums(res, (BUDGETS, BUDGETS[::-1]), "mode %d, %s" % (mode, name))
            for ply in range(2):
                assert res[ply][5]["sims"].tolist() == (BUDGETS if ply == 0 else BUDGETS[::-1]).tolist()
                assert not res[ply][5]["settled"].any()
            if name != first:
                _same(res, got[first][0], "mode %d, %s vs %s" % (mode, name, first))
        assert got["over-subscribed"][1]["launches"] > 0 and got[first][1]["launches"] == 0
        # the full budget everywhere and the noise switch on everywhere: the plain call's bits
        plain, _ = _two_plies(net, tau2=tau2)
        full = dict(sims=np.full(G, S, np.int32), noise=np.ones(G, np.uint8))
        _same(_two_plies(net, ply1=full, ply2=full, tau2=tau2)[0], plain, "mode %d, full budgets vs the plain call" % mode)
        _check_visit_sums(plain, (S, S), "mode %d, plain" % mode)
    finally:
        net.set_mode(0)


@pytest.mark.parametrize("row_cap", (0, 5))
@pytest.mark.parametrize("every", (1, 8))
def test_early_stop_equals_the_search_with_the_budgets_it_ran(net, row_cap, every):
    """Ply 2, tau 0 for six games and 1 for two, early_stop=True (the tau == 0 games), looked at every 1 / 8 simulations, rows
    packed per move / over-subscribed:
      A  early stop; B  fresh engine, same seeds, budgets = sims_run of A, no early stop: bit-identical visits, pi, priors,
      actions, streams; C  full budgets: the same action for every tau == 0 game, and the tau == 1 games bit-identical to A.
    At ply 1 every tau is 1: early_stop=True changes nothing there. settle_every = 0 is the plain search. A settled game ends
    with its pending leaf backed up (done == target): no ERR_SHORT."""
    from alpha_omok_amd.utils import move_decided
    net.set_mode(6)
    try:
        tau2 = np.array([0, 0, 0, 0, 0, 0, 1, 1], np.int8)
        es = dict(early_stop=True, settle_every=every)
        a, _ = _two_plies(net, row_cap=row_cap, ply1=es, ply2=es, tau2=tau2)
        c, _ = _two_plies(net, row_cap=row_cap, tau2=tau2)
        ran1, ran2 = a[0][5], a[1][5]
        print("row_cap %d, settle_every %d: simulations run at ply 2: %s, settled %s" % (row_cap, every, ran2["sims"].tolist(),
                                                                                        ran2["settled"].astype(int).tolist()))
        assert ran1["sims"].tolist() == [S] * G and not ran1["settled"].any()
        for i in (0, 1, 2, 3, 6, 7):
            np.testing.assert_array_equal(a[0][i], c[0][i], err_msg="ply 1 (tau 1 everywhere) with early_stop=True")
        # what settled, and what did not
        assert ran2["sims"][6:].tolist() == [S, S] and not ran2["settled"][6:].any()
        assert (ran2["sims"] <= S).all() and (ran2["sims"] >= 1).all()
        assert ((ran2["sims"] < S) == ran2["settled"]).all()
        assert ran2["settled"][:6].sum() >= 2, "the trained network decides at least two of six moves within 40 simulations"
        assert ran2["settled_total"] == int(ran2["settled"].sum()) and ran2["saved_total"] == int((S - ran2["sims"]).sum())
        if every == 8 and row_cap == 0:
            assert all(int(k) % 8 == 1 for k in ran2["sims"][ran2["settled"]])   # looked at after 8, 16, ... launches: one pending leaf more
        b, _ = _two_plies(net, row_cap=row_cap, ply2=dict(sims=ran2["sims"]), tau2=tau2)
        _same(b, a, "budgets = sims_run vs early stop")
        assert not b[1][5]["settled"].any()
        np.testing.assert_array_equal(a[1][3][:6], c[1][3][:6], err_msg="move of the full search")
        for g in np.flatnonzero(ran2["settled"]):               # a settled game's move is the only maximum of the full search's visits
            assert int(np.argmax(a[1][0][g])) == int(np.argmax(c[1][1][g])) and int((c[1][1][g] == c[1][1][g].max()).sum()) == 1
        for i in (0, 1, 2, 3):
            np.testing.assert_array_equal(a[1][i][6:], c[1][i][6:], err_msg="tau == 1 games are untouched")
        np.testing.assert_array_equal(a[1][6][6:], c[1][6][6:])
        if every == 1 and row_cap == 0:
            # the stop came as early as the rule allows: decided with the pending leaf still out (budget k - 1), not a look earlier
            k = ran2["sims"]
            on = ran2["settled"]
            d1, _ = _two_plies(net, ply2=dict(sims=np.where(on, k - 1, k)), tau2=tau2)
            d2, _ = _two_plies(net, ply2=dict(sims=np.where(on & (k > 2), k - 2, k)), tau2=tau2)
            for g in np.flatnonzero(on):
                assert move_decided(d1[1][1][g], S - (k[g] - 1)), g
                if k[g] > 2:
                    assert not move_decided(d2[1][1][g], S - (k[g] - 2)), g
        off, _ = _two_plies(net, row_cap=row_cap, ply1=dict(early_stop=True, settle_every=0), ply2=dict(early_stop=True, settle_every=0),
                            tau2=tau2)
        _same(off, c, "settle_every = 0 vs the plain search")
        assert not off[1][5]["settled"].any()
    finally:
        net.set_mode(0)
