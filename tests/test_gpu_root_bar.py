"""-m gpu: the root move restriction (begin_move / search with allowed=) on the STEP-WISE protocol with the oracle's stub
evaluator, S = 40, 8 games, boards 5, 9, 12 and 15 (NCH = 1, 2, 3, 4: every instantiation of k_begin_move and of the root
expansion), and once through the fused search with a native network.

The bar is data in the root's record -- a barred child carries q == BAR_Q, n == 0, w == 0 -- so a barred search is compared
with the unbarred search of a twin engine (same seeds, same roots, same evaluator): the priors are the same numbers, the
barred cells get nothing, and the visits that are made are as many. utils.root_bar is the host definition of which
children are barred."""
import numpy as np
import pytest

from gpu_helpers import HostEvalRunner, children_by_action
from test_gpu_board_sizes import ROOT_STONES, _mid_game_root, _win_mark
from test_gpu_search_budgets import _check_game, _roots

pytestmark = pytest.mark.gpu

S, G = 40, 8
BOARDS = (5, 9, 12, 15)


class Runner(HostEvalRunner):
    """HostEvalRunner.move with the arguments of begin_move; `look` is called once the move has begun, `settle_mask` asks
    for a settle call after every apply_evals."""

    def move_opts(self, eval_fn, tau=None, active=None, sims=None, noise=None, allowed=None, look=None, settle_mask=None):
        e, torch = self.e, self.torch
        e.begin_move(active, sims=sims, noise=noise, allowed=allowed)
        if look is not None:
            look(e)
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
        return e.end_move(tau)


def _stub(oracle, B):
    mode = B % 3
    return lambda g, sim, planes: oracle.stub_eval(planes, mode)


def _engine(B, noise, seeds, roots):
    from alpha_omok_amd.engine import Engine
    mark, _ = _win_mark(B)
    eng = Engine(B, S, 5, games=G, noise=noise, win_mark=mark)
    eng.seed_all(seeds)
    assert (eng.set_roots(roots) >= 0).all()
    return eng, Runner(eng)


def _random_allowed(eng, rs, keep=None):
    """per game between 1 and all-but-1 of the empty cells barred (keep: that many allowed instead); ones on every stone"""
    A = eng.A
    allowed = np.ones((G, A), np.uint8)
    for g in range(G):
        stones = eng.get_moves(g)
        empty = np.setdiff1d(np.arange(A), stones)
        if empty.size < 2:                        # (a game that has ended on a full board: nothing to bar)
            continue
        k = int(rs.randint(1, empty.size)) if keep is None else empty.size - keep
        allowed[g, rs.permutation(empty)[:k]] = 0
    return allowed


def _ids(eng):
    return [(0,) + tuple(eng.get_moves(g)) for g in range(G)]


def _states(eng):
    return [eng.get_rng_state(g)[:2] for g in range(G)]


def _check_barred(eng, allowed, out, tag):
    """no visit and no pi on a barred cell; the barred children read n == 0, w == 0, q == BAR_Q, the others do not"""
    from alpha_omok_amd import utils
    from alpha_omok_amd.engine import BAR_Q
    pi, vis, _ = out
    bar = utils.root_bar(allowed, _ids(eng), eng.board_size)
    assert not vis[bar].any() and not pi[bar].any(), tag
    for g in range(G):
        ch = eng.root_children(g)
        b = bar[g][ch["action"]]
        assert b.sum() == bar[g].sum(), tag
        assert (ch["n"][b] == 0).all() and (ch["w"][b] == 0).all() and (ch["q"][b] == BAR_Q).all(), "%s game %d" % (tag, g)
        assert (ch["q"][~b] != BAR_Q).all() and (np.abs(ch["q"][~b]) <= 1).all(), "%s game %d" % (tag, g)
    return bar


@pytest.mark.parametrize("B", BOARDS)
@pytest.mark.parametrize("form", ("ones", "none"))
def test_no_restriction_is_the_oracle(oracle, B, form):
    """allowed of all ones, and None through the same argument: three plies (tau 1, 1, 0) equal the oracle agents bit for
    bit -- visits, priors, pi, the children's w and q, the action, all 624 MT words and the position."""
    A = B * B
    mark, wm = _win_mark(B)
    roots = _roots(oracle, B, wm, np.random.RandomState(2500 + B))
    seeds = [8100 + 10 * B + g for g in range(G)]
    eng, run = _engine(B, True, seeds, roots)
    agents = []
    for g in range(G):
        a = oracle.Agent(B, S, 5, noise=True, evaluator="stub%d" % (B % 3))
        a.seed(seeds[g])
        a.set_win_mark(wm)
        agents.append(a)
    alive = np.ones(G, np.uint8)
    for t in range(3):
        tau = np.full(G, 1 if t < 2 else 0, np.int8)
        out = run.move_opts(_stub(oracle, B), tau=tau, active=alive, allowed=np.ones((G, A), np.uint8) if form == "ones" else None)
        kids = [children_by_action(eng.root_children(g), A) if alive[g] else None for g in range(G)]
        act, win = eng.play()
        for g in np.flatnonzero(alive):
            tag = "board %d game %d ply %d" % (B, g, t)
            roots[g], ow = _check_game(oracle, eng, agents[g], g, roots[g], tau[g], out, kids[g], act, win, wm, tag)
            assert eng.get_moves(g) == list(roots[g][1:]), tag
            if ow != 0:
                alive[g] = 0
    eng.close()


def _barred_twins(oracle, B, noise, inherited, seed0):
    """The unbarred engine and the barred one, same seeds and roots, through one move (after an unbarred first move and a
    play when `inherited`). Returns everything the barred run handed out, for the run-twice comparison."""
    mark, wm = _win_mark(B)
    roots = _roots(oracle, B, wm, np.random.RandomState(2600 + B + seed0))
    seeds = [8300 + 10 * B + g + seed0 for g in range(G)]
    ev = _stub(oracle, B)
    tau = np.ones(G, np.int8)
    (eu, ru), (eb, rb) = _engine(B, noise, seeds, roots), _engine(B, noise, seeds, roots)
    if inherited:
        for e, r in ((eu, ru), (eb, rb)):
            r.move_opts(ev, tau=tau)
        au, ab = eu.play(), eb.play()
        np.testing.assert_array_equal(au[0], ab[0])
        alive = (au[1] == 0).astype(np.uint8)
    else:
        alive = np.ones(G, np.uint8)
    allowed = _random_allowed(eb, np.random.RandomState(77 + B + seed0))
    before = [eb.root_children(g) for g in range(G)]
    tag = "board %d noise %s %s" % (B, noise, "inherited" if inherited else "fresh")
    out_u = ru.move_opts(ev, tau=tau, active=alive)
    out_b = rb.move_opts(ev, tau=tau, active=alive, allowed=allowed)
    allowed_live = np.where(alive[:, None] != 0, allowed, 1)
    bar = _check_barred(eb, allowed_live, out_b, tag)
    expanded = 0
    for g in np.flatnonzero(alive):
        cu, cb = children_by_action(eu.root_children(g), B * B), children_by_action(eb.root_children(g), B * B)
        assert cu["order"].tolist() == cb["order"].tolist(), tag
        np.testing.assert_array_equal(cu["p"], cb["p"], err_msg=tag + ": the priors of a barred search are the unbarred search's")
        np.testing.assert_array_equal(out_u[2][g], out_b[2][g], err_msg=tag + ": policy")
        was = before[g]["n"][bar[g][before[g]["action"]]].sum()   # visits the barred children had inherited
        assert out_b[1][g].sum() == out_u[1][g].sum() - was, "%s game %d: visits" % (tag, g)
        if before[g]["action"].size:              # an inherited, expanded root: the kept allowed visits + the budget
            expanded += 1
            assert out_b[1][g].sum() == before[g]["n"].sum() - was + S, "%s game %d: visits" % (tag, g)
        if not inherited:
            assert was == 0 and out_b[1][g].sum() == S
    assert expanded >= (4 if inherited else 0), "%s: %d inherited roots were expanded" % (tag, expanded)
    act, win = eb.play()
    assert not bar[np.flatnonzero(alive), act[alive != 0]].any(), tag + ": a barred cell was played"
    res = out_b + (act, win) + tuple(x for s in _states(eb) for x in s)
    eu.close()
    eb.close()
    return res


@pytest.mark.parametrize("B", BOARDS)
@pytest.mark.parametrize("noise", (True, False))
@pytest.mark.parametrize("inherited", (False, True))
def test_random_bars_against_the_unbarred_twin(oracle, B, noise, inherited):
    first = _barred_twins(oracle, B, noise, inherited, 0)
    if B in (9, 12) and noise:                    # two identical runs are bit-equal, streams included
        again = _barred_twins(oracle, B, noise, inherited, 0)
        for x, y in zip(first, again):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("B", BOARDS)
def test_single_allowed_cell_and_a_second_bar_on_the_same_root(oracle, B):
    """One allowed cell: every simulation goes through it and it is played (tau 0 and tau 1 alike). Then the SAME root is
    searched again under another bar: children barred before and allowed now read q == 0, n == 0 when the move begins, and
    two of them that are all the second bar allows share the whole budget."""
    from alpha_omok_amd import utils
    from alpha_omok_amd.engine import BAR_Q
    A = B * B
    mark, wm = _win_mark(B)
    roots = _roots(oracle, B, wm, np.random.RandomState(2700 + B))
    eng, run = _engine(B, True, [8500 + g for g in range(G)], roots)
    rs = np.random.RandomState(5 + B)
    one = _random_allowed(eng, rs, keep=1)
    tau = (np.arange(G) % 2).astype(np.int8)
    pi, vis, _ = run.move_opts(_stub(oracle, B), tau=tau, allowed=one)
    ids = _ids(eng)
    bar1 = utils.root_bar(one, ids, B)
    cell = np.array([int(np.flatnonzero((one[g] != 0) & ~np.isin(np.arange(A), ids[g][1:]))[0]) for g in range(G)])   # the one empty cell allowed
    assert (vis[np.arange(G), cell] == S).all() and (vis.sum(axis=1) == S).all() and (pi[np.arange(G), cell] == 1).all()
    # the same roots again: two cells barred before are all that is allowed now
    two = np.zeros((G, A), np.uint8)
    for g in range(G):
        two[g, rs.permutation(np.flatnonzero(bar1[g]))[:2]] = 1
    seen = {}

    def look(e):
        for g in range(G):
            ch = children_by_action(e.root_children(g), A)
            now = np.flatnonzero(two[g])
            assert (ch["q"][now] == 0).all() and (ch["n"][now] == 0).all() and (ch["w"][now] == 0).all(), "game %d" % g
            assert ch["q"][cell[g]] == BAR_Q and ch["n"][cell[g]] == 0 and ch["w"][cell[g]] == 0, "game %d: the old leader forgets" % g
            seen[g] = True

    pi2, vis2, _ = run.move_opts(_stub(oracle, B), tau=np.ones(G, np.int8), allowed=two, look=look)
    assert len(seen) == G
    assert (vis2[two != 0].reshape(G, 2).sum(axis=1) == S).all() and (vis2.sum(axis=1) == S).all()
    assert (vis2[two != 0] > 0).any()
    act, _ = eng.play()
    assert (two[np.arange(G), act] == 1).all()
    eng.close()


@pytest.mark.parametrize("B", (9, 15))
def test_settling_under_a_bar_never_names_a_barred_leader(oracle, B):
    """A policy with 0.85 on a BARRED cell and 0.1 on one of three allowed cells, value 0, settling after every simulation:
    the games settle on the allowed leader, and sims_run is the number of visits made."""
    A = B * B
    eng, run = _engine(B, False, list(range(G)), [(0,)] * G)
    allowed = _random_allowed(eng, np.random.RandomState(9 + B), keep=3)
    peak = np.array([int(np.flatnonzero(allowed[g] == 0)[g]) for g in range(G)])
    good = np.array([int(np.flatnonzero(allowed[g] == 1)[g % 3]) for g in range(G)])
    pol = np.full((G, A), np.float32(0.05) / np.float32(A - 2), np.float32)
    pol[np.arange(G), peak] = np.float32(0.85)
    pol[np.arange(G), good] = np.float32(0.1)
    tau = np.zeros(G, np.int8)
    pi, vis, _ = run.move_opts(lambda g, sim, planes: (pol[g], np.float32(0.0)), tau=tau, allowed=allowed,
                               settle_mask=np.ones(G, np.uint8))
    ran = eng.sims_run()
    assert ran["settled"].any()
    np.testing.assert_array_equal(vis.sum(axis=1), ran["sims"])
    assert not vis[allowed == 0].any() and not pi[allowed == 0].any()
    lead = vis.argmax(axis=1)
    np.testing.assert_array_equal(lead, good)
    assert (allowed[np.arange(G), lead] == 1).all() and (pi[np.arange(G), lead] == 1).all()
    assert (ran["sims"][ran["settled"]] < S).all()
    act, _ = eng.play()
    np.testing.assert_array_equal(act, lead)
    eng.close()


@pytest.mark.parametrize("B", (9, 12))
def test_export_import_of_a_barred_half_searched_move(oracle, B):
    """Half the budget under a bar, export, import into a second engine, the other half under the same bar on each: the
    snapshot carries the sentinel, and both engines go on bit for bit."""
    from alpha_omok_amd.engine import BAR_Q, Engine
    mark, wm = _win_mark(B)
    roots = _roots(oracle, B, wm, np.random.RandomState(2800 + B))
    a, ra = _engine(B, True, [8700 + g for g in range(G)], roots)
    allowed = _random_allowed(a, np.random.RandomState(3 + B))
    ev = _stub(oracle, B)
    tau = np.ones(G, np.int8)
    ra.move_opts(ev, tau=tau, sims=S // 2, allowed=allowed)
    snap = a.export_trees()
    assert (snap.q == np.float32(BAR_Q)).sum() == (allowed == 0).sum()
    b = Engine(B, S, 5, games=G, noise=True, win_mark=mark)
    b.import_trees(snap)
    rb = Runner(b)
    for t in range(2):
        al = allowed if t == 0 else None          # (t == 1: the sentinels of the imported roots are cleared on both)
        oa, ob = ra.move_opts(ev, tau=tau, sims=S // 2, allowed=al), rb.move_opts(ev, tau=tau, sims=S // 2, allowed=al)
        for x, y in zip(oa, ob):
            np.testing.assert_array_equal(x, y)
        for g in range(G):
            ca, cb = a.root_children(g), b.root_children(g)
            for key in ca:
                np.testing.assert_array_equal(ca[key], cb[key])
            assert ((ca["q"] == BAR_Q).sum() > 0) == (t == 0)
        if t == 1:
            pa, pb = a.play(), b.play()
            np.testing.assert_array_equal(pa[0], pb[0])
        for x, y in zip(_states(a), _states(b)):
            assert x[1] == y[1]
            np.testing.assert_array_equal(x[0], y[0])
    a.close()
    b.close()


def test_fp16_range_recovery_repeats_the_move_under_the_same_bar():
    """A checkpoint whose activations leave the fp16 range (as in test_gpu_net): the fused search repeats the move on the
    fp32-MFMA trunk with fresh trees -- and under the bar of the first attempt, whether it came from the host (allowed=) or
    was left on the device (tactics=, here with nothing proven: the caller's bar alone). The result is the search on the
    fp32-MFMA trunk under that bar."""
    import pvnet_weights
    from alpha_omok_amd.engine import Engine, Net
    B, Sn, Gn = 9, 6, 64
    A = B * B
    sd = pvnet_weights.make_state_dict(2, 5, 128, B, 4)
    big = dict(sd)
    big["bn1.weight"] = (sd["bn1.weight"] * 3.0e5).astype(np.float32)   # conv1 output ~1e5: beyond fp16
    net = Net(2, 5, 128, B, 0)
    net.load_state_dict(big)
    allowed = (np.random.RandomState(12).rand(Gn, A) < 0.5).astype(np.uint8)
    allowed[:, 40] = 1
    seeds = np.arange(Gn, dtype=np.uint32) + 50
    got = []
    for tactics in (None, True):
        net.set_mode(0)
        eng = Engine(B, Sn, 5, games=Gn, noise=True)
        eng.seed_all(seeds)
        with pytest.warns(RuntimeWarning, match="fp16 range"):
            out = eng.search(net, tau=1, allowed=allowed, tactics=tactics)
        assert eng.fp16_range_events() == (1, Gn)
        assert not out[1][allowed == 0].any() and (out[1].sum(axis=1) == Sn).all()
        got.append(out)
        eng.close()
    net.set_mode(2)
    eng = Engine(B, Sn, 5, games=Gn, noise=True)
    eng.seed_all(seeds)
    want = eng.search(net, tau=1, allowed=allowed)
    assert eng.fp16_range_events() == (0, 0)
    for out in got:
        for x, y in zip(out, want):
            np.testing.assert_array_equal(x, y)
    eng.close()
    net.close()


def test_fused_search_oversubscribed_under_a_bar():
    """Engine.search with a native network, 8 games on 4 rows per simulation against 8 rows: the same visits, nothing on a
    barred cell, and the barred children carry the sentinel."""
    import pvnet_weights
    from alpha_omok_amd.engine import Engine, Net
    B, Sn = 9, 24
    net = Net(1, 5, 128, B, 0)
    net.load_state_dict(pvnet_weights.make_state_dict(1, 5, 128, B, 3))
    net.set_mode(6)                               # one kernel family: an evaluation does not depend on the batch it sits in
    got = []
    for cap in (8, 4):
        eng = Engine(B, Sn, 5, games=G, noise=True)
        eng.seed_all(np.arange(900, 900 + G, dtype=np.uint32))
        eng.set_row_cap(cap)
        tau = np.ones(G, np.int8)
        eng.search(net, tau=tau)
        eng.play()
        allowed = _random_allowed(eng, np.random.RandomState(41))
        out = eng.search(net, tau=tau, allowed=allowed)
        _check_barred(eng, allowed, out, "fused, %d rows" % cap)
        assert (out[1].sum(axis=1) >= Sn).all()
        got.append(out + eng.play())
        eng.close()
    for x, y in zip(got[0], got[1]):
        np.testing.assert_array_equal(x, y)
    net.close()
