"""-m gpu: the paths only a SEARCH reaches, at history depths other than 2 (inplanes = 3, 7, 9 beside the 5 every other test
runs), held to float64.

tests/test_gpu_net_precision.py feeds float planes to ao_net_forward at every plane count. What ao_search runs is not
reachable that way: the bit-plane conv1s (k_trunk16hb, k_layer16h<.., 2>, k_boardh<.., 2>: one byte per cell, plane c = bit c),
the fused per-game step (k_step_board: conv1 as K = tap * 8 + plane, built only for up to 8 planes) and, at nine planes, which
do not fit a byte, the float-plane fallback with three live channel quads. Here the evaluation log (Engine.set_eval_log) hands
back the (p, v) the fused loop itself evaluated each leaf with; the oracle replays the search from them bit for bit, and in
the replay gives the planes of every leaf, on which net_reference.forward says in float64 what (p, v) should have been.

The bound is that of tests/test_gpu_net_precision.py for the split-fp16 families: 16 x E32 in centred log p and atanh v, E32
the float32-vs-float64 distance of the plain reference over the same leaves (floor net_reference.E32_FLOOR). The networks are
net_reference.case_network(2, B, 128, False, C), whose conditioning tests/test_net_reference.py asserts on the CPU; that the
search's own leaves are boards on which an error shows (min p, max |z|) is asserted here on the reference before anything of
the device is compared. With AO_PRECISION_REPORT=<file> every comparison appends its figures as a JSON line
(profiles/r17a_forward_precision_by_inplanes.txt keeps a copy)."""
import json
import os

import numpy as np
import pytest

import net_reference as R

pytestmark = pytest.mark.gpu

MULT = 16        # x E32: net_reference.Case.mult of the split-fp16 families, which every 128-plane network runs on
S = 24
OPENING = 10     # random stones every game of the search test starts from: from an empty board two plies of search set the
                 # three youngest history planes only (at C = 9 five planes, bits 0 .. 4 of a cell's byte, stay empty, and z of
                 # the float64 reference has a standard deviation of 0.01 over the leaves); after 10 plies every plane is in use


def _four_in_a_window(stones, B):
    """stones: 0/1 boards [n, B, B] -> True where some window of five cells in a row holds four or more of them."""
    bad = np.zeros(len(stones), bool)
    for dy, dx in ((0, 1), (1, 0), (1, 1), (1, -1)):
        h, w, x0 = B - 4 * dy, B - 4 * abs(dx), 4 if dx < 0 else 0
        s = sum(stones[:, k * dy:k * dy + h, x0 + k * dx:x0 + k * dx + w] for k in range(5))
        bad |= (s >= 4).reshape(len(stones), -1).any(axis=1)
    return bad


def opening_ids(C, G, B):
    """One opening of OPENING random moves per game, drawn again while either colour has four stones in a window of five:
    no game can then end within the two plies of the test, and the number of active games stays what the planner was asked for."""
    A = B * B
    rs = np.random.RandomState(1000 * C + G)
    moves = np.stack([rs.permutation(A)[:OPENING] for _ in range(G)])
    while True:
        bad = np.zeros(G, bool)
        for colour in (0, 1):
            stones = np.zeros((G, A), np.int32)
            np.put_along_axis(stones, moves[:, colour::2], 1, axis=1)
            bad |= _four_in_a_window(stones.reshape(G, B, B), B)
        if not bad.any():
            return [(0,) + tuple(m.tolist()) for m in moves]
        for g in np.flatnonzero(bad):
            moves[g] = rs.permutation(A)[:OPENING]


def _report(rec):
    print("PRECISION " + json.dumps(rec))
    if os.environ.get("AO_PRECISION_REPORT"):
        with open(os.environ["AO_PRECISION_REPORT"], "a") as f:
            f.write(json.dumps(rec) + "\n")


def _net(B, C):
    from alpha_omok_amd.engine import Net
    net = Net(2, C, 128, B, 0)
    net.load_state_dict(R.case_network(2, B, 128, False, C))
    return net


def _evals_of(rec, k, A):
    """Records of listed game k (rows [launch, n, A + 3]) -> its (policy, value, status) per simulation, as
    test_gpu_fused_parity._evals_of reads them (status 3: a terminal leaf, whose evaluation the search discards)."""
    out, last_done = [], None
    for r in rec[:, k]:
        st, done = int(r[A + 2]), int(r[A + 1])
        if st not in (1, 2, 3):
            continue
        if last_done is not None and done != 0:
            assert done == last_done + 1, (done, last_done)
        last_done = done
        out.append((r[:A].copy(), np.float32(r[A]), st))
    return out


def _against_float64(sd, planes, p, v, tag):
    """(p, v) float32 of the device on `planes` [n, C, B, B] against net_reference.forward: the conditions first, on the
    reference alone, then the distances in units of E32. Returns the record that is reported."""
    import torch
    x = np.ascontiguousarray(planes, np.float32)
    o64, o32 = R.forward(sd, x), R.forward(sd, x, torch.float32)
    p64 = torch.softmax(o64["logits"], dim=1)
    assert p64.min().item() >= 1e-8 and o64["z"].abs().max().item() <= 1.5, (tag, p64.min().item(), o64["z"].abs().max().item())
    l64, z64 = R.centred(o64["logits"]).numpy(), o64["z"].numpy()
    el = max(float(np.abs(R.centred(o32["logits"].double()).numpy() - l64).max()), R.E32_FLOOR)
    ez = max(float(np.abs(o32["z"].double().numpy() - z64).max()), R.E32_FLOOR)
    p, v = np.asarray(p, np.float64), np.asarray(v, np.float64)
    assert np.isfinite(p).all() and np.isfinite(v).all() and p.min() > 0 and np.abs(v).max() < 1, tag
    lp = np.log(p)
    err_l = float(np.abs(lp - lp.mean(axis=1, keepdims=True) - l64).max())
    err_z = float(np.abs(np.arctanh(v) - z64).max())
    return dict(tag, n=len(x), mult=MULT, E32_l=el, E32_z=ez, err_l=err_l, err_z=err_z, ratio_l=err_l / el, ratio_z=err_z / ez,
                z_spread=float(z64.std()), distinct=len(np.unique(x.reshape(len(x), -1), axis=0)))


def _assert_within(rec):
    _report(rec)
    assert rec["err_l"] <= MULT * rec["E32_l"] and rec["err_z"] <= MULT * rec["E32_z"], \
        "%s: centred logits off by %.2f x E32 (%.2e), atanh v by %.2f x E32 (%.2e); allowed %d x" % (
            rec["id"], rec["ratio_l"], rec["err_l"], rec["ratio_z"], rec["err_z"], MULT)


def planned(C, G):
    """(the kind of planes ao_search hands the network at C input planes, the kernel the planner must name for G boards)"""
    in_kind = 2 if C <= 8 else 1                # nine planes do not fit the byte of a cell: float planes, three channel quads
    trunk = "k_trunk16hb<9, 4, 0>" if in_kind == 2 else "k_trunk16h<9, 4, 0>"
    return in_kind, {5: "k_conv_cells_h<9, 8>", 40: "k_row16hk<9>", 3072: trunk}[G]


@pytest.mark.parametrize("G", [5, 40, 3072])
@pytest.mark.parametrize("C", [3, 7, 9])
def test_search_evaluations_against_float64(C, G, oracle):
    """ao_search at C input planes, two plies (tau = 1, then 0) of S = 24 simulations from random openings, with as many
    active games as put the planner on the per-board path with the fused per-game step (5; at C = 9 its three-launch form:
    the step's conv1 packing is built for up to 8 planes), the per-layer kernels (40) and the resident trunk (3072). Four logged games: the oracle, fed the logged (p, v), reproduces visits, priors, pi,
    action and MT19937 position bit for bit; every logged evaluation is within 16 x E32 of float64 on the planes the oracle
    built for that leaf."""
    import torch
    from alpha_omok_amd.engine import Engine, plan_kernel
    B = 9
    A = B * B
    in_kind, kernel = planned(C, G)
    assert plan_kernel(2, C, 128, B, G, in_kind)[0].startswith(kernel)
    net = _net(B, C)
    eng = Engine(B, S, C, games=G, noise=True)
    seeds = np.arange(81000 + 100 * C, 81000 + 100 * C + G, dtype=np.uint32)
    eng.seed_all(seeds)
    sample = sorted({0, 1, G // 2, G - 1})
    assert len(sample) == 4
    log = torch.zeros(((S + 8) * len(sample) * (A + 3),), dtype=torch.float32, device="cuda")
    recs, cursor = {}, {}
    leaves, got_p, got_v = [], [], []

    def make_agent(g):
        def replay(moves, pl, sim, g=g):
            p, v, st = recs[g][cursor[g]]
            cursor[g] += 1
            if st != 3:
                leaves.append(np.array(pl, np.float32))
                got_p.append(p)
                got_v.append(v)
            return p, v
        ag = oracle.Agent(B, S, C, noise=True, evaluator=replay)
        ag.seed(int(seeds[g]))
        return ag

    agents = {g: make_agent(g) for g in sample}
    ids = opening_ids(C, G, B)
    assert (eng.set_roots(ids) == 0).all()                                # nothing was known: fresh roots
    roots = {g: ids[g] for g in sample}
    for t in range(2):
        tau = np.full(G, 1 if t == 0 else 0, np.int8)
        eng.set_eval_log(sample, log.data_ptr(), log.numel())
        pi, vis, pol = eng.search(net, tau=tau)
        n_rec = eng.eval_log_count()
        assert n_rec == S + (1 if t == 0 else 0)
        rec = log[:n_rec * len(sample) * (A + 3)].cpu().numpy().reshape(n_rec, len(sample), A + 3)
        act, win = eng.play()
        assert np.all(win == 0)
        for k, g in enumerate(sample):
            tag = "C %d, %d games, game %d, ply %d" % (C, G, g, t)
            recs[g], cursor[g] = _evals_of(rec, k, A), 0
            assert len(recs[g]) == n_rec, tag
            opi, ovis, opol = agents[g].get_pi(roots[g], int(tau[g]))
            assert cursor[g] == n_rec, tag
            np.testing.assert_array_equal(vis[g], ovis, err_msg=tag)
            np.testing.assert_array_equal(pol[g], opol, err_msg=tag)
            np.testing.assert_array_equal(pi[g], opi, err_msg=tag)
            oa = agents[g].rng.choice_p(opi)
            assert act[g] == oa, tag
            roots[g] = roots[g] + (int(oa),)
            mt, pos, _, _ = eng.get_rng_state(g)
            assert pos == agents[g].rng.pos, tag
            np.testing.assert_array_equal(mt, agents[g].rng.state_words(), err_msg="mt " + tag)
    eng.set_eval_log([])
    assert net.status() == 0
    eng.close()
    net.close()
    x = np.stack(leaves)
    assert 4 * 2 * S <= len(x) <= 4 * (2 * S + 1) and x.shape[1:] == (C, B, B) and set(np.unique(x)) <= {0.0, 1.0}   # (a few may be terminal)
    for c in range(C - 1):                       # a history plane nobody ever set could be dropped unseen
        assert x[:, c].any(), c
    assert {0.0, 1.0} == set(x[:, C - 1, 0, 0].tolist())
    rec = _against_float64(R.case_network(2, B, 128, False, C), x, np.stack(got_p), np.array(got_v),
                           dict(id="search_leaves-C%d-G%d" % (C, G), family="search_leaves", kernel=kernel, C=C, B=B, batch=G, in_kind=in_kind))
    assert rec["distinct"] >= 2 * S and rec["z_spread"] > 0.02, rec        # (leaves of a search are near one another, not one board)
    _assert_within(rec)


@pytest.mark.parametrize("B,G,Sims", [(9, 64, 24), (9, 3072, 12), (15, 40, 16)])
def test_search_at_nine_planes_equals_the_stepwise_protocol(B, G, Sims):
    """C = 9: ao_search cannot hand the network a byte per cell, and takes the float-plane interleaved batch with three live
    channel quads. It must agree bit for bit with the stepwise protocol (collect_leaves -> net(planes) -> apply_evals), which
    goes through k_nchw_to_il: the layout of test_gpu_net.test_fused_search_on_bit_planes_equals_stepwise_on_float_planes, on
    the per-layer kernel, the resident trunk and a wide board, conditioned weights."""
    import torch
    from alpha_omok_amd.engine import Engine
    C = 9
    net = _net(B, C)
    net.set_mode(5)
    seeds = np.arange(40, 40 + G, dtype=np.uint32)
    e1 = Engine(B, Sims, C, games=G, noise=True)
    e2 = Engine(B, Sims, C, games=G, noise=True)
    e1.seed_all(seeds)
    e2.seed_all(seeds)
    planes = torch.zeros((G, C, B, B), dtype=torch.float32, device="cuda")
    for t in range(3):
        tau = np.full(G, 1 if t < 2 else 0, np.int8)
        pi1, vis1, pol1 = e1.search(net, tau=tau)
        e2.begin_move()
        while e2.sims_left() > 0:
            e2.collect_leaves(planes.data_ptr())
            e2.sync()
            p, v = net(planes)
            torch.cuda.synchronize()
            e2.apply_evals(p.data_ptr(), v.data_ptr())
        pi2, vis2, pol2 = e2.end_move(tau)
        np.testing.assert_array_equal(vis1, vis2)
        np.testing.assert_array_equal(pol1, pol2)
        np.testing.assert_array_equal(pi1, pi2)
        a1, w1 = e1.play()
        a2, w2 = e2.play()
        np.testing.assert_array_equal(a1, a2)
        np.testing.assert_array_equal(w1, w2)
    assert len(np.unique(pol1.round(6), axis=0)) > G // 4            # the priors move with the position
    assert net.status() == 0
    e1.close()
    e2.close()
    net.close()


@pytest.mark.parametrize("C", [1, 4, 8, 9])
def test_position_batch_evaluate_against_float64(C):
    """PositionBatch(9, inplanes=C).evaluate builds the planes on the device (one history plane per earlier ply, then the colour)
    and runs the native forward on them: against float64 on utils.get_state_pt of the same ids, at the bound of the kernel the
    planner names for the batch."""
    from alpha_omok_amd import utils
    from alpha_omok_amd.engine import plan_kernel
    from alpha_omok_amd.positions import PositionBatch
    from test_gpu_positions import _game_ids
    B, n = 9, 40
    kernel = plan_kernel(2, C, 128, B, n, in_kind=1)[0].split(" (")[0]
    assert R.is_split_fp16(kernel), kernel                                   # MULT is the split-fp16 families'
    ids = _game_ids(B, n, seed=40 + C)
    x = np.stack([utils.get_state_pt(i, B, C) for i in ids]).astype(np.float32)
    net = _net(B, C)
    with PositionBatch(B, inplanes=C) as pb:
        pol, val, status, err = pb.evaluate(net, ids)
    assert not err.any() and status[1] == 1 and status[n // 2] == 1
    assert net.status() == 0
    net.close()
    rec = _against_float64(R.case_network(2, B, 128, False, C), x, pol, val,
                           dict(id="positions_evaluate-C%d" % C, family="positions_evaluate", kernel=kernel, C=C, B=B, batch=n, in_kind=1))
    assert rec["distinct"] == (n if C > 1 else 2), rec["distinct"]           # (one plane: the colour alone)
    _assert_within(rec)


def test_plane_counts_outside_a_handle_s_range_are_refused():
    from alpha_omok_amd.engine import Engine, EngineError, Net
    for C in (13, 0):
        with pytest.raises(EngineError, match=r"1\.\.12"):
            Net(2, C, 128, 9)
    with pytest.raises(EngineError, match="3, 5, 7 or 9"):
        Engine(9, 8, 4)


def test_search_refuses_a_network_of_another_plane_count():
    from alpha_omok_amd.engine import Engine, EngineError
    net = _net(9, 5)
    eng = Engine(9, 8, 7, games=2)
    with pytest.raises(EngineError, match="network board/inplanes differ"):
        eng.search(net, tau=1)
    eng.close()
    net.close()
