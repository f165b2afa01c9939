"""-m gpu: the device tree read-out (Engine.tree_lookup / principal_variations / tree_stats, the ZeroAgent.tree view) against the
CPU oracle's tree, bit for bit. Driven like test_gpu_tree_parity.test_multi_game_parity_with_oracle: G games in lock-step with
the oracle's exact-arithmetic stub evaluators, one oracle.Agent per game, same seeds; after every search and again after every
eng.play() EVERY expanded node of the oracle's subtree below the root is looked up on the device in one call.

node_cap = 3 * sims: k_play moves the root in place while nodes_used <= node_cap - sims - 1 = 2 * sims - 1 (the first move
leaves sims + 1 records) and compacts with k_reroot above that (the second move leaves up to 2 * sims + 1); a kept subtree has
fewer nodes than its root has visits, far below 2 * sims - 1 with noisy priors, so nothing is trimmed (asserted)."""
import ctypes as C

import numpy as np
import pytest

from gpu_helpers import HostEvalRunner

pytestmark = pytest.mark.gpu

ABSENT, LEAF, TERMINAL, EXPANDED = 0, 1, 2, 3
G = 6
CASES = [(3, 50, 5), (5, 40, 5), (9, 120, 4), (15, 60, 3)]     # board, sims, plies: NCH 1, 1, 2 and 4
PARAMS = [(b, s, p, mode) for (b, s, p) in CASES for mode in (0, 1)]
_SEEN = {}      # case -> dict(states=set of arena states met, tie=bool, terminal=int, leaf=int)


def _engine(*a, **k):
    from alpha_omok_amd.engine import Engine
    return Engine(*a, **k)


def _subtree(agent, root):
    """id -> children() of every EXPANDED node of the oracle's tree at or below `root` (recursion over children())."""
    out = {}
    stack = [tuple(root)]
    while stack:
        nid = stack.pop()
        ch = agent.children(nid)
        if ch is None or len(ch["order"]) == 0:
            continue
        out[nid] = ch
        for a in ch["order"].tolist():
            if ch["n"][a] > 0:
                stack.append(nid + (a,))
    return out


def _oracle_pv(tree, root, max_len):
    """The line of first maxima of n in stored order, from the oracle's tree. Returns (actions, n, q, met_a_tie)."""
    acts, ns, qs, tie = [], [], [], False
    nid = tuple(root)
    while len(acts) < max_len and nid in tree:
        ch = tree[nid]
        order = ch["order"]
        n = ch["n"][order]
        i = int(np.argmax(n))                  # first maximum
        if n[i] <= 0:
            break
        tie = tie or int((n == n[i]).sum()) > 1
        a = int(order[i])
        acts.append(a)
        ns.append(n[i])
        qs.append(ch["q"][a])
        nid = nid + (a,)
    return acts, ns, qs, tie


def _check_readout(oracle, eng, agents, roots, alive, over, trees, board, wm, seen, tag):
    A = board * board
    ids, games, expect = [], [], []

    def ask(g, nid, st):
        ids.append(tuple(nid))
        games.append(g)
        expect.append(st)

    for g in range(G):
        root, T = roots[g], trees[g]
        if not alive[g]:
            # a finished game keeps no tree; its final id is known (its parent was expanded) but has no record
            ask(g, root, LEAF if over[g] else ABSENT)
            ask(g, root + (A,), ABSENT)
            continue
        assert root in T, tag
        for nid, ch in T.items():
            ask(g, nid, EXPANDED)
            for a in ch["order"].tolist():
                if ch["n"][a] > 0 and nid + (a,) not in T:
                    # visited but never expanded: the oracle must say the move ends the game
                    assert oracle.check_win(oracle.get_board(list(nid + (a,))[1:], board), wm) != 0, tag
                    ask(g, nid + (a,), TERMINAL)
                    seen["terminal"] += 1
        # entries with n == 0 of the root and of the root's expanded children
        rch = T[root]
        firsts = [root] + [root + (a,) for a in rch["order"].tolist() if root + (a,) in T]
        a_leaf = None
        for nid in firsts:
            ch = T[nid]
            for a in ch["order"].tolist():
                if ch["n"][a] == 0:
                    ask(g, nid + (a,), LEAF)
                    seen["leaf"] += 1
                    a_leaf = nid + (a,)
        # ABSENT: below a leaf, an occupied cell, off the board, ids that do not extend the root, an id longer than the board
        if a_leaf is not None:
            free = next(c for c in range(A) if c not in a_leaf[1:])
            ask(g, a_leaf + (free,), ABSENT)
        a0 = int(rch["order"][0])
        ask(g, root + (a0, a0), ABSENT)
        ask(g, root + (A,), ABSENT)
        ask(g, root + (-1,), ABSENT)
        ask(g, root + (a0, A + 7), ABSENT)
        ask(g, (0,) + tuple(range(A)) + (0, 1), ABSENT)
        if len(root) > 1:
            ask(g, root[:-1], ABSENT)
            other = next(c for c in range(A) if c not in root[1:])
            ask(g, root[:-1] + (other,), ABSENT)
            ask(g, root[:-1] + (other, a0), ABSENT)
    r = eng.tree_lookup(ids, games)                     # ONE call for everything, all games
    np.testing.assert_array_equal(r["status"], np.array(expect, np.int32), err_msg=tag)
    for k, (g, nid, st) in enumerate(zip(games, ids, expect)):
        t = "%s game %d id %r" % (tag, g, nid)
        if st != EXPANDED:
            assert r["nchild"][k] == 0, t
            assert (r["child_action"][k] == -1).all() and not r["child_n"][k].any() and not r["child_p"][k].any(), t
        if st == ABSENT:
            assert np.isnan([r["n"][k], r["w"][k], r["q"][k], r["p"][k]]).all(), t
            continue
        root, T = roots[g], trees[g]
        if nid == root:
            assert np.isnan([r["w"][k], r["q"][k], r["p"][k]]).all(), t
            if st == LEAF:
                assert np.isnan(r["n"][k]), t
                continue
            ch = T[nid]
            assert r["n"][k] == 1 + ch["n"].sum(), t
            if len(root) > 1:        # the oracle keeps the root's own entry: its parent's child statistics
                assert r["n"][k] == agents[g].children(root[:-1])["n"][root[-1]], t
        else:
            par, a = T[nid[:-1]], nid[-1]
            assert r["n"][k] == par["n"][a], t
            assert np.float64(r["w"][k]) == par["w"][a] and np.float64(r["q"][k]) == par["q"][a], t
            assert r["p"][k] == par["p"][a], t
            if st != EXPANDED:
                continue
            ch = T[nid]
        order = ch["order"]
        L = len(order)
        assert r["nchild"][k] == L, t
        np.testing.assert_array_equal(r["child_action"][k, :L], order, err_msg=t)
        assert (r["child_action"][k, L:] == -1).all(), t
        np.testing.assert_array_equal(r["child_n"][k, :L], ch["n"][order], err_msg=t)
        np.testing.assert_array_equal(r["child_w"][k, :L].astype(np.float64), ch["w"][order], err_msg=t)
        np.testing.assert_array_equal(r["child_q"][k, :L].astype(np.float64), ch["q"][order], err_msg=t)
        np.testing.assert_array_equal(r["child_p"][k, :L], ch["p"][order], err_msg=t)
        assert not r["child_n"][k, L:].any() and not r["child_p"][k, L:].any(), t
    # stats: the independent host walk (tree_nodes), and the oracle's keys
    st = eng.tree_stats()
    pv = eng.principal_variations()
    short = eng.principal_variations(max_len=2)
    for g in range(G):
        t = "%s game %d" % (tag, g)
        ex, en = eng.tree_nodes(g)
        assert (st["expanded"][g], st["entries"][g]) == (ex, en), t
        root, T = roots[g], trees[g]
        if not alive[g]:
            assert (ex, en, st["nodes_used"][g]) == (0, 0, 0), t
            assert st["depth"][g] == (len(root) - 1 if over[g] else 0), t
            assert pv["len"][g] == 0 and (pv["action"][g] == -1).all(), t
            continue
        assert ex == len(T) and en == 1 + sum(len(ch["order"]) for ch in T.values()), t
        assert st["depth"][g] == max(len(nid) for nid in T), t          # keys one ply below the deepest expanded node
        assert st["nodes_used"][g] >= ex, t
        acts, ns, qs, tie = _oracle_pv(T, root, A)
        seen["tie"] = seen["tie"] or tie
        L = len(acts)
        assert pv["len"][g] == L and (L >= 1 or not T[root]["n"].any()), t     # (a root taken over after its only visit has no line yet)
        np.testing.assert_array_equal(pv["action"][g, :L], acts, err_msg=t)
        np.testing.assert_array_equal(pv["n"][g, :L], ns, err_msg=t)
        np.testing.assert_array_equal(pv["q"][g, :L].astype(np.float64), qs, err_msg=t)
        assert (pv["action"][g, L:] == -1).all() and not pv["n"][g, L:].any(), t
        Ls = min(L, 2)
        assert short["len"][g] == Ls, t
        np.testing.assert_array_equal(short["action"][g, :Ls], acts[:Ls], err_msg=t)
        np.testing.assert_array_equal(short["n"][g, :Ls], ns[:Ls], err_msg=t)
    return st


def _run_case(oracle, board, sims, plies, mode):
    key = (board, sims, plies, mode)
    seen = dict(states=set(), tie=False, terminal=0, leaf=0)
    eng = _engine(board, sims, 5, games=G, noise=True, node_cap=3 * sims)
    run = HostEvalRunner(eng)
    seeds = [1000 + 17 * g for g in range(G)]
    eng.seed_all(seeds)
    agents = [oracle.Agent(board, sims, 5, noise=True, evaluator="stub%d" % mode) for _ in range(G)]
    for g in range(G):
        agents[g].seed(seeds[g])
    roots = [(0,) for _ in range(G)]
    alive = np.ones(G, np.uint8)
    over = np.zeros(G, np.uint8)
    wm = 3 if board == 3 else 5
    # before any search: no game has a tree
    r = eng.tree_lookup([(0,)] * G)
    assert (r["status"] == ABSENT).all()
    st = eng.tree_stats()
    assert not st["expanded"].any() and not st["depth"].any() and not st["nodes_used"].any()
    assert not eng.principal_variations()["len"].any()

    def ev(g, sim, planes):
        return oracle.stub_eval(planes, mode)

    for t in range(plies):
        if not alive.any():
            break
        tau = np.array([1 if t < 2 else 0] * G, np.int8)
        pi, vis, pol = run.move(ev, tau=tau, active=alive)
        res = {}
        for g in range(G):
            if alive[g]:
                res[g] = agents[g].get_pi(roots[g], int(tau[g]))
                # (the search that followed the previous ply's read-outs is the oracle's search: they wrote nothing)
                np.testing.assert_array_equal(vis[g], res[g][1], err_msg="visit game %d ply %d" % (g, t))
                np.testing.assert_array_equal(pol[g], res[g][2], err_msg="policy game %d ply %d" % (g, t))
        trees = [_subtree(agents[g], roots[g]) if alive[g] else {} for g in range(G)]
        st = _check_readout(oracle, eng, agents, roots, alive, over, trees, board, wm, seen, "search ply %d" % t)
        used_before = st["nodes_used"].copy()
        if t == 0:
            assert (st["nodes_used"] == st["expanded"]).all()       # a fresh tree: every record is reachable
            seen["states"].add("fresh")
        act, win = eng.play()
        for g in range(G):
            if not alive[g]:
                continue
            oa = agents[g].rng.choice_p(res[g][0])
            assert act[g] == oa, (g, t)
            roots[g] = roots[g] + (int(oa),)
            ow = oracle.check_win(oracle.get_board(list(roots[g])[1:], board), wm)
            assert win[g] == ow, (g, t)
            if ow != 0:
                alive[g], over[g] = 0, 1
        trees = [{nid: ch for nid, ch in trees[g].items() if nid[:len(roots[g])] == roots[g]} if alive[g] else {} for g in range(G)]
        st = _check_readout(oracle, eng, agents, roots, alive, over, trees, board, wm, seen, "play ply %d" % t)
        for g in range(G):
            if not alive[g]:
                continue
            if st["nodes_used"][g] == used_before[g] and st["nodes_used"][g] > st["expanded"][g]:
                seen["states"].add("in_place")        # the root moved, dead records stay behind it
            if st["nodes_used"][g] == st["expanded"][g] and st["nodes_used"][g] < used_before[g]:
                seen["states"].add("compacted")       # k_reroot copied the subtree into the other arena
        assert eng.trim_stats() == (0, 0)             # nothing forgotten: the oracle comparison stays valid
    eng.close()
    _SEEN[key] = seen
    return seen


@pytest.mark.parametrize("board,sims,plies,mode", PARAMS)
def test_readout_matches_oracle_tree(oracle, board, sims, plies, mode):
    seen = _run_case(oracle, board, sims, plies, mode)
    print("arena states %s, tie on a PV %s, terminal edges %d, leaf entries %d" %
          (sorted(seen["states"]), seen["tie"], seen["terminal"], seen["leaf"]))
    assert "fresh" in seen["states"] and seen["leaf"] > 0


def test_cases_met_every_arena_state_a_tie_and_terminal_edges(oracle):
    """The cases TOGETHER: a fresh tree, a root moved in place with dead records behind it, a tree after k_reroot's compaction
    (each established through tree_stats: nodes_used against expanded); a tie in n on a principal variation; TERMINAL edges."""
    for p in PARAMS:
        if p not in _SEEN:            # (selected alone: run what the parametrised test would have run)
            _run_case(oracle, *p)
    states = set().union(*(s["states"] for s in _SEEN.values()))
    assert states == {"fresh", "in_place", "compacted"}, states
    assert any(s["tie"] for s in _SEEN.values())
    assert sum(s["terminal"] for s in _SEEN.values()) > 0


def _finish_move(run, eval_fn, tau):
    """HostEvalRunner.move without its begin_move: the simulations and end_move of a move that is already open."""
    e, torch = run.e, run.torch
    sim = 0
    while e.sims_left() > 0:
        e.collect_leaves(run.planes.data_ptr())
        e.sync()
        pl = run.planes.cpu().numpy()
        for g in range(e.G):
            run.h_policy[g], run.h_value[g] = eval_fn(g, sim, pl[g])
        run.policy.copy_(torch.from_numpy(run.h_policy))
        run.value.copy_(torch.from_numpy(run.h_value))
        torch.cuda.synchronize()
        e.apply_evals(run.policy.data_ptr(), run.value.data_ptr())
        sim += 1
    return e.end_move(tau)


def test_guards_and_masks(oracle):
    """Inside an open move all three calls fail and touch nothing: the move then runs to the oracle's result. A game index out
    of range fails. Rows of masked-out games are left as the caller filled them."""
    from alpha_omok_amd.engine import EngineError
    B, S, Gn = 5, 40, 4
    A = B * B
    eng = _engine(B, S, 5, games=Gn, noise=True)
    run = HostEvalRunner(eng)
    agents = [oracle.Agent(B, S, 5, noise=True, evaluator="stub1") for _ in range(Gn)]
    for g in range(Gn):
        eng.seed(g, 40 + g)
        agents[g].seed(40 + g)
    ev = lambda g, sim, pl: oracle.stub_eval(pl, 1)  # noqa: E731
    roots = [(0,)] * Gn
    tau = np.ones(Gn, np.int8)
    for t in range(2):
        eng.begin_move()
        for call in (lambda: eng.tree_lookup(roots), lambda: eng.principal_variations(), lambda: eng.tree_stats()):
            with pytest.raises(EngineError, match="inside a move"):
                call()
        pi, vis, pol = _finish_move(run, ev, tau)
        act, _ = eng.play()
        for g in range(Gn):
            opi, ovis, opol = agents[g].get_pi(roots[g], 1)
            np.testing.assert_array_equal(vis[g], ovis)
            np.testing.assert_array_equal(pol[g], opol)
            np.testing.assert_array_equal(pi[g], opi)
            assert act[g] == agents[g].rng.choice_p(opi)
            roots[g] = roots[g] + (int(act[g]),)
            mt, pos, _, _ = eng.get_rng_state(g)
            assert pos == agents[g].rng.pos
    for bad in (-1, Gn):
        with pytest.raises(EngineError, match="out of range"):
            eng.tree_lookup([roots[0]], games=[bad])
    with pytest.raises(EngineError):
        eng.principal_variations(max_len=0)
    with pytest.raises(EngineError):
        eng.principal_variations(max_len=A + 1)
    # masks, at the C ABI: the caller's rows of masked-out games keep the caller's bytes (after a search: every root has a line)
    run.move(ev, tau=tau)
    full_pv, full_st = eng.principal_variations(), eng.tree_stats()
    mask = np.array([1, 0, 0, 1], np.uint8)
    i32p, f32p, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    act = np.full((Gn, A), -77, np.int32)
    n = np.full((Gn, A), -77, np.int32)
    q = np.full((Gn, A), -77.0, np.float32)
    ln = np.full(Gn, -77, np.int32)
    assert eng._L.ao_tree_pv(eng._h, mask.ctypes.data_as(u8p), A, act.ctypes.data_as(i32p), n.ctypes.data_as(i32p),
                             q.ctypes.data_as(f32p), ln.ctypes.data_as(i32p)) == 0
    out = np.full((Gn, 4), -77, np.int32)
    assert eng._L.ao_tree_stats(eng._h, mask.ctypes.data_as(u8p), out.ctypes.data_as(i32p)) == 0
    for g in range(Gn):
        if mask[g]:
            L = int(full_pv["len"][g])
            assert ln[g] == L and L >= 1
            np.testing.assert_array_equal(act[g, :L], full_pv["action"][g, :L])
            np.testing.assert_array_equal(n[g, :L], full_pv["n"][g, :L])
            np.testing.assert_array_equal(q[g, :L], full_pv["q"][g, :L])
            assert (act[g, L:] == -77).all()
            assert out[g].tolist() == [full_st[k][g] for k in ("expanded", "entries", "depth", "nodes_used")]
        else:
            assert (act[g] == -77).all() and (n[g] == -77).all() and (q[g] == -77.0).all() and ln[g] == -77
            assert (out[g] == -77).all()
    masked = eng.tree_stats(mask)
    assert (masked["expanded"][mask == 0] == -1).all() and (masked["expanded"][mask == 1] == full_st["expanded"][mask == 1]).all()
    # NULL outputs are allowed
    g0 = np.zeros(1, np.int32)
    mv = np.array(list(roots[0])[1:], np.int32)
    m0 = np.array([mv.size], np.int32)
    stt = np.zeros(1, np.int32)
    assert eng._L.ao_tree_lookup(eng._h, g0.ctypes.data_as(i32p), mv.ctypes.data_as(i32p), int(mv.size), m0.ctypes.data_as(i32p), 1,
                                 stt.ctypes.data_as(i32p), None, None, None, None, None, None, None) == 0
    assert stt[0] == EXPANDED
    eng.close()


def test_stats_after_native_search_agree_with_host_walk():
    """ao_search with a native network, 64 games x 32 simulations, two moves with a re-rooting between them: tree_stats of all
    games in one launch against the host walk of ao_tree_nodes on a sample of 8 games; PV and root lookup are consistent."""
    import pvnet_weights
    from alpha_omok_amd.engine import Net
    B, S, Gn = 9, 32, 64
    net = Net(1, 5, 32, B, 0)
    net.load_state_dict(pvnet_weights.make_state_dict(1, 5, 32, B, 3))
    eng = _engine(B, S, 5, games=Gn, noise=True)
    eng.seed_all(np.arange(700, 700 + Gn, dtype=np.uint32))
    sample = [0, 1, 7, 20, 31, 32, 50, Gn - 1]
    for t in range(2):
        pi, vis, pol = eng.search(net, tau=np.ones(Gn, np.int8))
        for phase in range(2):
            st = eng.tree_stats()
            for g in sample:
                assert (st["expanded"][g], st["entries"][g]) == eng.tree_nodes(g), (t, phase, g)
            assert (st["expanded"] >= 1).all() and (st["nodes_used"] >= st["expanded"]).all()
            assert (st["depth"] >= t + phase + 1).all()
            r = eng.tree_lookup([(0,) + tuple(eng.get_moves(g)) for g in range(Gn)])
            assert (r["status"] == EXPANDED).all()
            pv = eng.principal_variations(max_len=4)
            np.testing.assert_array_equal(pv["len"] >= 1, r["child_n"].max(axis=1) > 0)
            assert phase == 1 or (pv["len"] >= 1).all()
            np.testing.assert_array_equal(pv["n"][:, 0], r["child_n"].max(axis=1))
            first = r["child_n"].argmax(axis=1)
            has = pv["len"] >= 1
            np.testing.assert_array_equal(pv["action"][has, 0], r["child_action"][np.arange(Gn), first][has])
            if phase == 0:
                np.testing.assert_array_equal(r["n"], 1 + vis.sum(axis=1))
                np.testing.assert_array_equal(pv["n"][:, 0], vis.max(axis=1))
                eng.play()
    eng.close()
    net.close()


class _StubModel:
    """Agent.model stand-in: the oracle's exact-arithmetic stub, batch-capable."""

    def __init__(self, oracle, mode):
        self.oracle, self.mode = oracle, mode

    def eval(self):
        return self

    def __call__(self, x):
        import torch
        xs = x.detach().cpu().numpy().astype(np.float32)
        ps, vs = zip(*(self.oracle.stub_eval(xs[i], self.mode) for i in range(xs.shape[0])))
        return torch.from_numpy(np.stack(ps)), torch.from_numpy(np.array(vs, np.float32))


def test_zero_agent_tree_view(oracle):
    """The reference's read idiom on the drop-in agent: tree[root_id], tree[root_id + (a,)], `in`, KeyError,
    principal_variation() and tree_depth() against the oracle; len(agent.tree) is what it was."""
    from alpha_omok_amd import agents
    agents.PRINT_MCTS = False
    B, S = 9, 60
    A = B * B
    agent = agents.ZeroAgent(B, S, 5, noise=True)
    agent.model = _StubModel(oracle, 1)
    assert (0,) not in agent.tree and len(agent.tree) == 0
    ag = oracle.Agent(B, S, 5, noise=True, evaluator="stub1")
    np.random.seed(11)
    ag.seed(11)
    root = (0,)
    for t in range(3):
        agent.get_pi(root, 1)
        ag.get_pi(root, 1)
        np.testing.assert_array_equal(agent.get_visit(), ag.children(root)["n"])
        T = _subtree(ag, root)
        ch = T[root]
        order = ch["order"].tolist()
        node = agent.tree[root]
        assert node["child"] == order and isinstance(node["child"], list)
        assert isinstance(node["n"], float) and node["n"] == 1 + ch["n"].sum()
        assert isinstance(node["w"], np.float32) and isinstance(node["q"], np.float32) and isinstance(node["p"], np.float64)
        assert np.isnan(node["w"]) and np.isnan(node["q"]) and np.isnan(node["p"])
        assert root in agent.tree
        for a in order:
            e = agent.tree[root + (a,)]
            assert (e["n"], np.float64(e["w"]), np.float64(e["q"]), e["p"]) == (ch["n"][a], ch["w"][a], ch["q"][a], ch["p"][a])
            assert isinstance(e["w"], np.float32) and isinstance(e["p"], np.float64) and isinstance(e["n"], float)
            sub = T.get(root + (a,))
            assert e["child"] == ([] if sub is None else sub["order"].tolist())
            assert root + (a,) in agent.tree
        occupied = root + (order[0], order[0])
        for bad in (occupied, root + (A,), (0, A + 3), root[:-1] if len(root) > 1 else (1,), "x", ()):
            assert bad not in agent.tree
            with pytest.raises(KeyError):
                agent.tree[bad]
        acts, ns, qs, _ = _oracle_pv(T, root, A)
        pa, pn, pq = agent.principal_variation()
        assert pa.tolist() == acts and pn.tolist() == ns and pq.astype(np.float64).tolist() == qs
        pa2, _, _ = agent.principal_variation(max_len=1)
        assert pa2.tolist() == acts[:1]
        assert agent.tree_depth() == max(len(nid) for nid in T)
        assert len(agent.tree) == agent._engine.tree_nodes(0)[1] == 1 + sum(len(c["order"]) for c in T.values())
        root = root + (int(np.argmax(ag.children(root)["n"])),)
    agent.tree.clear()
    assert root not in agent.tree and len(agent.tree) == 0
