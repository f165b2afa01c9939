"""-m gpu: tree snapshots (Engine.export_trees / import_trees, TreeSnapshot, ZeroAgent.save_tree / load_tree). A search resumed
from a snapshot must be bit for bit the search that never stopped.

Driven like test_gpu_tree_readout: G = 6 games in lock-step with the oracle's exact-arithmetic stub evaluators, node_cap =
3 * sims so that k_play moves the root in place after the first move and compacts after the second, and nothing is trimmed.
Engine A plays; before the first move and after every play() it is exported and the snapshot imported into a fresh engine,
which from then on makes every move A makes, with the same evaluations. The oracle follows A throughout: an export wrote nothing."""
import numpy as np
import pytest

from gpu_helpers import HostEvalRunner

pytestmark = pytest.mark.gpu

G = 6
CASES = [(3, 50, 5), (5, 40, 5), (9, 120, 4), (15, 60, 3)]     # board, sims, plies: 1, 1, 2 and 4 edge chunks
PARAMS = [(b, s, p, mode) for (b, s, p) in CASES for mode in (0, 1)]
FRESH, UNEXPANDED, EXPANDED = 0, 1, 2
_SEEN = {}


def _engine(*a, **k):
    from alpha_omok_amd.engine import Engine
    return Engine(*a, **k)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _subtree_ids(agent, root):
    """ids of every EXPANDED node of the oracle's tree at or below `root`."""
    out, stack = [], [tuple(root)]
    while stack:
        nid = stack.pop()
        ch = agent.children(nid)
        if ch is None or len(ch["order"]) == 0:
            continue
        out.append(nid)
        stack.extend(nid + (a,) for a in ch["order"].tolist() if ch["n"][a] > 0)
    return out


def _same_trees(a, b, ids, games, tag, slots_a=None, slots_b=None, imported=True):
    """Every read-out of engine b's games slots_b equals engine a's games slots_a, bitwise (floats compared as bytes).
    ids / games: the lookups, `games` as indices into the slot lists. imported: b's games hold no record the root does not reach."""
    slots_a = list(range(a.G)) if slots_a is None else slots_a
    slots_b = list(range(b.G)) if slots_b is None else slots_b
    ra = a.tree_lookup(ids, [slots_a[g] for g in games])
    rb = b.tree_lookup(ids, [slots_b[g] for g in games])
    for k in ra:
        assert _bits(ra[k]) == _bits(rb[k]), "%s: tree_lookup %s" % (tag, k)
    pa, pb = a.principal_variations(), b.principal_variations()
    sa, sb = a.tree_stats(), b.tree_stats()
    for ga, gb in zip(slots_a, slots_b):
        for k in pa:
            assert _bits(pa[k][ga]) == _bits(pb[k][gb]), "%s: principal_variations %s game %d" % (tag, k, ga)
        for k in ("expanded", "entries", "depth"):
            assert sa[k][ga] == sb[k][gb], "%s: tree_stats %s game %d" % (tag, k, ga)
        if imported:
            assert sb["nodes_used"][gb] == sb["expanded"][gb], "%s: imported game %d holds dead records" % (tag, gb)
        else:
            assert sa["nodes_used"][ga] == sb["nodes_used"][gb], "%s: nodes_used game %d" % (tag, ga)
        ca, cb = a.root_children(ga), b.root_children(gb)
        for k in ca:
            assert _bits(ca[k]) == _bits(cb[k]), "%s: root_children %s game %d" % (tag, k, ga)
        assert a.get_moves(ga) == b.get_moves(gb), tag
    return sa


def _same_streams(a, b, tag, slots_a=None, slots_b=None):
    slots_a = list(range(a.G)) if slots_a is None else slots_a
    slots_b = list(range(b.G)) if slots_b is None else slots_b
    for ga, gb in zip(slots_a, slots_b):
        ma, mb = a.get_rng_state(ga), b.get_rng_state(gb)
        assert _bits(ma[0]) == _bits(mb[0]) and ma[1:3] == mb[1:3] and _bits(np.float64(ma[3])) == _bits(np.float64(mb[3])), \
            "%s: MT19937 state of game %d" % (tag, ga)


def _expected_nbytes(snap, st, g):
    from alpha_omok_amd.snapshot import TreeSnapshot
    nodes = int(st["expanded"][g])
    edges = int(st["entries"][g]) - 1 if nodes > 0 else 0
    return 25 * edges + 12 * nodes + TreeSnapshot.header_nbytes(snap.board)


def _run_case(oracle, board, sims, plies, mode):
    seen = dict(states=set(), fresh=0, unexpanded=0, finished=0, terminal=0)
    eng = _engine(board, sims, 5, games=G, noise=True, node_cap=3 * sims)
    run = HostEvalRunner(eng)
    seeds = [1000 + 17 * g for g in range(G)]
    eng.seed_all(seeds)
    agents = [oracle.Agent(board, sims, 5, noise=True, evaluator="stub%d" % mode) for _ in range(G)]
    for g in range(G):
        agents[g].seed(seeds[g])
    roots = [(0,) for _ in range(G)]
    alive = np.ones(G, np.uint8)
    wm = 3 if board == 3 else 5
    followers = []          # (engine, runner, tag): every one resumed from a snapshot of `eng` and moved along with it since

    def ev(g, sim, planes):
        return oracle.stub_eval(planes, mode)

    def lookups():
        ids, games = [], []
        for g in range(G):
            mine = _subtree_ids(agents[g], roots[g]) if alive[g] else []
            for nid in mine or [roots[g]]:
                ids.append(nid)
                games.append(g)
        return ids, games

    def resume(tag, ids, games):
        """export `eng`, import into a fresh engine, compare every read-out; the new engine follows from here on"""
        st = eng.tree_stats()
        snap = eng.export_trees()
        snap.check()
        assert (snap.games, snap.board, snap.inplanes, snap.win_mark, snap.sims, snap.noise) == (G, board, 5, wm, sims, 1), tag
        for g in range(G):      # the size a game packs to, from the stats pass alone
            assert snap.game_nbytes(g) == _expected_nbytes(snap, st, g), "%s game %d" % (tag, g)
            assert (snap.hdr[g, 0], snap.hdr[g, 1]) == (st["expanded"][g], st["entries"][g] - 1 if st["expanded"][g] else 0), tag
        assert snap.nbytes == sum(_expected_nbytes(snap, st, g) for g in range(G)), tag
        seen["fresh"] += int((snap.hdr[:, 3] == FRESH).sum())
        seen["unexpanded"] += int(((snap.hdr[:, 3] == UNEXPANDED) & (snap.hdr[:, 4] == 0)).sum())
        seen["finished"] += int((snap.hdr[:, 4] != 0).sum())
        seen["terminal"] += int((snap.child == -2).sum())
        b = _engine(board, sims, 5, games=G, noise=True, node_cap=3 * sims)
        b.import_trees(snap)
        _same_trees(eng, b, ids, games, tag)
        _same_streams(eng, b, tag)
        followers.append((b, HostEvalRunner(b), tag))
        return st

    def move_all(tau, t):
        """one move of `eng` and of every follower: outputs, actions and streams equal"""
        pi, vis, pol = run.move(ev, tau=tau, active=alive)
        outs = [r.move(ev, tau=tau, active=alive) for (_, r, _) in followers]
        on = alive != 0          # (the output rows of a game that sits out are per-move buffers, not part of a snapshot)
        for (b, _, tag), (pb, vb, lb) in zip(followers, outs):
            w = "%s, ply %d" % (tag, t)
            assert _bits(pi[on]) == _bits(pb[on]) and _bits(vis[on]) == _bits(vb[on]) and _bits(pol[on]) == _bits(lb[on]), w
        return pi, vis, pol

    def play_all(t):
        act, win = eng.play()
        for (b, _, tag) in followers:
            ab, wb = b.play()
            w = "%s, ply %d" % (tag, t)
            assert _bits(act) == _bits(ab) and _bits(win) == _bits(wb), w
            _same_streams(eng, b, w)
        return act, win

    resume("before the first move", *lookups())
    for t in range(plies):
        if not alive.any():
            break
        tau = np.array([1 if t < 2 else 0] * G, np.int8)
        pi, vis, pol = move_all(tau, t)
        res = {}
        for g in range(G):
            if alive[g]:
                # the search that followed the export is the oracle's search: the export wrote nothing
                res[g] = agents[g].get_pi(roots[g], int(tau[g]))
                np.testing.assert_array_equal(vis[g], res[g][1], err_msg="visit game %d ply %d" % (g, t))
                np.testing.assert_array_equal(pol[g], res[g][2], err_msg="policy game %d ply %d" % (g, t))
                np.testing.assert_array_equal(pi[g], res[g][0], err_msg="pi game %d ply %d" % (g, t))
        used_before = eng.tree_stats()["nodes_used"].copy()
        act, win = play_all(t)
        for g in range(G):
            if not alive[g]:
                continue
            oa = agents[g].rng.choice_p(res[g][0])
            assert act[g] == oa, (g, t)
            roots[g] = roots[g] + (int(oa),)
            ow = oracle.check_win(oracle.get_board(list(roots[g])[1:], board), wm)
            assert win[g] == ow, (g, t)
            mt, pos, _, _ = eng.get_rng_state(g)
            assert pos == agents[g].rng.pos, (g, t)
            np.testing.assert_array_equal(mt, agents[g].rng.state_words(), err_msg="mt game %d ply %d" % (g, t))
            if ow != 0:
                alive[g] = 0
        st = resume("after play %d" % t, *lookups())
        for g in range(G):
            if not alive[g]:
                continue
            if st["nodes_used"][g] == used_before[g] and st["nodes_used"][g] > st["expanded"][g]:
                seen["states"].add("in_place")        # the root moved, dead records stay behind it
            if st["nodes_used"][g] == st["expanded"][g] and st["nodes_used"][g] < used_before[g]:
                seen["states"].add("compacted")       # k_reroot copied the subtree into the other arena
        assert eng.trim_stats() == (0, 0)
    # a root that is known but not expanded: move one game's root to a child no simulation has visited
    for g in range(G):
        ch = eng.root_children(g) if alive[g] else None
        if ch is not None and len(ch["n"]) and (ch["n"] == 0).any():
            a = int(ch["action"][int(np.argmax(ch["n"] == 0))])
            mask = np.zeros(G, np.uint8)
            mask[g] = 1
            ids = [roots[k] + ((a,) if k == g else ()) for k in range(G)]
            for e in [eng] + [b for (b, _, _) in followers]:
                assert e.set_roots(ids, mask)[g] == UNEXPANDED
            roots[g] = ids[g]
            before = seen["unexpanded"]
            resume("a root that is only known", roots, list(range(G)))
            assert seen["unexpanded"] > before
            move_all(np.zeros(G, np.int8), plies)
            play_all(plies)
            resume("after the move from a known root", roots[:0], [])
            break
    eng.close()
    for (b, _, _) in followers:
        b.close()
    _SEEN[(board, sims, plies, mode)] = seen
    return seen


@pytest.mark.parametrize("board,sims,plies,mode", PARAMS)
def test_resume_equals_never_stopping(oracle, board, sims, plies, mode):
    """Parts 1 - 3 of the issue: resume equals never stopping, the export is read-only (the oracle follows engine A through every
    export), and a game's packed size is 25 * edges + 12 * nodes + the fixed header, from tree_stats alone."""
    seen = _run_case(oracle, board, sims, plies, mode)
    print("arena states %s, fresh %d, known-only roots %d, finished %d, terminal edges %d" %
          (sorted(seen["states"]), seen["fresh"], seen["unexpanded"], seen["finished"], seen["terminal"]))
    assert seen["fresh"] >= G


def test_cases_met_every_state(oracle):
    """The cases TOGETHER exported and resumed: a finished game, a root that is known but unexpanded, a fresh game, a terminal
    edge, a root moved in place with dead records behind it, and a compacted arena."""
    for p in PARAMS:
        if p not in _SEEN:            # (selected alone: run what the parametrised test would have run)
            _run_case(oracle, *p)
    total = {k: sum(s[k] for s in _SEEN.values()) for k in ("fresh", "unexpanded", "finished", "terminal")}
    assert all(v > 0 for v in total.values()), total
    states = set().union(*(s["states"] for s in _SEEN.values()))
    assert states == {"in_place", "compacted"}, states


# ---- the side cases run on one small shape --------------------------------------------------------
B5, S5 = 5, 40


class _Played:
    """engine + runner + stub evaluator on the 5x5 board, `plies` moves played"""

    def __init__(self, oracle, games, seed0, plies, node_cap, mode=1):
        self.oracle, self.mode = oracle, mode
        self.eng = _engine(B5, S5, 5, games=games, noise=True, node_cap=node_cap)
        self.run = HostEvalRunner(self.eng)
        self.eng.seed_all([seed0 + 7 * g for g in range(games)])
        for t in range(plies):
            self.move()

    def ev(self, g, sim, planes):
        return self.oracle.stub_eval(planes, self.mode)

    def move(self, begun=False):
        """one move and play(); begun: begin_move has been called already"""
        e = self.eng
        tau = np.ones(e.G, np.int8)
        if not begun:
            out = self.run.move(self.ev, tau=tau)
        else:
            r, torch, sim = self.run, self.run.torch, 0
            while e.sims_left() > 0:
                e.collect_leaves(r.planes.data_ptr())
                e.sync()
                pl = r.planes.cpu().numpy()
                for g in range(e.G):
                    r.h_policy[g], r.h_value[g] = self.ev(g, sim, pl[g])
                r.policy.copy_(torch.from_numpy(r.h_policy))
                r.value.copy_(torch.from_numpy(r.h_value))
                torch.cuda.synchronize()
                e.apply_evals(r.policy.data_ptr(), r.value.data_ptr())
                sim += 1
            out = e.end_move(tau)
        return out + self.eng.play()


def _same_move(ra, rb, rows_a, rows_b, tag):
    for x, y, name in zip(ra, rb, ("pi", "visit", "policy", "action", "win")):
        assert _bits(x[rows_a]) == _bits(y[rows_b]), "%s: %s" % (tag, name)


def test_migration_into_a_running_engine(oracle):
    """Games [4, 1] of A go into slots [0, 3] of a 5-game engine C with another node_cap, mid-game on its own seeds: those slots
    continue like A's games, C's other games exactly as in a twin of C that imported nothing."""
    a = _Played(oracle, G, 300, 2, 3 * S5)
    c, twin = _Played(oracle, 5, 900, 1, 5 * S5), _Played(oracle, 5, 900, 1, 5 * S5)
    snap = a.eng.export_trees().select([4, 1])
    assert snap.games == 2 and snap.hdr[:, 0].tolist() == a.eng.tree_stats()["expanded"][[4, 1]].tolist()
    c.eng.import_trees(snap, games=[0, 3])
    ids = [(0,) + tuple(a.eng.get_moves(g)) for g in (4, 1)]
    _same_trees(a.eng, c.eng, ids, [0, 1], "migrated", [4, 1], [0, 3])
    _same_streams(a.eng, c.eng, "migrated", [4, 1], [0, 3])
    _same_trees(twin.eng, c.eng, [(0,) + tuple(twin.eng.get_moves(g)) for g in (1, 2, 4)], [0, 1, 2], "bystanders", [1, 2, 4], [1, 2, 4], imported=False)
    for t in range(2):
        ra, rc, rt = a.move(), c.move(), twin.move()
        _same_move(ra, rc, [4, 1], [0, 3], "migrated games, move %d" % t)
        _same_move(rt, rc, [1, 2, 4], [1, 2, 4], "bystanders, move %d" % t)
        _same_streams(a.eng, c.eng, "migrated games, move %d" % t, [4, 1], [0, 3])
        _same_streams(twin.eng, c.eng, "bystanders, move %d" % t, [1, 2, 4], [1, 2, 4])
    for x in (a, c, twin):
        x.eng.close()


def test_refusals_leave_the_destination_as_it_was(oracle):
    """Ordinary error returns: nothing is launched, the destination game stays readable and unchanged."""
    from alpha_omok_amd.engine import EngineError
    a = _Played(oracle, G, 300, 2, 3 * S5)
    st = a.eng.tree_stats()
    big = int(np.argmax(st["expanded"]))
    nodes = int(st["expanded"][big])
    assert nodes >= 2
    one = a.eng.export_trees().select([big])
    # keep_max = node_cap - sims - 1 is one less than the game's nodes
    d, twin = _Played(oracle, 2, 500, 1, nodes + S5), _Played(oracle, 2, 500, 1, nodes + S5)

    def unchanged(tag):
        _same_trees(twin.eng, d.eng, [(0,) + tuple(twin.eng.get_moves(g)) for g in range(2)], [0, 1], tag, imported=False)
        _same_streams(twin.eng, d.eng, tag)

    with pytest.raises(EngineError, match=r"node_cap - sims - 1"):
        d.eng.import_trees(one, games=[1])
    unchanged("one node too many")
    roomy = _engine(B5, S5, 5, games=1, noise=True, node_cap=nodes + S5 + 1)     # one more record and it fits
    roomy.import_trees(one)
    assert roomy.tree_stats()["expanded"][0] == nodes
    roomy.close()
    small = _engine(3, S5, 5, games=1, noise=True)
    with pytest.raises(EngineError, match="board"):
        d.eng.import_trees(small.export_trees(), games=[0])
    small.close()
    unchanged("board mismatch")
    for bad in (-1, 2):
        with pytest.raises(EngineError, match="out of range"):
            d.eng.import_trees(one, games=[bad])
    with pytest.raises(EngineError, match="listed twice"):
        d.eng.import_trees(a.eng.export_trees().select([0, 1]), games=[1, 1])
    unchanged("game index")
    d.eng.begin_move()
    with pytest.raises(EngineError, match="inside a move"):
        d.eng.export_trees()
    with pytest.raises(EngineError, match="inside a move"):
        d.eng.import_trees(one, games=[0])
    _same_move(twin.move(), d.move(begun=True), [0, 1], [0, 1], "the move the refused calls interrupted")
    unchanged("after one more move")
    for x in (a, d, twin):
        x.eng.close()


def test_occupied_cell_resets_that_game_and_imports_the_rest(oracle):
    """An edge of the root with an expanded child gets the action of the game's own first move: distinct within its node, so the
    host check passes, but the child's position cannot be built. The import fails, that game is reset, the other one is in."""
    from alpha_omok_amd.engine import EngineError
    a = _Played(oracle, G, 300, 2, 3 * S5)
    full = a.eng.export_trees()
    victim = int(np.argmax(full.hdr[:, 0]))
    other = (victim + 1) % G
    snap = full.select([victim, other])
    assert snap.hdr[0, 0] >= 2 and snap.hdr[0, 2] == 2
    e = int(np.flatnonzero(snap.child[:snap.nchild[0]] >= 0)[0])
    snap.act[e] = snap.moves[0, 0]
    snap.check()
    b = _engine(B5, S5, 5, games=2, noise=True, node_cap=3 * S5)
    with pytest.raises(EngineError, match="occupied"):
        b.import_trees(snap)
    st = b.tree_stats()
    assert (st["expanded"][0], st["nodes_used"][0]) == (0, 0) and b.get_moves(0) == []
    assert b.tree_lookup([(0,)], [0])["status"][0] == 0
    _same_trees(a.eng, b, [(0,) + tuple(a.eng.get_moves(other))], [0], "the other game of the call", [other], [1])
    _same_streams(a.eng, b, "the other game of the call", [other], [1])
    a.eng.close()
    b.close()


def test_fused_search_resumes_bit_for_bit():
    """ao_search with the native network, reproducible mode (one kernel family): two searches, export, import into a second
    engine, two more searches on each -- outputs, actions and streams equal."""
    import pvnet_weights
    from alpha_omok_amd.engine import Net
    B, S, Gn = 9, 32, 64
    net = Net(1, 5, 128, B, 0)
    net.load_state_dict(pvnet_weights.make_state_dict(1, 5, 128, B, 3))
    net.set_mode(6)
    a = _engine(B, S, 5, games=Gn, noise=True)
    a.seed_all(np.arange(700, 700 + Gn, dtype=np.uint32))
    tau = np.ones(Gn, np.int8)
    for t in range(2):
        a.search(net, tau=tau)
        a.play()
    b = _engine(B, S, 5, games=Gn, noise=True)
    b.import_trees(a.export_trees())
    ids = [(0,) + tuple(a.get_moves(g)) for g in range(Gn)]
    _same_trees(a, b, ids, list(range(Gn)), "fused, after the import")
    for t in range(2):
        ra, rb = a.search(net, tau=tau), b.search(net, tau=tau)
        pa, pb = a.play(), b.play()
        _same_move(ra + pa, rb + pb, slice(None), slice(None), "fused, search %d after the import" % t)
        _same_streams(a, b, "fused, search %d after the import" % t)
    a.close()
    b.close()
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


def test_zero_agent_round_trip(oracle, tmp_path):
    """save_tree / load_tree through a file: the loaded agent answers tree[id], principal_variation() and the next get_pi as
    the saved one does."""
    from alpha_omok_amd import agents
    agents.PRINT_MCTS = False
    saved, loaded = agents.ZeroAgent(B5, S5, 5, noise=True), agents.ZeroAgent(B5, S5, 5, noise=True)
    saved.model = loaded.model = _StubModel(oracle, 1)
    np.random.seed(21)
    root = (0,)
    for t in range(2):
        pi = saved.get_pi(root, 1)
        root = root + (int(np.argmax(pi)),)
    path = str(tmp_path / "position.npz")
    saved.save_tree(path)
    loaded.load_tree(path)
    assert loaded.root_id == saved.root_id
    prev = saved.root_id
    ids = [prev] + [prev + (a,) for a in saved.tree[prev]["child"]] + [root]
    for nid in ids:
        x, y = saved.tree[nid], loaded.tree[nid]
        assert x["child"] == y["child"] and all(_bits(x[k]) == _bits(y[k]) for k in ("n", "w", "q", "p")), nid
    assert (root + (root[-1],)) not in loaded.tree and len(loaded.tree) == len(saved.tree)
    for x, y in zip(saved.principal_variation(), loaded.principal_variation()):
        assert _bits(x) == _bits(y)
    assert loaded.tree_depth() == saved.tree_depth()
    state = np.random.get_state()
    pi_s = saved.get_pi(root, 0)
    after = np.random.get_state()
    np.random.set_state(state)
    pi_l = loaded.get_pi(root, 0)
    assert _bits(pi_s) == _bits(pi_l) and _bits(saved.get_visit()) == _bits(loaded.get_visit())
    assert _bits(saved.get_policy()) == _bits(loaded.get_policy())
    assert _bits(after[1]) == _bits(np.random.get_state()[1]) and after[2:] == np.random.get_state()[2:]
    assert loaded.is_real_root == saved.is_real_root
