"""-m gpu: what a re-rooting by copying (k_reroot) keeps, forgets and counts, against the definition restated on the host.

Every play() re-roots by copying (AO_COMPACT_ALWAYS=1) inside an arena of node_cap = sims + 1 + keep_max records. The trees are
exported before and after the move; from the export BEFORE it the host walks the played child's subtree breadth first with a
plain queue -- children in stored edge order, every followable child takes the next number, a child is kept if and only if its
number is below keep_max -- and the export AFTER the move must be exactly that tree, bit for bit, and trim_stats() must have
grown by exactly what the walk dropped. (export_trees is held to the oracle by test_gpu_tree_snapshot / test_gpu_tree_readout.)

The evaluator is a peaked stub -- the oracle's mode-1 policy to the fourth power, its mode-2 (small) value -- and every move is
the most visited one (tau = 0), so the played child keeps much of the root's visits. Seeds 700 + 13 * game and CUT were chosen on
the CPU with the oracle, which predicts the first re-rooting of every case exactly: on every board the first played subtrees
hold 11 - 22 nodes (more than eight), keep_max = CUT falls inside a breadth-first level and inside a node's edge row, and on the
boards with more than one 64-edge chunk a kept child hangs on a stored edge index >= 64. Later moves inherit larger trees."""
import numpy as np
import pytest

from gpu_helpers import HostEvalRunner

pytestmark = pytest.mark.gpu

G, SIMS, PLIES = 4, 48, 4
SEEDS = [700 + 13 * g for g in range(G)]
CUT, ROOMY = 10, 200                       # ROOMY > PLIES * SIMS: nothing is ever dropped
BOARDS = [8, 9, 12, 15]                    # 1, 2, 3, 4 chunks of 64 edges
PARAMS = [(b, k) for b in BOARDS for k in (1, CUT, ROOMY)]
CH_UNVISITED = -1
_NODE = ("nchild", "parent", "parent_edge")
_EDGE = ("act", "n", "w", "q", "p", "child")
_SEEN = {}


def peaked_eval(oracle, planes):
    p, _ = oracle.stub_eval(planes, 1)
    _, v = oracle.stub_eval(planes, 2)
    p = p * p
    return p * p, v


def _games_of(snap):
    """per game: dict of its node and edge arrays (views) + `first` (a node's first edge inside the game)"""
    n1 = np.concatenate([[0], np.cumsum(snap.hdr[:, 0], dtype=np.int64)])
    e1 = np.concatenate([[0], np.cumsum(snap.hdr[:, 1], dtype=np.int64)])
    out = []
    for g in range(snap.games):
        t = {k: getattr(snap, k)[n1[g]:n1[g + 1]] for k in _NODE}
        t.update({k: getattr(snap, k)[e1[g]:e1[g + 1]] for k in _EDGE})
        t["first"] = np.concatenate([[0], np.cumsum(t["nchild"], dtype=np.int64)])[:-1]
        out.append(t)
    return out


def _expected(t, action, keep_max):
    """The tree a re-rooting on `action` leaves of tree t, and what the walk saw: (tree, dropped children, coverage flags)."""
    cov = dict(rounds=False, row_cut=False, far_edge=False)
    empty = {k: np.zeros(0, t[k].dtype) for k in _NODE + _EDGE}
    if len(t["nchild"]) == 0:
        return empty, 0, cov
    hit = np.flatnonzero(t["act"][:t["nchild"][0]] == action)
    if hit.size == 0 or t["child"][hit[0]] < 0:
        return empty, 0, cov
    queue = [int(t["child"][hit[0]])]
    out = {k: [] for k in _NODE + _EDGE}
    out["parent"].append(-1)
    out["parent_edge"].append(-1)
    nxt, dropped, h = 1, 0, 0
    while h < len(queue):
        old = queue[h]
        L, f = int(t["nchild"][old]), int(t["first"][old])
        out["nchild"].append(L)
        kept_here = dropped_here = 0
        for e in range(L):
            ch = int(t["child"][f + e])
            row = {k: t[k][f + e] for k in _EDGE}
            if ch >= 0:
                idx, nxt = nxt, nxt + 1
                if idx < keep_max:
                    queue.append(ch)
                    out["parent"].append(h)
                    out["parent_edge"].append(e)
                    row["child"] = idx
                    kept_here += 1
                    cov["far_edge"] |= e >= 64
                else:
                    row.update(n=0, w=np.float32(0), q=np.float32(0), child=CH_UNVISITED)
                    dropped_here += 1
            for k in _EDGE:
                out[k].append(row[k])
        dropped += dropped_here
        cov["row_cut"] |= kept_here > 0 and dropped_here > 0
        h += 1
    cov["rounds"] = len(queue) > 8
    return {k: np.array(out[k], t[k].dtype) for k in _NODE + _EDGE}, dropped, cov


def _same_bits(got, want, tag):
    for k in _NODE + _EDGE:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == b.dtype, "%s: %s" % (tag, k)
        if a.dtype.kind == "f":
            a, b = a.view("u%d" % a.itemsize), b.view("u%d" % b.itemsize)
        np.testing.assert_array_equal(a, b, err_msg="%s: %s" % (tag, k))


def _run_case(oracle, monkeypatch, board, keep_max):
    from alpha_omok_amd.engine import Engine
    monkeypatch.setenv("AO_COMPACT_ALWAYS", "1")
    eng = Engine(board, SIMS, 5, games=G, noise=True, node_cap=SIMS + 1 + keep_max)
    monkeypatch.delenv("AO_COMPACT_ALWAYS", raising=False)
    eng.seed_all(SEEDS)
    run = HostEvalRunner(eng)
    seen = dict(rounds=0, row_cut=0, far_edge=0, dropped=0, reroots=0)
    alive = np.ones(G, bool)
    for t in range(PLIES):
        run.move(lambda g, sim, pl: peaked_eval(oracle, pl), tau=np.zeros(G, np.int8), active=alive.astype(np.uint8))
        before = _games_of(eng.export_trees())
        trims0 = eng.trim_stats()
        act, win = eng.play()
        alive &= win == 0
        after = _games_of(eng.export_trees())
        dropped = trimmed = 0
        for g in np.flatnonzero(alive):
            want, d, cov = _expected(before[g], int(act[g]), keep_max)
            _same_bits(after[g], want, "board %d keep_max %d ply %d game %d" % (board, keep_max, t, g))
            dropped += d
            trimmed += d > 0
            seen["reroots"] += len(want["nchild"]) > 0
            for k in cov:
                seen[k] += bool(cov[k])
        trims1 = eng.trim_stats()
        assert (trims1[0] - trims0[0], trims1[1] - trims0[1]) == (dropped, trimmed), "board %d keep_max %d ply %d" % (board, keep_max, t)
        seen["dropped"] += dropped
        if not alive.any():
            break
    eng.close()
    _SEEN[(board, keep_max)] = seen
    return seen


@pytest.mark.parametrize("board,keep_max", PARAMS)
def test_trimmed_reroot_equals_the_host_walk(oracle, monkeypatch, board, keep_max):
    seen = _run_case(oracle, monkeypatch, board, keep_max)
    print("board %d keep_max %d: %s" % (board, keep_max, seen))
    assert seen["reroots"] > 0
    assert (seen["dropped"] > 0) == (keep_max != ROOMY)


def test_cases_cut_where_the_walk_can_go_wrong(oracle, monkeypatch):
    """The cases TOGETHER -- here held per board, which is more: a re-rooting that keeps more than 8 nodes (a second round of the
    eight waves), one that drops a child and keeps another child of the same node (the cut inside an edge row), and, where a
    node has more than 64 edges, one that keeps a child behind a stored edge index >= 64."""
    for p in PARAMS:
        if p not in _SEEN:            # (selected alone: run what the parametrised test would have run)
            _run_case(oracle, monkeypatch, *p)
    for b in BOARDS:
        total = {k: sum(_SEEN[(b, km)][k] for km in (1, CUT, ROOMY)) for k in ("rounds", "row_cut", "far_edge")}
        assert total["rounds"] > 0 and total["row_cut"] > 0, (b, total)
        assert total["far_edge"] > 0 or b * b <= 64, (b, total)
