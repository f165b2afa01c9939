"""CPU: the definitions of proven outcomes -- utils.tree_proofs on hand-built TreeSnapshot arrays against an independent
brute-force negamax over the full 3x3 game, and utils.proof_pi case by case. (That the header, _lib.SYMBOLS and the library
agree on ao_tree_proofs / ao_set_proof_moves / ao_proof_move_records is test_abi.py's check.)"""
import functools

import numpy as np
import pytest

from alpha_omok_amd import utils
from alpha_omok_amd.snapshot import TreeSnapshot
from alpha_omok_amd.utils import (PM_MOVED, PM_NONE, PM_PRUNED, PM_WIN, PROOF_DRAW, PROOF_LOSS, PROOF_UNKNOWN, PROOF_WIN)

B, WM = 3, 3
LINES = [(0, 1, 2), (3, 4, 5), (6, 7, 8), (0, 3, 6), (1, 4, 7), (2, 5, 8), (0, 4, 8), (2, 4, 6)]


def result_of(moves):
    """0 playing / 1 black / 2 white / 3 draw, from the eight lines of the 3x3 board (not utils.check_win)."""
    for side in (0, 1):
        mine = set(moves[side::2])
        if any(all(c in mine for c in ln) for ln in LINES):
            return side + 1
    return 3 if len(moves) == 9 else 0


def build_snapshot(root_moves, visited=lambda moves: True):
    """A TreeSnapshot of one 3x3 game: breadth first from the root, children in utils.legal_actions order; a child that ends the
    game is CH_TERMINAL, one with visited(moves) is expanded, any other CH_UNVISITED."""
    nodes = [list(root_moves)]
    nchild, parent, parent_edge, act, child = [], [-1], [-1], [], []
    j = 0
    while j < len(nodes):
        mv = nodes[j]
        legal = utils.legal_actions([0] + mv, B)
        nchild.append(len(legal))
        for k, a in enumerate(legal):
            nm = mv + [a]
            act.append(a)
            if result_of(nm):
                child.append(-2)
            elif visited(tuple(nm)):
                child.append(len(nodes))
                nodes.append(nm)
                parent.append(j)
                parent_edge.append(k)
            else:
                child.append(-1)
        j += 1
    N, E = len(nodes), len(act)
    hdr = np.array([[N, E, len(root_moves), 2, 0, 624, 0, 0]], np.int32)
    mv = np.zeros((1, B * B), np.int32)
    mv[0, :len(root_moves)] = root_moves
    snap = TreeSnapshot(B, 5, WM, hdr=hdr, gauss=np.zeros(1), mt=np.zeros((1, 624), np.uint32), moves=mv, nchild=nchild, parent=parent,
                        parent_edge=parent_edge, act=np.array(act, np.uint8), n=(np.array(child + [0])[:E] != -1).astype(np.int32), w=np.zeros(E, np.float32),
                        q=np.zeros(E, np.float32), p=np.zeros(E), child=child)
    return snap, [tuple(m) for m in nodes]


def negamax(visited):
    """(status, plies) of the side to move after `moves`, over the game itself with the tree's horizon `visited`."""
    @functools.lru_cache(maxsize=None)
    def f(moves):
        vals = []
        for a in range(9):
            if a in moves:
                continue
            nm = moves + (a,)
            r = result_of(nm)
            if r == 3:
                vals.append((PROOF_DRAW, 1))
            elif r:
                vals.append((PROOF_WIN, 1))          # only the side that placed the stone can have completed a line
            elif not visited(nm):
                vals.append((PROOF_UNKNOWN, 0))
            else:
                st, pl = f(nm)
                vals.append(({PROOF_WIN: PROOF_LOSS, PROOF_LOSS: PROOF_WIN}.get(st, st), pl + 1 if st else 0))
        wins = [p for s, p in vals if s == PROOF_WIN]
        if wins:
            return PROOF_WIN, min(wins)
        if any(s == PROOF_UNKNOWN for s, _ in vals):
            return PROOF_UNKNOWN, 0
        draws = [p for s, p in vals if s == PROOF_DRAW]
        if draws:
            return PROOF_DRAW, min(draws)
        return PROOF_LOSS, max(p for _, p in vals)
    return f


def check_against_negamax(root_moves, visited):
    snap, nodes = build_snapshot(root_moves, visited)
    snap.check()
    out = utils.tree_proofs(snap, 0)
    f = negamax(visited)
    for j, mv in enumerate(nodes):
        assert (int(out["status"][j]), int(out["plies"][j])) == f(mv), (j, mv)
    assert tuple(out["root"]) == (f(nodes[0])[0], f(nodes[0])[1], int(np.count_nonzero(out["status"])), len(nodes))
    return snap, nodes, out


@pytest.mark.parametrize("root", [(0, 4, 8, 2), (4, 0, 8, 2), (0, 1, 4, 8), (0, 4, 1, 2), (4, 1, 0, 8), (0, 1, 3, 6, 4), (0, 4)])
def test_complete_tree_equals_negamax(root):
    """A complete game tree below the root: every node's status and plies are the game's own."""
    snap, nodes, out = check_against_negamax(list(root), lambda m: True)
    assert out["root"][0] != PROOF_UNKNOWN and out["root"][2] == len(nodes)
    # the line: as long as the root's plies, legal, ends the game for the side the status names, no result before its end
    ln = [int(a) for a in out["line"][:out["len"]]]
    assert out["len"] == out["root"][1] and (out["line"][out["len"]:] == -1).all()
    mv = list(root)
    for i, a in enumerate(ln):
        assert a not in mv and result_of(mv) == 0
        mv.append(a)
    r = result_of(mv)
    mover = 1 + (len(root) & 1)
    want = {PROOF_WIN: mover, PROOF_LOSS: 3 - mover, PROOF_DRAW: 3}[int(out["root"][0])]
    assert r == want
    # the root's edges by action
    f = negamax(lambda m: True)
    for a in range(9):
        if a in root:
            assert out["child_status"][a] == -1 and out["child_plies"][a] == 0
            continue
        nm = tuple(root) + (a,)
        if result_of(nm):
            want = (PROOF_DRAW if result_of(nm) == 3 else PROOF_WIN, 1)
        else:
            st, pl = f(nm)
            want = ({PROOF_WIN: PROOF_LOSS, PROOF_LOSS: PROOF_WIN}.get(st, st), pl + 1)
        assert (int(out["child_status"][a]), int(out["child_plies"][a])) == want


def test_known_classes():
    """The classes the searches of the GPU tests are picked for, on complete trees: ids of the issue's CPU runs."""
    assert tuple(check_against_negamax([0, 1, 4, 8], lambda m: True)[2]["root"][:2]) == (PROOF_WIN, 3)
    assert tuple(check_against_negamax([0, 1, 4], lambda m: True)[2]["root"][:2]) == (PROOF_LOSS, 4)
    assert check_against_negamax([5, 6, 0, 8, 2, 1], lambda m: True)[2]["root"][0] == PROOF_DRAW


def test_incomplete_tree_unknown_where_an_unvisited_edge_blocks():
    root = [0, 1, 2, 4]                                      # X to move must block at 7, every reply of O then draws
    full = check_against_negamax(root, lambda m: True)[2]
    assert full["root"][0] == PROOF_DRAW
    # one unvisited grandchild below the only non-losing move: the root's proof is gone, the refutations of the other moves stay
    hole = (0, 1, 2, 4, 7, 3)
    snap, nodes, out = check_against_negamax(root, lambda m: m != hole)
    assert out["root"][0] == PROOF_UNKNOWN and out["len"] == 0 and (out["line"] == -1).all()
    assert out["child_status"][7] == PROOF_UNKNOWN and out["child_plies"][7] == 0
    lost = [a for a in range(9) if out["child_status"][a] == PROOF_LOSS]
    assert lost == [a for a in range(9) if full["child_status"][a] == PROOF_LOSS] and lost
    unknown = {nodes[j] for j in range(len(nodes)) if out["status"][j] == PROOF_UNKNOWN}
    assert unknown == {(0, 1, 2, 4), (0, 1, 2, 4, 7)}        # exactly the ancestors whose value hung on the hole
    # a WIN needs one edge only: an unvisited sibling does not block it
    snap, nodes, out = check_against_negamax([0, 1, 4, 8], lambda m: m[:5] not in {(0, 1, 4, 8, 2), (0, 1, 4, 8, 5)})
    assert tuple(out["root"][:2]) == (PROOF_WIN, 3)
    # nothing expanded below the root: unknown, unless a terminal edge decides
    assert check_against_negamax([0, 1], lambda m: False)[2]["root"][0] == PROOF_UNKNOWN
    assert tuple(check_against_negamax([0, 3, 1, 4], lambda m: False)[2]["root"][:2]) == (PROOF_WIN, 1)


def test_draw_edge_is_not_a_win_edge():
    snap, nodes, out = check_against_negamax([0, 1, 2, 4, 3, 5, 7, 6], lambda m: True)    # the last stone fills the board, no line
    assert tuple(out["root"][:2]) == (PROOF_DRAW, 1) and out["child_status"][8] == PROOF_DRAW and list(out["line"][:1]) == [8]
    snap, nodes, out = check_against_negamax([0, 2, 4, 3, 1, 6, 5, 7], lambda m: True)    # the last stone fills the board AND a line
    assert tuple(out["root"][:2]) == (PROOF_WIN, 1) and out["child_status"][8] == PROOF_WIN
    # one ply up, white to move: 6 draws two plies on, 8 loses to black's 6 -- a draw, with the DRAW edge's plies, not the lost one's
    snap, nodes, out = check_against_negamax([0, 1, 2, 4, 3, 5, 7], lambda m: True)
    assert tuple(out["root"][:2]) == (PROOF_DRAW, 2)
    assert (out["child_status"][6], out["child_plies"][6]) == (PROOF_DRAW, 2)
    assert (out["child_status"][8], out["child_plies"][8]) == (PROOF_LOSS, 2)


def test_game_index_and_empty_game():
    """Two games in one snapshot, the second without a tree: game 1 is all defaults, game 0 is untouched by its neighbour."""
    a, _ = build_snapshot([0, 1, 4, 8])
    arrays = {k: getattr(a, k) for k in ("nchild", "parent", "parent_edge", "act", "n", "w", "q", "p", "child")}
    hdr = np.concatenate([a.hdr, np.array([[0, 0, 2, 1, 0, 624, 0, 0]], np.int32)])
    mv = np.concatenate([a.moves, np.array([[3, 5, 0, 0, 0, 0, 0, 0, 0]], np.int32)])
    two = TreeSnapshot(B, 5, WM, hdr=hdr, gauss=np.zeros(2), mt=np.zeros((2, 624), np.uint32), moves=mv, **arrays)
    one, empty = utils.tree_proofs(two, 0), utils.tree_proofs(two, 1, max_len=4)
    assert tuple(one["root"][:2]) == (PROOF_WIN, 3)
    assert tuple(empty["root"]) == (0, 0, 0, 0) and (empty["child_status"] == -1).all() and (empty["child_plies"] == 0).all()
    assert empty["len"] == 0 and list(empty["line"]) == [-1] * 4
    assert list(utils.tree_proofs(two, 0, max_len=2)["line"]) == list(one["line"][:2])


# ---- proof_pi ----

def _row(**kw):
    A = 9
    st, pl = np.full(A, -1, np.int8), np.zeros(A, np.int16)
    for a, (s, p) in kw.get("edges", {}).items():
        st[a], pl[a] = s, p
    return st, pl


def test_proof_pi_win_and_its_ties():
    pi = np.array([0.5, 0.25, 0.25, 0, 0, 0, 0, 0, 0])
    vis = np.array([4., 2, 2, 0, 0, 0, 0, 0, 0])
    # the fewest plies beat visits
    st, pl = _row(edges={0: (PROOF_WIN, 3), 1: (PROOF_UNKNOWN, 0), 2: (PROOF_WIN, 1), 3: (PROOF_LOSS, 2)})
    out, v = utils.proof_pi(pi, vis, st, pl)
    assert v == PM_WIN and list(out) == [0, 0, 1, 0, 0, 0, 0, 0, 0]
    # equal plies: the larger visit
    st, pl = _row(edges={0: (PROOF_WIN, 3), 1: (PROOF_WIN, 3), 2: (PROOF_WIN, 5)})
    out, v = utils.proof_pi(pi, vis, st, pl)
    assert v == PM_WIN and int(np.argmax(out)) == 0 and out.sum() == 1.0
    # equal plies and visits: the lowest action
    st, pl = _row(edges={1: (PROOF_WIN, 3), 2: (PROOF_WIN, 3), 5: (PROOF_WIN, 3)})
    out, v = utils.proof_pi(pi, vis, st, pl)
    assert v == PM_WIN and int(np.argmax(out)) == 1
    # the verdict is PM_WIN also where pi already sat there
    onehot = np.eye(9)[1]
    out, v = utils.proof_pi(onehot, vis, st, pl)
    assert v == PM_WIN and np.array_equal(out, onehot)


def test_proof_pi_pruned_is_the_sequential_sum():
    pi = np.array([0.1, 0.2, 0.3, 0.05, 0.15, 0.2, 0, 0, 0])
    vis = pi * 20
    st, pl = _row(edges={0: (PROOF_UNKNOWN, 0), 1: (PROOF_LOSS, 2), 2: (PROOF_DRAW, 3), 3: (PROOF_UNKNOWN, 0), 4: (PROOF_LOSS, 4),
                         5: (PROOF_UNKNOWN, 0), 6: (PROOF_UNKNOWN, 0)})
    out, v = utils.proof_pi(pi, vis, st, pl)
    s = ((0.1 + 0.3) + 0.05) + 0.2 + 0.0                     # ascending action order, one addition at a time
    assert v == PM_PRUNED
    want = np.array([0.1 / s, 0.0, 0.3 / s, 0.05 / s, 0.0, 0.2 / s, 0.0, 0.0, 0.0])
    assert out.tobytes() == want.tobytes()
    # an order that rounds differently gives another divisor: the definition is the ascending one
    big = np.array([1e-17, 1.0, 1e-17, 1e-17, 0.5, 0, 0, 0, 0])
    st, pl = _row(edges={0: (PROOF_UNKNOWN, 0), 1: (PROOF_UNKNOWN, 0), 2: (PROOF_UNKNOWN, 0), 3: (PROOF_UNKNOWN, 0), 4: (PROOF_LOSS, 2)})
    out, v = utils.proof_pi(big, big, st, pl)
    s = ((1e-17 + 1.0) + 1e-17) + 1e-17
    assert v == PM_PRUNED and out[1] == 1.0 / s and out[0] == 1e-17 / s and out[4] == 0.0


def test_proof_pi_moved_when_nothing_is_left():
    vis = np.array([9., 3, 5, 5, 0, 0, 0, 0, 0])
    onehot = np.eye(9)[0]                                    # tau == 0 on a lost move
    st, pl = _row(edges={0: (PROOF_LOSS, 2), 1: (PROOF_UNKNOWN, 0), 2: (PROOF_DRAW, 5), 3: (PROOF_UNKNOWN, 0), 4: (PROOF_LOSS, 2)})
    out, v = utils.proof_pi(onehot, vis, st, pl)
    assert v == PM_MOVED and list(out) == [0, 0, 1, 0, 0, 0, 0, 0, 0]      # most visits among the kept, lowest action on the tie


def test_proof_pi_no_op_cases_return_the_input():
    pi = np.array([0.5, 0.25, 0.25, 0, 0, 0, 0, 0, 0])
    vis = pi * 8
    cases = {
        "nothing proven": {0: (PROOF_UNKNOWN, 0), 1: (PROOF_UNKNOWN, 0), 2: (PROOF_DRAW, 3)},
        "root proven LOSS": {0: (PROOF_LOSS, 2), 1: (PROOF_LOSS, 4), 2: (PROOF_LOSS, 2), 3: (PROOF_LOSS, 2)},
        "no lost edge carries pi": {0: (PROOF_UNKNOWN, 0), 1: (PROOF_UNKNOWN, 0), 2: (PROOF_UNKNOWN, 0), 3: (PROOF_LOSS, 2)},
        "no edges": {},
    }
    for name, edges in cases.items():
        st, pl = _row(edges=edges)
        out, v = utils.proof_pi(pi, vis, st, pl)
        assert v == PM_NONE and out is pi, name
    nan = np.full(9, np.nan)
    st, pl = _row(edges={0: (PROOF_UNKNOWN, 0), 1: (PROOF_LOSS, 2)})
    out, v = utils.proof_pi(nan, vis, st, pl)
    assert v == PM_NONE and out is nan


def test_constants_are_exported_from_engine():
    from alpha_omok_amd import engine
    assert (engine.PROOF_UNKNOWN, engine.PROOF_WIN, engine.PROOF_LOSS, engine.PROOF_DRAW) == (0, 1, 2, 3)
    assert (engine.PM_NONE, engine.PM_WIN, engine.PM_PRUNED, engine.PM_MOVED) == (0, 1, 2, 3)
