"""Shared by test_gpu_tree_proofs.py and test_gpu_proof_moves.py: the roots and seeds whose stub-evaluator searches hold each class
of proof, and one cached search of every case per (tau, switch).

The roots and seeds were picked on the CPU with the oracle beforehand (oracle.Agent, evaluator 'stub0', noise on, the search of a
fresh agent on the root id; a recursive minimax over Agent.children): the class listed beside each game is what that run gave, and
the GPU tests assert it game by game -- these searches are bit-equal to the oracle's. Classes: WIN1 (the root's mover wins in one
ply), WIN3 (in three or more), LOSS2, LOSS4 (four or more), DRAW, UL (root unknown, at least one child proven lost), UN (root
unknown, no child proven lost). `*` marks a game whose tau == 0 pi sits on a proven-lost move (PM_MOVED)."""
import numpy as np

from gpu_helpers import HostEvalRunner

# (board, win_mark, simulations) -> [(root id, seed, class)]
CASES = {
    (3, 3, 300): [
        ((0, 5, 8, 0, 1, 6, 4), 0, "WIN1"), ((0, 8, 2, 3, 4, 5), 0, "WIN1"), ((0, 3, 7, 6, 4), 0, "WIN1"), ((0, 8, 4, 0, 7, 2, 6), 1, "WIN1"),
        ((0, 0, 1, 4, 8), 0, "WIN3"), ((0, 8, 1, 3, 7), 0, "WIN3"), ((0, 7, 2, 0, 4), 1, "WIN3"), ((0, 3, 8, 7), 0, "WIN3"),
        ((0, 6, 7, 3, 0, 5, 4), 0, "LOSS2"), ((0, 8, 6, 7, 1, 4, 0), 0, "LOSS2"), ((0, 2, 5, 8, 1, 6), 0, "LOSS2"),
        ((0, 7, 2, 5, 0), 0, "LOSS4"), ((0, 7, 2, 5, 0), 1, "LOSS4"), ((0, 1, 4, 7, 0), 0, "LOSS4"), ((0, 1, 4, 7, 0), 1, "LOSS4"),
        ((0, 7, 5, 8), 0, "LOSS4"), ((0, 7, 5, 8), 1, "LOSS4"),
        ((0, 5, 6, 0, 8, 2, 1), 0, "DRAW"), ((0, 5, 7, 1, 4, 0), 0, "DRAW*"), ((0, 5, 2, 6, 4, 8), 1, "DRAW*"), ((0, 7, 0, 3, 4), 0, "DRAW"),
        ((0, 4, 2, 5, 7, 6, 3), 0, "DRAW"),
        ((0, 0, 1, 4), 1, "UL*"), ((0, 4, 0, 8), 0, "UL*"), ((0, 4, 8, 2), 0, "UL*"), ((0, 6, 8, 0, 4, 5), 0, "UL*"), ((0, 2, 0, 3, 4), 0, "UL"),
        ((0, 4), 0, "UN"), ((0, 2, 4, 7), 0, "UN"), ((0, 5, 8, 1), 1, "UN"), ((0, 1, 2, 5), 0, "UN"),
    ],
    (4, 3, 300): [
        ((0, 5, 0, 6), 1, "LOSS2"), ((0, 7, 4, 6, 13, 3), 1, "LOSS2"),
        ((0, 10, 11, 6, 3), 0, "WIN1"), ((0, 13, 11, 15, 3, 4), 0, "WIN1"),
        ((0, 12, 13, 11, 10), 0, "WIN3"), ((0, 2, 13, 15, 8, 6), 0, "WIN3"), ((0, 15, 7, 2, 13), 0, "WIN3"),
        ((0, 5, 0, 6), 0, "UL*"), ((0, 6, 7, 11), 1, "UL*"), ((0, 4, 10, 14), 1, "UL*"), ((0, 12, 13, 11, 10), 1, "UL"),
        ((0, 5, 0), 0, "UN"), ((0, 5, 13), 1, "UN"),
    ],
    (5, 4, 1000): [
        ((0, 6, 0, 7, 1, 8), 0, "LOSS2"), ((0, 6, 0, 7, 1, 8), 1, "LOSS2"),
        ((0, 6, 0, 7, 1, 8, 2), 0, "WIN1"),
        ((0, 0, 23, 12, 3, 14, 19, 8, 22, 5, 6), 0, "WIN3"), ((0, 11, 6, 2, 21, 8, 14, 3, 15, 5, 13), 0, "WIN3"),
        ((0, 10, 2, 11, 22, 0, 7, 5), 0, "UL"), ((0, 12, 4, 2, 21, 7, 0, 8, 10, 24), 0, "UL*"),
        ((0, 12, 0, 11, 1), 0, "UN"), ((0, 1, 13, 10, 2, 22, 11), 0, "UN"),
    ],
}


def class_of(status, plies, child_status):
    """The class name (without `*`) of a root row of Engine.tree_proofs / utils.tree_proofs."""
    from alpha_omok_amd.utils import PROOF_DRAW, PROOF_LOSS, PROOF_WIN
    if status == PROOF_WIN:
        return "WIN1" if plies == 1 else "WIN3"
    if status == PROOF_LOSS:
        return "LOSS2" if plies == 2 else "LOSS4"
    if status == PROOF_DRAW:
        return "DRAW"
    return "UL" if (np.asarray(child_status) == PROOF_LOSS).any() else "UN"


def stream(eng, g):
    mt, pos, hg, gs = eng.get_rng_state(g)
    return mt.tobytes(), pos, hg, gs


_RUNS = {}


def searched(oracle, case, tau, on):
    """One search of every game of CASES[case] with Engine.set_proof_moves(on), stub0 through HostEvalRunner, then play(). Returns a
    dict: pi / visit / policy of end_move, the streams behind end_move and behind play, action / win; with the switch off also
    tree_proofs() and export_trees() of the searched trees, with it on proof_move_stats(per_game=True). Cached: a run is shared."""
    key = (case, tau, on)
    if key in _RUNS:
        return _RUNS[key]
    from alpha_omok_amd.engine import Engine
    board, wm, sims = case
    games = CASES[case]
    G = len(games)
    eng = Engine(board, sims, 5, games=G, noise=True, win_mark=wm)
    eng.seed_all([s for _, s, _ in games])
    eng.set_roots([r for r, _, _ in games])
    if on:
        eng.set_proof_moves(True)
    run = HostEvalRunner(eng)
    pi, vis, pol = run.move(lambda g, sim, planes: oracle.stub_eval(planes, 0), tau=np.full(G, tau, np.int8))
    out = dict(pi=pi, visit=vis, policy=pol, after_end=[stream(eng, g) for g in range(G)])
    if on:
        out["stats"] = eng.proof_move_stats(per_game=True)
    else:
        out["proofs"] = eng.tree_proofs()
        out["snapshot"] = eng.export_trees()
    out["action"], out["win"] = eng.play()
    out["after_play"] = [stream(eng, g) for g in range(G)]
    eng.close()
    _RUNS[key] = out
    return out


def assert_same_proofs(dev, g, ref, tag):
    """Row g of Engine.tree_proofs() against utils.tree_proofs of that game: root row, both [A] maps, line and length."""
    got = (int(dev["status"][g]), int(dev["plies"][g]), int(dev["proven"][g]), int(dev["walked"][g]))
    assert got == tuple(int(x) for x in ref["root"]), (tag, got, ref["root"])
    np.testing.assert_array_equal(dev["child_status"][g], ref["child_status"], err_msg=tag)
    np.testing.assert_array_equal(dev["child_plies"][g], ref["child_plies"], err_msg=tag)
    assert int(dev["len"][g]) == ref["len"], tag
    np.testing.assert_array_equal(dev["line"][g], ref["line"], err_msg=tag)


def assert_line_is_a_game(root_id, status, plies, line, board, wm, tag):
    """A proven WIN / LOSS root's line replayed with utils.check_win: no result before the last move, the last move wins for the
    side the status names, the length is `plies`."""
    from alpha_omok_amd import utils
    from alpha_omok_amd.utils import PROOF_WIN
    assert len(line) == plies, tag
    moves = list(root_id)[1:]
    mover = 1 + (len(moves) & 1)                      # check_win's index of the side to move at the root
    for k, a in enumerate(line):
        assert a not in moves, tag
        assert utils.check_win(utils.get_board([0] + moves, board), wm) == 0, (tag, k)
        moves.append(int(a))
    want = mover if status == PROOF_WIN else 3 - mover
    assert utils.check_win(utils.get_board([0] + moves, board), wm) == want, tag
    assert (plies % 2 == 1) == (status == PROOF_WIN), tag
