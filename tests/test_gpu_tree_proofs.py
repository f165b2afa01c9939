"""-m gpu: Engine.tree_proofs (k_tree_proofs) against its definition, utils.tree_proofs of the exported trees, exactly: root row,
both [A] maps, line and length; the classes the games were picked for; the proof lines replayed as real games; and that the
read-out writes nothing a later search could see. Roots, seeds and classes: proof_cases.py."""
import numpy as np
import pytest

import proof_cases as pc
from gpu_helpers import HostEvalRunner

pytestmark = pytest.mark.gpu


def _every_game_equals_definition(dev, snap, G, tag):
    from alpha_omok_amd import utils
    refs = []
    for g in range(G):
        ref = utils.tree_proofs(snap, g)
        pc.assert_same_proofs(dev, g, ref, "%s game %d" % (tag, g))
        refs.append(ref)
    return refs


# ---- 1. device equals definition, on small boards where every class is reached -----------------------------------------------

@pytest.mark.parametrize("case", sorted(pc.CASES))
def test_device_equals_definition(oracle, case):
    r = pc.searched(oracle, case, 1, False)
    games = pc.CASES[case]
    dev = r["proofs"]
    _every_game_equals_definition(dev, r["snapshot"], len(games), str(case))
    for g, (root, seed, cls) in enumerate(games):
        got = pc.class_of(dev["status"][g], dev["plies"][g], dev["child_status"][g])
        print(case, root, seed, cls, "->", got, int(dev["plies"][g]), int(dev["proven"][g]), int(dev["walked"][g]))
        assert got == cls.rstrip("*"), (case, root, seed)


def test_cases_cover_every_class(oracle):
    """Over the games of test 1: at least 4 roots each that are WIN in 1, WIN in >= 3, LOSS in 2, LOSS in >= 4, DRAW, unknown with a
    lost child, unknown without one -- counted from what the DEVICE returned."""
    count = {}
    for case in pc.CASES:
        dev = pc.searched(oracle, case, 1, False)["proofs"]
        for g in range(len(pc.CASES[case])):
            c = pc.class_of(dev["status"][g], dev["plies"][g], dev["child_status"][g])
            count[c] = count.get(c, 0) + 1
    print(count)
    for c in ("WIN1", "WIN3", "LOSS2", "LOSS4", "DRAW", "UL", "UN"):
        assert count.get(c, 0) >= 4, (c, count)


# ---- 2. wide boards: NCH 2 and 4, a network's trees ----------------------------------------------------------------------------

def _wide_roots(B):
    """Constructed roots on a B x B board, win_mark 5; r = the middle row. Each is searched under four seeds."""
    r = (B // 2) * B
    far = [0, 2, B - 1, 2 * B + 1, 4]                       # scattered stones of the other side: no line of theirs
    four = [r + 2, r + 3, r + 4, r + 5]
    mine = (0,) + tuple(x for k in range(4) for x in (four[k], far[k]))                  # black to move with an open four
    theirs = mine + (far[4],)                                                            # one stone more: white faces the four
    quiet = (0, r + 4)
    return [("mover has an open four", mine), ("the opponent has a four", theirs), ("quiet", quiet), ("not expanded", (0, 1))]


@pytest.mark.parametrize("B", [9, 15])
def test_wide_boards(B):
    import pvnet_weights
    from alpha_omok_amd.engine import Engine, Net
    from alpha_omok_amd.utils import PROOF_LOSS, PROOF_WIN
    S, per = 200, 4
    roots = _wide_roots(B)
    ids = [rid for _, rid in roots for _ in range(per)]
    G = len(ids)
    net = Net(1, 5, 32, B, 0)
    net.load_state_dict(pvnet_weights.make_state_dict(1, 5, 32, B, 5))
    eng = Engine(B, S, 5, games=G, noise=True)
    eng.seed_all([100 + g for g in range(G)])
    eng.set_roots(ids)
    active = np.array([0 if name == "not expanded" else 1 for name, _ in roots for _ in range(per)], np.uint8)
    eng.search(net, tau=np.ones(G, np.int8), active=active)
    dev = eng.tree_proofs()
    snap = eng.export_trees()
    refs = _every_game_equals_definition(dev, snap, G, "board %d" % B)
    seen = dict(win1=0, lost_child=0, lines=0)
    for g in range(G):
        name = roots[g // per][0]
        st, pl = int(dev["status"][g]), int(dev["plies"][g])
        print(B, name, "status", st, "plies", pl, "lost children", int((dev["child_status"][g] == PROOF_LOSS).sum()),
              "proven", int(dev["proven"][g]), "walked", int(dev["walked"][g]))
        if name == "not expanded":
            assert (st, pl, int(dev["proven"][g]), int(dev["walked"][g]), int(dev["len"][g])) == (0, 0, 0, 0, 0)
            assert (dev["child_status"][g] == -1).all() and (dev["line"][g] == -1).all()
            continue
        assert int(dev["walked"][g]) > 1 and (dev["child_status"][g][list(ids[g][1:])] == -1).all()
        seen["win1"] += (st, pl) == (PROOF_WIN, 1)
        seen["lost_child"] += bool((dev["child_status"][g] == PROOF_LOSS).any())
        if st in (PROOF_WIN, PROOF_LOSS):                                                # 3. the line is a real game
            pc.assert_line_is_a_game(ids[g], st, pl, dev["line"][g, :dev["len"][g]].tolist(), B, 5, "board %d game %d" % (B, g))
            seen["lines"] += 1
    # a cut line is the head of the full one, and unmasked games keep the caller's rows
    mask = np.arange(G) % 2 == 0
    cut = eng.tree_proofs(mask=mask, max_len=1)
    for g in range(G):
        if mask[g]:
            assert cut["len"][g] == min(1, dev["len"][g]) and cut["line"][g, 0] == dev["line"][g, 0]
            assert cut["status"][g] == dev["status"][g] and np.array_equal(cut["child_plies"][g], dev["child_plies"][g])
        else:
            assert cut["status"][g] == -1 and cut["walked"][g] == -1 and (cut["child_status"][g] == -1).all() and cut["len"][g] == 0
    eng.close()
    net.close()
    assert seen["win1"] >= 1 and seen["lost_child"] >= 1, seen


# ---- 3. the line is a real game ------------------------------------------------------------------------------------------------

def test_every_proof_line_is_a_real_game(oracle):
    from alpha_omok_amd.utils import PROOF_LOSS, PROOF_WIN
    n = 0
    for case in pc.CASES:
        board, wm, _ = case
        dev = pc.searched(oracle, case, 1, False)["proofs"]
        for g, (root, seed, cls) in enumerate(pc.CASES[case]):
            st = int(dev["status"][g])
            if st in (PROOF_WIN, PROOF_LOSS):
                pc.assert_line_is_a_game(root, st, int(dev["plies"][g]), dev["line"][g, :dev["len"][g]].tolist(), board, wm,
                                         "%r %r seed %d" % (case, root, seed))
                n += 1
    assert n >= 16


# ---- 4. read-only ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,S,node_cap", [(3, 50, 0), (3, 50, 15000), (9, 60, 0)])
def test_read_only(oracle, B, S, node_cap):
    """Two identically seeded engines; one reads its proofs between the moves. Visits, pi, policy, actions and the streams (624
    words and the position) are equal over three moves. node_cap 15000 is the largest ao_create accepts: the largest workspace
    row and the largest queue in the LDS."""
    from alpha_omok_amd.engine import Engine
    G = 4
    engs = [Engine(B, S, 5, games=G, noise=True, node_cap=node_cap) for _ in range(2)]
    if node_cap:
        assert engs[0].node_cap()[0] == node_cap
    runs = [HostEvalRunner(e) for e in engs]
    for e in engs:
        e.seed_all([7 + g for g in range(G)])
    alive = np.ones(G, np.uint8)
    for ply in range(3):
        outs = []
        for k, (e, run) in enumerate(zip(engs, runs)):
            if k == 1:
                before = e.tree_proofs()
                assert (before["walked"][alive == 1] > 0).all() if ply else not before["walked"].any()
            pi, vis, pol = run.move(lambda g, sim, planes: oracle.stub_eval(planes, 0), tau=np.full(G, 1 if ply < 2 else 0, np.int8),
                                    active=alive)
            if k == 1:
                e.tree_proofs()
                e.tree_proofs(max_len=2)
            act, win = e.play()
            outs.append((pi, vis, pol, act, win, [pc.stream(e, g) for g in range(G)]))
        for a, b in zip(outs[0][:5], outs[1][:5]):
            assert np.array_equal(a[alive == 1], b[alive == 1]), ply
        assert outs[0][5] == outs[1][5], ply
        alive &= (outs[0][4] == 0).astype(np.uint8)
        if not alive.any():
            break
    for e in engs:
        e.close()
