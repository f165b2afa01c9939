"""-m gpu: Engine.set_proof_moves -- end_move's pi follows what the root's tree proves (k_tree_proofs + k_proof_pi behind
k_end_move), exactly utils.proof_pi of the plain engine's pi, with visits, priors and streams untouched; and the edges of the
switch. Roots, seeds and classes: proof_cases.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import proof_cases as pc
from conftest import REPO
from gpu_helpers import HostEvalRunner

pytestmark = pytest.mark.gpu


# ---- 5. move choice ------------------------------------------------------------------------------------------------------------

def _compare(oracle, case, tau):
    """The games of one case, switch off against switch on. Returns the verdicts and whether pi changed, per game."""
    from alpha_omok_amd import utils
    off, on = pc.searched(oracle, case, tau, False), pc.searched(oracle, case, tau, True)
    games = pc.CASES[case]
    verdicts, changed = [], []
    assert np.array_equal(on["visit"], off["visit"]) and np.array_equal(on["policy"], off["policy"])
    assert on["after_end"] == off["after_end"] and on["after_play"] == off["after_play"]
    for g, (root, seed, cls) in enumerate(games):
        tag = "%r %r seed %d tau %d" % (case, root, seed, tau)
        want, v = utils.proof_pi(off["pi"][g], off["visit"][g], off["proofs"]["child_status"][g], off["proofs"]["child_plies"][g])
        assert on["pi"][g].tobytes() == np.asarray(want).tobytes(), tag
        assert int(on["stats"]["verdict"][g]) == v, tag
        if v == utils.PM_NONE:
            assert on["pi"][g].tobytes() == off["pi"][g].tobytes() and on["action"][g] == off["action"][g], tag
        if tau == 0:
            assert on["action"][g] == int(np.argmax(on["pi"][g])) and on["pi"][g].max() == 1.0, tag
        else:
            assert on["pi"][g][on["action"][g]] > 0, tag
        if v in (utils.PM_PRUNED, utils.PM_MOVED):                    # never a move that is proven lost while another is not
            assert off["proofs"]["child_status"][g][on["action"][g]] != utils.PROOF_LOSS, tag
        if v == utils.PM_WIN:                                         # ... and a proven win is played, the fastest one
            cs, cp = off["proofs"]["child_status"][g], off["proofs"]["child_plies"][g]
            assert cs[on["action"][g]] == utils.PROOF_WIN and cp[on["action"][g]] == cp[cs == utils.PROOF_WIN].min(), tag
        verdicts.append(v)
        changed.append(on["pi"][g].tobytes() != off["pi"][g].tobytes())
    st = on["stats"]
    assert [st["none"], st["win"], st["pruned"], st["moved"]] == [verdicts.count(k) for k in range(4)]
    return verdicts, changed


@pytest.mark.parametrize("tau", [1, 0])
def test_pi_is_proof_pi_of_the_plain_pi(oracle, tau):
    """Per game: pi_on == utils.proof_pi(pi_off, visit, the root's edge values)[0] bit for bit, the verdicts match, visit and
    policy are equal, the streams behind end_move and behind play are equal, and under tau == 0 the action played is the argmax
    of pi_on. Coverage, asserted: under tau == 1 at least 3 games with PM_WIN whose pi changed and 3 with PM_PRUNED; under
    tau == 0 at least 3 with PM_MOVED."""
    from alpha_omok_amd import utils
    verdicts, changed = [], []
    for case in sorted(pc.CASES):
        v, c = _compare(oracle, case, tau)
        verdicts += v
        changed += c
    print("tau", tau, "verdicts none/win/pruned/moved", [verdicts.count(k) for k in range(4)], "pi changed", sum(changed))
    if tau == 1:
        assert sum(1 for v, c in zip(verdicts, changed) if v == utils.PM_WIN and c) >= 3
        assert verdicts.count(utils.PM_PRUNED) >= 3
    else:
        assert verdicts.count(utils.PM_MOVED) >= 3
        stars = [cls.endswith("*") for case in sorted(pc.CASES) for _, _, cls in pc.CASES[case]]
        assert [v == utils.PM_MOVED for v in verdicts] == stars


# ---- 6. edges of the switch --------------------------------------------------------------------------------------------------

def test_inactive_games_keep_their_rows_and_the_counters_sum_to_the_moves(oracle):
    from alpha_omok_amd.engine import Engine
    case = (3, 3, 300)
    games = pc.CASES[case][:12]
    G = len(games)
    eng = Engine(3, 60, 5, games=G, noise=True, win_mark=3)
    eng.seed_all([s for _, s, _ in games])
    eng.set_roots([r for r, _, _ in games])
    eng.set_proof_moves(True)
    run = HostEvalRunner(eng)
    ev = lambda g, sim, planes: oracle.stub_eval(planes, 0)                             # noqa: E731
    assert eng.proof_move_stats(per_game=True)["verdict"].tolist() == [0] * G
    pi1, _, _ = run.move(ev, tau=np.ones(G, np.int8))
    first = eng.proof_move_stats(per_game=True)
    assert first["none"] + first["win"] + first["pruned"] + first["moved"] == G
    assert first["win"] >= 1                                                            # (the WIN1 roots need no search to speak of)
    act, win = eng.play()
    active = ((win == 0) & (np.arange(G) % 2 == 0)).astype(np.uint8)
    assert active.any() and not active.all()
    pi2, _, _ = run.move(ev, tau=np.zeros(G, np.int8), active=active)
    second = eng.proof_move_stats(per_game=True)
    idle = active == 0
    assert np.array_equal(pi2[idle], pi1[idle])                                         # the rows of the move before, untouched
    assert np.array_equal(second["verdict"][idle], first["verdict"][idle])
    assert sum(second[k] for k in ("none", "win", "pruned", "moved")) == G + int(active.sum())
    assert eng.proof_move_stats(reset=True)["win"] == second["win"] and sum(v for k, v in eng.proof_move_stats().items()) == 0
    # off again: the next move is a plain one, and nothing is counted
    eng.play()
    eng.set_proof_moves(False)
    eng.close()


def test_switch_is_refused_inside_a_move_and_refuses_a_roll():
    import pvnet_weights
    from alpha_omok_amd.engine import Engine, EngineError, Net
    B = 5
    eng = Engine(B, 8, 5, games=2, noise=True)
    net = Net(1, 5, 32, B, 0)
    net.load_state_dict(pvnet_weights.make_state_dict(1, 5, 32, B, 3))
    eng.begin_move()
    with pytest.raises(EngineError, match="inside a move"):
        eng.set_proof_moves(True)
    with pytest.raises(EngineError, match="inside a move"):
        eng.tree_proofs()
    eng.reset()
    eng.set_proof_moves(True)
    with pytest.raises(EngineError, match="ao_set_proof_moves"):
        eng.roll_begin(net)
    eng.set_proof_moves(False)
    eng.roll_begin(net)                                      # off: the roll opens, and the read-out is refused while it is open
    with pytest.raises(EngineError, match="a roll is open"):
        eng.tree_proofs()
    with pytest.raises(EngineError, match="a roll is open"):
        eng.set_proof_moves(True)
    eng.roll_drain()
    while len(eng.roll_run()["game"]):
        pass
    eng.roll_end()
    with pytest.raises(EngineError, match="max_len"):
        eng.tree_proofs(max_len=0)
    eng.close()
    net.close()


_GUARDED = r"""
import json, sys
import numpy as np
sys.path.insert(0, "tests")
import pvnet_weights
from alpha_omok_amd.engine import Engine, Net, guard_check, guard_mode
B, G = 5, 8
net = Net(1, 5, 32, B, 0)
net.load_state_dict(pvnet_weights.make_state_dict(1, 5, 32, B, 3))
eng = Engine(B, 40, 5, games=G, noise=True, win_mark=4)
eng.seed_all(list(range(G)))
eng.set_roots([(0, 6, 0, 7, 1, 8, 2)] * 4 + [(0, 6, 0, 7, 1, 8)] * 4)
eng.search(net, tau=np.ones(G, np.int8))
before = guard_check()
pr = eng.tree_proofs()
eng.set_proof_moves(True)
act, win = eng.play()
alive = (win == 0).astype(np.uint8)
for ply in range(2):
    if not alive.any():
        break
    pi, vis, pol = eng.search(net, tau=np.zeros(G, np.int8), active=alive)
    act, win = eng.play()
    alive &= (win == 0).astype(np.uint8)
stats = eng.proof_move_stats()
after = guard_check()
eng.close()
net.close()
print(json.dumps(dict(mode=list(guard_mode()), before=list(before), after=list(after), freed=list(guard_check()),
                      walked=pr["walked"].tolist(), stats=stats)))
"""


def test_guarded_allocations_see_no_stray_write():
    """A child process with AO_POOL_GUARD set: the workspace of the proofs is allocated under guards (more blocks after the first
    call than before), and neither tree_proofs nor two proof-move searches damage a guard."""
    env = dict(os.environ, AO_POOL_GUARD="65536", AO_POOL_FILL="90")
    r = subprocess.run([sys.executable, "-c", _GUARDED], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out)
    assert out["mode"] == [65536, 90]
    assert out["before"][0] > 0 and out["before"][1] == 0
    assert out["after"][0] >= out["before"][0] + 5, "the proofs' buffers did not go through the guarded allocator"
    assert out["after"][1] == 0, out["after"][2]
    assert out["freed"][1] == 0, out["freed"][2]
    assert min(out["walked"]) > 0 and sum(out["stats"].values()) > 0


def test_evaluate_batched_with_proof_moves_completes():
    import torch
    import pvnet_weights
    from alpha_omok_amd import evaluate
    from alpha_omok_amd.pvnet import PVNet
    B = 5
    nets = []
    for seed in (1, 2):
        m = PVNet(1, 5, 32, B)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in pvnet_weights.make_state_dict(1, 5, 32, B, seed).items()})
        nets.append(m.cuda().eval())
    result, elos, games = evaluate.evaluate_batched(nets[0], nets[1], B, 30, n_match=8, seed=3, proof_moves=True)
    assert sum(result.values()) == 8 and len(games) == 8
    pm = evaluate.last_proof_moves
    assert sorted(pm) == [0, 1]
    moves = sum(len(mv) for _, mv in games)
    assert sum(sum(pm[k].values()) for k in pm) == moves              # one verdict per move played, over both sides
    plain, _, _ = evaluate.evaluate_batched(nets[0], nets[1], B, 30, n_match=8, seed=3, proof_moves=(True, False))
    assert sum(plain.values()) == 8 and sorted(evaluate.last_proof_moves) == [0]
    with pytest.raises(ValueError):
        evaluate.evaluate_batched(nets[0], nets[1], B, 30, n_match=2, proof_moves=(True,))


def test_agent_and_configure(oracle):
    """ZeroAgent(proof_moves=True).get_pi plays the proven win and get_proof tells it; main.configure refuses the switch with
    rolling=True and hands it to the self-play engine otherwise."""
    import torch
    import pvnet_weights
    import alpha_omok_amd.main as m
    from alpha_omok_amd import agents, utils
    from alpha_omok_amd.pvnet import PVNet
    B = 9
    model = PVNet(1, 5, 32, B)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in pvnet_weights.make_state_dict(1, 5, 32, B, 4).items()})
    model = model.cuda().eval()
    ag = agents.ZeroAgent(B, 200, 5, noise=False, proof_moves=True)
    ag.model = model
    assert ag.get_proof()["status"] == utils.PROOF_UNKNOWN
    root = (0, 38, 0, 39, 2, 40, 8, 41, 19)                  # black to move with an open four on 38..41
    np.random.seed(5)
    pi = ag.get_pi(root, 1)
    pr = ag.get_proof(root)
    assert (pr["status"], pr["plies"]) == (utils.PROOF_WIN, 1) and ag.last_proof_verdict == utils.PM_WIN
    assert pi.max() == 1.0 and int(np.argmax(pi)) in (37, 42) and list(pr["line"]) == [int(np.argmax(pi))]
    assert pr["cells"].shape == (B, B) and pr["cells"][4, 1] == utils.PROOF_WIN and pr["cells"][4, 2] == -1
    with pytest.raises(ValueError):
        ag.get_proof((0, 1))
    with pytest.raises(ValueError, match="rolling"):
        m.configure(board_size=B, n_mcts=20, n_blocks=1, out_planes=32, rolling=True, proof_moves=True)
    m.configure(board_size=B, n_mcts=20, n_blocks=1, out_planes=32, proof_moves=True)
    assert m.PROOF_MOVES is True and m.Agent.proof_moves is True
    m.configure(board_size=B, n_mcts=20, n_blocks=1, out_planes=32)
    assert m.PROOF_MOVES is False
