#!/usr/bin/env python
"""Measures proven outcomes (Engine.tree_proofs: exact minimax over the trees) and proof moves (Engine.set_proof_moves).

    python tools/time_proof_moves.py --leg cost --json a.json       4096 games, 9x9, the trained 4-block checkpoint, one 400-simulation move:
                                                                     the move with the switch off and on (host clock around Engine.search), and
                                                                     on the SAME trees the read-out calls tree_stats() and tree_proofs(max_len=1)
                                                                     -- the same walk without and with the sweep; the classes of the roots
    python tools/time_proof_moves.py --leg kernels                   one such move, then --calls of each read-out and one move with the switch on:
                                                                     the leg to run under `rocprofv3 --kernel-trace --stats` for the kernels' own
                                                                     times (k_tree_stats, k_tree_proofs, k_proof_pi, k_end_move)
    python tools/time_proof_moves.py --leg selfplay --json b.json    --selfplay-games games played to the end with the switch on: moves per verdict
    python tools/time_proof_moves.py --leg evaluate --json c.json    64 matches of the checkpoint against itself, proof moves on the player's side
                                                                     only, colours alternating: W / D / L and the verdicts
    python tools/time_proof_moves.py --all --out DIR                 legs cost, selfplay, evaluate: a fresh child process each, under its own limit

Leg cost: the games are first played --plies plies from the empty board at --open-sims simulations and the positions kept; every timed
search starts from them with the same seeds on fresh trees, so the searches with the switch off and on build THE SAME trees (the switch
changes pi alone) and the difference of their times is what the two launches and the verdict copy cost. The configurations alternate,
--repeats times, after one untimed search of each. The read-out calls are timed on the trees of the last search with the switch off; a
call's time includes its mask upload, its download and its synchronise, so the KERNEL times come from leg kernels under rocprofv3.
Leg evaluate is one sample of 64 games and claims nothing beyond it."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
CKPT = os.path.join(REPO, "profiles", "r4_trained_9x9_4block.pt")


def model(ckpt):
    import torch
    from alpha_omok_amd.pvnet import PVNet
    m = PVNet(4, 5, 128, 9)
    m.load_state_dict(torch.load(ckpt, map_location="cpu"))
    return m.eval()


def midgame(a, eng, net, games, seeds):
    """The ids every configuration searches: --plies plies at --open-sims simulations; a slot whose game ended searches a copy of one
    that has not (under its own seed)."""
    eng.seed_all(seeds)
    alive = np.ones(games, np.uint8)
    for _ in range(a.plies):
        eng.search(net, tau=np.ones(games, np.int8), active=alive, sims=a.open_sims)
        _, win = eng.play()
        alive &= (win == 0).astype(np.uint8)
    ids = [(0,) + tuple(eng.get_moves(g)) for g in range(games)]
    live = np.flatnonzero(alive)
    if live.size == 0:
        raise SystemExit("every game ended within %d plies: nothing to time" % a.plies)
    ended = np.flatnonzero(alive == 0)
    for k, g in enumerate(ended):
        ids[g] = ids[live[k % live.size]]
    return ids, int(ended.size)


def leg_cost(a, kernels_only=False):
    import torch
    from alpha_omok_amd import utils
    from alpha_omok_amd.engine import Engine, Net
    games = a.games
    net = Net(4, 5, 128, 9, 0)
    net.load_state_dict(model(a.ckpt).state_dict())
    eng = Engine(9, a.sims, 5, games=games, noise=True)
    seeds = np.arange(1000, 1000 + games, dtype=np.uint32)
    ids, copies = midgame(a, eng, net, games, seeds)
    mask = np.ones(games, np.uint8)

    def search(on, tau):
        eng.set_proof_moves(on)
        eng.reset()
        eng.seed_all(seeds)
        eng.set_roots(ids, mask)
        eng.proof_move_stats(reset=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = eng.search(net, tau=np.full(games, tau, np.int8), active=mask)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def call(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        return time.perf_counter() - t0, r

    search(False, 1)                                        # warm-up: every kernel of both forms
    search(True, 1)
    if kernels_only:
        search(False, 1)
        for _ in range(a.calls):
            eng.tree_stats()
            eng.tree_proofs(max_len=1)
        search(True, 1)
        eng.close()
        net.close()
        return dict(games=games, sims=a.sims, calls=a.calls)
    t_off, t_on, verdicts, same = [], [], {}, True
    for _ in range(a.repeats):
        for tau in (1, 0):
            s, (pi_on, vis_on, _) = search(True, tau)
            t_on.append(s)
            verdicts[tau] = eng.proof_move_stats()
            s, (pi_off, vis_off, _) = search(False, tau)      # (last: the read-outs below read the trees of a plain search)
            t_off.append(s)
            same = same and np.array_equal(vis_on, vis_off)
    eng.tree_stats()
    eng.tree_proofs(max_len=1)
    t_stats, t_proofs = [], []
    for _ in range(a.calls):
        t_stats.append(call(eng.tree_stats)[0])
        s, pr = call(lambda: eng.tree_proofs(max_len=1))
        t_proofs.append(s)
    st = eng.tree_stats()
    full_s, full = call(eng.tree_proofs)
    classes = {name: int((full["status"] == v).sum()) for name, v in
               (("unknown", utils.PROOF_UNKNOWN), ("win", utils.PROOF_WIN), ("loss", utils.PROOF_LOSS), ("draw", utils.PROOF_DRAW))}
    lost_child = int(((full["child_status"] == utils.PROOF_LOSS).any(axis=1) & (full["status"] == utils.PROOF_UNKNOWN)).sum())
    eng.close()
    net.close()
    ms = lambda v: [round(1e3 * x, 3) for x in v]                                       # noqa: E731
    move = min(t_off)
    return dict(board=9, blocks=4, games=games, slots_searching_a_copy=copies, sims=a.sims, plies_played_first=a.plies, open_sims=a.open_sims,
                weights="checkpoint " + os.path.relpath(a.ckpt, REPO), repeats=a.repeats, calls=a.calls,
                clock="host clock around the call; every call ends in a stream synchronise",
                move_ms_off=ms(t_off), move_ms_on=ms(t_on), best_move_ms_off=round(1e3 * move, 3), best_move_ms_on=round(1e3 * min(t_on), 3),
                on_over_off=round(min(t_on) / move, 5), visits_equal_on_and_off=bool(same),
                tree_stats_call_ms=ms(t_stats), tree_proofs_call_ms=ms(t_proofs), best_tree_stats_call_ms=round(1e3 * min(t_stats), 3),
                best_tree_proofs_call_ms=round(1e3 * min(t_proofs), 3), tree_proofs_full_lines_call_ms=round(1e3 * full_s, 3),
                proofs_call_share_of_move=round(min(t_proofs) / move, 5),
                mean_nodes_walked=round(float(st["expanded"].mean()), 1), mean_proven_nodes=round(float(full["proven"].mean()), 2),
                root_classes=classes, unknown_roots_with_a_lost_child=lost_child,
                verdicts_tau1=verdicts[1], verdicts_tau0=verdicts[0])


def leg_selfplay(a):
    import torch
    from alpha_omok_amd.engine import Engine, Net
    games = a.selfplay_games
    net = Net(4, 5, 128, 9, 0)
    net.load_state_dict(model(a.ckpt).state_dict())
    eng = Engine(9, a.sims, 5, games=games, noise=True)
    eng.seed_all(np.arange(5000, 5000 + games, dtype=np.uint32))
    eng.set_proof_moves(True)
    alive = np.ones(games, np.uint8)
    by_ply, wins, ply = [], np.zeros(4, np.int64), 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while alive.any():
        tau = np.full(games, 1 if ply < a.tau_plies else 0, np.int8)            # main.self_play's schedule
        eng.search(net, tau=tau, active=alive)
        st = eng.proof_move_stats(reset=True)
        by_ply.append([st["none"], st["win"], st["pruned"], st["moved"]])
        _, win = eng.play()
        for w in win[alive == 1]:
            wins[int(w)] += 1 if w else 0
        alive &= (win == 0).astype(np.uint8)
        ply += 1
    torch.cuda.synchronize()
    s = time.perf_counter() - t0
    eng.close()
    net.close()
    tot = np.array(by_ply).sum(axis=0)
    return dict(leg="selfplay", games=games, sims=a.sims, tau_plies=a.tau_plies, plies=ply, moves=int(tot.sum()),
                verdicts=dict(none=int(tot[0]), win=int(tot[1]), pruned=int(tot[2]), moved=int(tot[3])),
                verdicts_by_ply=by_ply, results=dict(black=int(wins[1]), white=int(wins[2]), draw=int(wins[3])), seconds=round(s, 2))


def leg_evaluate(a):
    import torch
    from alpha_omok_amd import evaluate
    net = model(a.ckpt).cuda()
    evaluate.evaluate_batched(net, net, 9, 16, n_match=4, seed=1, proof_moves=(True, False))      # warm-up: library, kernels, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    result, elo, games = evaluate.evaluate_batched(net, net, 9, a.sims, n_match=a.matches, seed=a.seed, proof_moves=(True, False))
    torch.cuda.synchronize()
    s = time.perf_counter() - t0
    plies = sum(len(g[1]) for g in games)
    return dict(leg="evaluate", matches=a.matches, sims=a.sims, proof_moves=[True, False], result=result, verdicts_player=evaluate.last_proof_moves.get(0),
                elo=dict(player=round(elo[0], 1), enemy=round(elo[1], 1)), plies=plies, seconds=round(s, 3), moves_per_s=round(plies / s, 1))


def run_all(a):
    """Every leg in a child process of its own, each under its own time limit; stops at the first that fails or runs out of time."""
    os.makedirs(a.out, exist_ok=True)
    for leg in a.legs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--json", os.path.join(a.out, leg + ".json"), "--games", str(a.games),
               "--sims", str(a.sims), "--matches", str(a.matches), "--seed", str(a.seed), "--ckpt", a.ckpt, "--repeats", str(a.repeats),
               "--plies", str(a.plies), "--open-sims", str(a.open_sims), "--calls", str(a.calls), "--selfplay-games", str(a.selfplay_games),
               "--tau-plies", str(a.tau_plies)]
        try:
            rc = subprocess.run(cmd, timeout=a.leg_timeout).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit("leg %s ran out of its %d s: stopping here" % (leg, a.leg_timeout))
        if rc != 0:
            raise SystemExit("leg %s failed with exit status %d: stopping here" % (leg, rc))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--leg", choices=("cost", "kernels", "selfplay", "evaluate"))
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--legs", default="cost,selfplay,evaluate", help="with --all: the legs to run, in order")
    ap.add_argument("--out", default="proof_moves_timing")
    ap.add_argument("--leg-timeout", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=2, help="leg cost: timed searches per configuration and tau, the configurations alternating")
    ap.add_argument("--calls", type=int, default=10, help="legs cost / kernels: timed calls of each read-out")
    ap.add_argument("--ckpt", default=CKPT)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--plies", type=int, default=12, help="legs cost / kernels: plies played before the timed move")
    ap.add_argument("--open-sims", type=int, default=32, help="... at this many simulations")
    ap.add_argument("--selfplay-games", type=int, default=1024)
    ap.add_argument("--tau-plies", type=int, default=6, help="leg selfplay: tau is 1 for this many plies, then 0")
    ap.add_argument("--matches", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", default=None, help="write the result here")
    a = ap.parse_args()
    if a.all:
        run_all(a)
        return
    if not a.leg:
        ap.error("--leg or --all")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    if a.leg == "cost":
        res = dict(leg="cost", **leg_cost(a))
    elif a.leg == "kernels":
        res = dict(leg="kernels", **leg_cost(a, kernels_only=True))
    elif a.leg == "selfplay":
        res = leg_selfplay(a)
    else:
        res = leg_evaluate(a)
    res.update(gpu=torch.cuda.get_device_name(0))
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
