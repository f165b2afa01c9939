#!/usr/bin/env python
"""Measures leaf tactics (Engine.set_leaf_tactics: the forced-win solver on every leaf, its proof overriding the value).

    python tools/time_leaf_tactics.py --leg cost --json a.json       time per simulation of one 400-simulation move of 4096 games on the
                                                                     trained 9x9 4-block checkpoint: the switch off, on (the solver beside
                                                                     the network launch) and on (AO_LEAF_TACTICS_SERIAL), for (max_depth,
                                                                     max_nodes) in (2,16), (4,64), (6,256), forward "fp32" and "fp16"
    python tools/time_leaf_tactics.py --leg cost15 --json b.json     the same at 15x15, 10 blocks, 1024 games (random weights: no 15x15
                                                                     checkpoint is committed; the cost is what is measured)
    python tools/time_leaf_tactics.py --leg evaluate --json c.json   64 matches of the checkpoint against itself, leaf tactics on the
                                                                     player's side only, colours alternating: W / D / L and the move rate
    python tools/time_leaf_tactics.py --all --out DIR                every leg, a fresh child process each, under its own time limit

Legs cost / cost15: every configuration searches THE SAME move -- the games are first played --plies plies from the empty board at
--open-sims simulations, the positions are kept, and each timed search starts from them with the same seeds on fresh trees. The time is
a host clock around Engine.search, which ends in a stream synchronise, divided by the simulations; every configuration runs --repeats
times, the configurations alternating, after one untimed search that warms every kernel up. With the switch on the searches differ from
the plain one (other values, other trees), so a row compares times per simulation, not identical work. The counters of
Engine.leaf_tactics_stats are reported per configuration: leaves searched, proven, out of nodes, solver nodes per leaf.
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
LIMITS = ((2, 16), (4, 64), (6, 256))
SERIAL = "AO_LEAF_TACTICS_SERIAL"


def model(board, blocks, ckpt):
    import torch
    from alpha_omok_amd.pvnet import PVNet
    torch.manual_seed(15)
    m = PVNet(blocks, 5, 128, board)
    if ckpt:
        m.load_state_dict(torch.load(ckpt, map_location="cpu"))
    return m.eval()


def leg_cost(a, board, blocks, games, ckpt):
    import torch
    from alpha_omok_amd.engine import Engine, Net
    net = Net(blocks, 5, 128, board, 0)
    net.load_state_dict(model(board, blocks, ckpt).state_dict())
    eng = Engine(board, a.sims, 5, games=games, noise=True)
    seeds = np.arange(1000, 1000 + games, dtype=np.uint32)
    # the positions every configuration searches: --plies plies of self-play at --open-sims simulations, games that ended left out
    eng.seed_all(seeds)
    alive = np.ones(games, np.uint8)
    for _ in range(a.plies):
        eng.search(net, tau=np.ones(games, np.int8), active=alive, sims=a.open_sims)
        _, win = eng.play()
        alive &= (win == 0).astype(np.uint8)
    ids = [(0,) + tuple(eng.get_moves(g)) for g in range(games)]
    # a slot whose game has ended searches a copy of a position that has not (under its own seed): every row of the batch is live
    live = np.flatnonzero(alive)
    if live.size == 0:
        raise SystemExit("every game ended within %d plies: nothing to time" % a.plies)
    ended = np.flatnonzero(alive == 0)
    for k, g in enumerate(ended):
        ids[g] = ids[live[k % live.size]]
    mask = np.ones(games, np.uint8)
    tau = np.ones(games, np.int8)

    def once(limits, serial, precision):
        net.precision(precision)
        eng.set_leaf_tactics(*limits) if limits else eng.set_leaf_tactics(None)
        eng.reset()
        eng.seed_all(seeds)
        eng.set_roots(ids, mask)
        eng.leaf_tactics_stats(reset=True)
        if serial:
            os.environ[SERIAL] = "1"
        else:
            os.environ.pop(SERIAL, None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.search(net, tau=tau, active=mask)
        torch.cuda.synchronize()
        s = time.perf_counter() - t0
        os.environ.pop(SERIAL, None)
        st = eng.leaf_tactics_stats()
        return s, st

    configs = [(None, False)] + [(lim, ser) for lim in LIMITS for ser in (False, True)]
    rows = []
    for precision in ("fp32", "fp16"):
        once((4, 64), False, precision)                     # warm-up: every kernel of both forms
        once((4, 64), True, precision)
        once(None, False, precision)
        times = {c: [] for c in configs}
        stats = {}
        for _ in range(a.repeats):
            for c in configs:
                s, st = once(c[0], c[1], precision)
                times[c].append(s)
                stats[c] = st
        off = min(times[configs[0]])
        for c in configs:
            st = stats[c]
            per_sim = [1e6 * s / (a.sims + 1) for s in times[c]]          # (a fresh root's expansion is one simulation more)
            rows.append(dict(forward=precision, limits=list(c[0]) if c[0] else None, form="off" if not c[0] else ("serial" if c[1] else "overlapped"),
                             us_per_simulation=[round(x, 1) for x in per_sim], best_us_per_simulation=round(min(per_sim), 1),
                             over_off=round(min(times[c]) / off, 4), searched=st["searched"], proven=st["proven"], unknown=st["unknown"],
                             nodes_per_leaf=round(st["nodes"] / max(st["searched"], 1), 2)))
    eng.close()
    net.close()
    return dict(board=board, blocks=blocks, games=games, slots_searching_a_copy=int(ended.size), sims=a.sims, plies_played_first=a.plies, open_sims=a.open_sims,
                weights="checkpoint " + os.path.relpath(ckpt, REPO) if ckpt else "random (torch.manual_seed(15))", repeats=a.repeats,
                clock="host clock around Engine.search (ends in a stream synchronise) / (sims + 1)", rows=rows)


def leg_evaluate(a):
    import torch
    from alpha_omok_amd import evaluate
    net = model(9, 4, a.ckpt).cuda()
    lt = dict(max_depth=a.depth, max_nodes=a.nodes)
    evaluate.evaluate_batched(net, net, 9, 16, n_match=4, seed=1, leaf_tactics=(lt, None))      # warm-up: library, kernels, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    result, elo, games = evaluate.evaluate_batched(net, net, 9, a.sims, n_match=a.matches, seed=a.seed, leaf_tactics=(lt, None))
    torch.cuda.synchronize()
    s = time.perf_counter() - t0
    plies = sum(len(g[1]) for g in games)
    return dict(leg="evaluate", matches=a.matches, sims=a.sims, leaf_tactics=[lt, None], result=result,
                elo=dict(player=round(elo[0], 1), enemy=round(elo[1], 1)), plies=plies, seconds=round(s, 3), moves_per_s=round(plies / s, 1))


def run_all(a):
    """Every leg in a child process of its own, each under its own time limit; stops at the first that fails or runs out of time."""
    os.makedirs(a.out, exist_ok=True)
    for leg in a.legs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--json", os.path.join(a.out, leg + ".json"), "--games", str(a.games),
               "--sims", str(a.sims), "--matches", str(a.matches), "--seed", str(a.seed), "--ckpt", a.ckpt, "--repeats", str(a.repeats),
               "--plies", str(a.plies), "--open-sims", str(a.open_sims), "--depth", str(a.depth), "--nodes", str(a.nodes)]
        try:
            rc = subprocess.run(cmd, timeout=a.leg_timeout).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit("leg %s ran out of its %d s: stopping here" % (leg, a.leg_timeout))
        if rc != 0:
            raise SystemExit("leg %s failed with exit status %d: stopping here" % (leg, rc))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--leg", choices=("cost", "cost15", "evaluate"))
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--legs", default="cost,cost15,evaluate", help="with --all: the legs to run, in order")
    ap.add_argument("--out", default="leaf_tactics_timing")
    ap.add_argument("--leg-timeout", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=2, help="legs cost / cost15: timed searches per configuration, the configurations alternating")
    ap.add_argument("--ckpt", default=CKPT)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--games", type=int, default=4096, help="leg cost (leg cost15 searches a quarter as many)")
    ap.add_argument("--plies", type=int, default=12, help="legs cost / cost15: plies played before the timed move")
    ap.add_argument("--open-sims", type=int, default=32, help="... at this many simulations")
    ap.add_argument("--matches", type=int, default=64)
    ap.add_argument("--depth", type=int, default=2, help="leg evaluate: the player's max_depth")
    ap.add_argument("--nodes", type=int, default=16, help="leg evaluate: the player's max_nodes")
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
        res = dict(leg="cost", **leg_cost(a, 9, 4, a.games, a.ckpt))
    elif a.leg == "cost15":
        res = dict(leg="cost15", **leg_cost(a, 15, 10, max(1, a.games // 4), None))
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
