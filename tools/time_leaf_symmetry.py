#!/usr/bin/env python
"""Measures leaf symmetries (main.configure(leaf_symmetry=KEY), Engine.set_leaf_symmetry) with the committed trained 9x9 4-block
checkpoint.

    python tools/time_leaf_symmetry.py --leg self_play --json a.json    self_play(4096) at 400 simulations, the switch off / on / off / on in one process
    python tools/time_leaf_symmetry.py --leg evaluate  --json b.json    evaluate_batched of the checkpoint against itself, 64 matches:
                                                                         the player searches with leaf symmetries, the enemy plainly
    python tools/time_leaf_symmetry.py --all --out DIR                  both legs, a fresh child process each, under its own time limit

Leg self_play reports wall seconds and move decisions per second of every run and the ratio of the mean rates (on / off): the switch
adds no forward, only two index maps in the tree kernels and one dependent policy gather. The runs with the switch play other games than
those without (the evaluations differ), so the ratio compares rates, not the same work; the two runs of either kind play the same games
and show the run-to-run spread the ratio has to be read against. Leg evaluate reports the tally and the ELO after the 64 matches: a strength
measurement of one sample of 64 games, no more."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
CKPT = os.path.join(REPO, "profiles", "r4_trained_9x9_4block.pt")
B, BLOCKS, PLANES = 9, 4, 128


def model(ckpt):
    import torch
    from alpha_omok_amd.pvnet import PVNet
    m = PVNet(BLOCKS, 5, PLANES, B)
    m.load_state_dict(torch.load(ckpt, map_location="cpu"))
    return m.cuda().eval()


def leg_self_play(a):
    import torch
    import alpha_omok_amd.main as m
    net = model(a.ckpt)
    runs = {"warm_up": [], "off": [], "on": []}
    for name, key in [("warm_up", None)] + [("off", None), ("on", a.key)] * a.repeats:
        games = a.games if name != "warm_up" else min(a.games, 256)
        m.configure(board_size=B, n_mcts=a.sims, n_blocks=BLOCKS, out_planes=PLANES, seed=a.seed, model=net, device_replay=True,
                    carry_over=False, oversubscribe=a.oversubscribe, leaf_symmetry=key)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = m.self_play(games)
        torch.cuda.synchronize()
        s = time.perf_counter() - t0
        runs[name].append(dict(leaf_symmetry=key, games=games, seconds=round(s, 3), play_seconds=round(m.phase_seconds["play"], 3),
                               searches=int(out["moves"]), move_decisions_per_s=round(out["moves"] / s, 1)))
        m.release_engine()

    def mean_rate(rs):
        return sum(r["move_decisions_per_s"] for r in rs) / len(rs)
    return dict(leg="self_play", sims=a.sims, oversubscribe=a.oversubscribe, order="off, on" + ", off, on" * (a.repeats - 1), off=runs["off"],
                on=runs["on"], rate_on_over_off=round(mean_rate(runs["on"]) / mean_rate(runs["off"]), 4))


def leg_evaluate(a):
    import torch
    from alpha_omok_amd import evaluate
    net = model(a.ckpt)
    evaluate.evaluate_batched(net, net, B, 16, n_match=4, seed=1, leaf_symmetry=(a.key, None))      # warm-up: library, kernels, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    result, elo, games = evaluate.evaluate_batched(net, net, B, a.sims, n_match=a.matches, seed=a.seed, leaf_symmetry=(a.key, None))
    torch.cuda.synchronize()
    s = time.perf_counter() - t0
    return dict(leg="evaluate", matches=a.matches, sims=a.sims, leaf_symmetry=[a.key, None], result=result,
                elo=dict(player=round(elo[0], 1), enemy=round(elo[1], 1)), plies=sum(len(g[1]) for g in games), seconds=round(s, 3))


def run_all(a):
    """Both legs in child processes of their own, each under its own time limit; stops at the first that fails or runs out of time."""
    os.makedirs(a.out, exist_ok=True)
    for leg in ("self_play", "evaluate"):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--json", os.path.join(a.out, leg + ".json"), "--games", str(a.games),
               "--sims", str(a.sims), "--matches", str(a.matches), "--oversubscribe", str(a.oversubscribe), "--seed", str(a.seed),
               "--key", str(a.key), "--ckpt", a.ckpt, "--repeats", str(a.repeats)]
        try:
            rc = subprocess.run(cmd, timeout=a.leg_timeout).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit("leg %s ran out of its %d s: stopping here" % (leg, a.leg_timeout))
        if rc != 0:
            raise SystemExit("leg %s failed with exit status %d: stopping here" % (leg, rc))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--leg", choices=("self_play", "evaluate"))
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--out", default="leaf_symmetry_timing")
    ap.add_argument("--leg-timeout", type=int, default=600)
    ap.add_argument("--repeats", type=int, default=2, help="leg self_play: runs of either kind, alternating")
    ap.add_argument("--key", type=int, default=20260, help="the base key of the runs with the switch on")
    ap.add_argument("--ckpt", default=CKPT)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--matches", type=int, default=64)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--oversubscribe", type=float, default=1.25)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", default=None, help="write the result here")
    a = ap.parse_args()
    if a.all:
        run_all(a)
        return
    if not a.leg:
        ap.error("--leg or --all")
    import torch
    res = leg_self_play(a) if a.leg == "self_play" else leg_evaluate(a)
    res.update(gpu=torch.cuda.get_device_name(0))
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
