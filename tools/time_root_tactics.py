#!/usr/bin/env python
"""Measures what the tactics switch (Engine.root_tactics, Engine.search(tactics=...)) costs and what it changes, with the
committed trained 9x9 4-block checkpoint.

    python tools/time_root_tactics.py --leg cost --max-nodes 128|512|2000 --json cost_512.json
        4096 games of self-play positions: the engine plays --warm-plies moves, then for --plies moves root_tactics is timed
        (host clock round the call, synchronised) beside the move's plain search: ms per move, its share of the search time,
        the share of games that reach the reply stage, and the slowest possible wave of k_forced_wins' rate for comparison
    python tools/time_root_tactics.py --leg effect --json effect.json
        64 evaluation matches, the side with the switch against the same network without it, same simulations: score, ELO
        difference, and evaluate.forced_win_summary / forced_defence_summary of either side's plies
    python tools/time_root_tactics.py --update-design cost_128.json cost_512.json cost_2000.json effect.json

One run per row, no claim beyond it. --update-design rewrites the block between the root_tactics_timing markers of DESIGN.md
section 6 from the JSON files."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
CKPT = os.path.join(REPO, "profiles", "r4_trained_9x9_4block.pt")
BEGIN, END = "<!-- root_tactics_timing:begin -->", "<!-- root_tactics_timing:end -->"
B, BLOCKS, PLANES = 9, 4, 128
US_PER_NODE = 32.5            # k_forced_wins, one wavefront


def model(ckpt):
    import torch
    from alpha_omok_amd.pvnet import PVNet
    m = PVNet(BLOCKS, 5, PLANES, B)
    m.load_state_dict(torch.load(ckpt, map_location="cpu"))
    return m.cuda().eval()


def leg_cost(a):
    from alpha_omok_amd.engine import RT_DEFEND, RT_LOST, RT_WIN, Engine
    net = model(a.ckpt).to_native(0)
    eng = Engine(B, a.sims, 5, games=a.games, noise=True)
    eng.seed_all(np.arange(a.seed, a.seed + a.games, dtype=np.uint32))
    alive = np.ones(a.games, np.uint8)
    tau = np.ones(a.games, np.int8)
    rows = []
    for ply in range(a.warm_plies + a.plies):
        if ply >= a.warm_plies:
            eng.root_tactics(alive, a.max_depth, a.max_nodes)       # (the first call allocates the workspace)
            eng.sync()
            t0 = time.perf_counter()
            rt = eng.root_tactics(alive, a.max_depth, a.max_nodes)
            eng.sync()
            t_rt = time.perf_counter() - t0
        t0 = time.perf_counter()
        eng.search(net, tau=tau, active=alive)
        eng.sync()
        t_search = time.perf_counter() - t0
        _, win = eng.play()
        if ply >= a.warm_plies:
            on = alive != 0
            v = rt["verdict"][on]
            rows.append(dict(ply=ply, games=int(on.sum()), ms_root_tactics=round(1e3 * t_rt, 3), ms_search=round(1e3 * t_search, 3),
                             win=int((v == RT_WIN).sum()), stage_b=int(((v == RT_DEFEND) | (v == RT_LOST)).sum()),
                             unknown=int((rt["unknown"][on] != 0).sum()), nodes_max=int(rt["nodes"][on].max()) if on.any() else 0))
        alive &= (win == 0).astype(np.uint8)
        if not alive.any():
            break
    ms_rt, ms_s = sum(r["ms_root_tactics"] for r in rows), sum(r["ms_search"] for r in rows)
    games = sum(r["games"] for r in rows)
    return dict(leg="cost", games=a.games, sims=a.sims, max_depth=a.max_depth, max_nodes=a.max_nodes, plies=len(rows),
                ms_per_move=round(ms_rt / max(len(rows), 1), 3), ms_search_per_move=round(ms_s / max(len(rows), 1), 3),
                share_of_search=round(ms_rt / max(ms_s, 1e-9), 4), share_stage_b=round(sum(r["stage_b"] for r in rows) / max(games, 1), 4),
                share_win=round(sum(r["win"] for r in rows) / max(games, 1), 4), share_unknown=round(sum(r["unknown"] for r in rows) / max(games, 1), 4),
                ms_max=max(r["ms_root_tactics"] for r in rows), ms_bound_one_wave=round(a.max_nodes * US_PER_NODE / 1e3, 2), rows=rows)


def _by_side(games, summary):
    """a by-colour summary of `games` as (player's plies, enemy's plies): match i's player is black when i is even"""
    even, odd = [g for i, g in enumerate(games) if i % 2 == 0], [g for i, g in enumerate(games) if i % 2 == 1]
    se, so = summary(even), summary(odd)
    add = lambda x, y: {k: x[k] + y[k] for k in x}
    return add(se["black"], so["white"]), add(se["white"], so["black"])


def leg_effect(a):
    from alpha_omok_amd import evaluate
    net = model(a.ckpt)
    tactics = dict(max_depth=a.max_depth, max_nodes=a.max_nodes)
    evaluate.evaluate_batched(net, net, B, 16, n_match=4, seed=1, tactics=(tactics, None))      # warm-up
    t0 = time.perf_counter()
    result, (pe, ee), games = evaluate.evaluate_batched(net, net, B, a.sims, n_match=a.matches, seed=a.seed, tactics=(tactics, None))
    s = time.perf_counter() - t0
    n = max(sum(result.values()), 1)
    score = (result["Player"] + 0.5 * result["Draw"]) / n
    elo = None if score in (0.0, 1.0) else round(-400.0 * math.log10(1.0 / score - 1.0), 1)
    fw = _by_side(games, lambda g: evaluate.forced_win_summary(g, B, a.max_depth, a.max_nodes))
    fd = _by_side(games, lambda g: evaluate.forced_defence_summary(g, B, a.max_depth, a.max_nodes))
    return dict(leg="effect", matches=a.matches, sims=a.sims, max_depth=a.max_depth, max_nodes=a.max_nodes, result=result,
                score=round(score, 4), elo_difference=elo, elo_after_K32=[round(pe, 1), round(ee, 1)], seconds=round(s, 2),
                plies=sum(len(g[1]) for g in games), forced_wins=dict(tactics=fw[0], plain=fw[1]), forced_defences=dict(tactics=fd[0], plain=fd[1]))


def update_design(paths):
    runs = []
    for p in paths:
        with open(p) as f:
            runs.append(json.load(f))
    cost = sorted((r for r in runs if r["leg"] == "cost"), key=lambda r: r["max_nodes"])
    lines = [BEGIN, "`Engine.root_tactics` with the trained 9×9 4-block checkpoint (`python tools/time_root_tactics.py`; one run per row, no claim "
             "beyond it):", "",
             "| games | max_nodes | moves timed | ms per move (largest) | the move's plain search, ms | share of it | games with a proven win | games "
             "at the reply stage | games with a search out of nodes | one wave at 32.5 µs per node, ms |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in cost:
        lines.append("| %d | %d | %d | %.2f (%.2f) | %.1f | %.2f %% | %.2f %% | %.2f %% | %.2f %% | %.2f |" % (
            r["games"], r["max_nodes"], r["plies"], r["ms_per_move"], r["ms_max"], r["ms_search_per_move"], 100 * r["share_of_search"],
            100 * r["share_win"], 100 * r["share_stage_b"], 100 * r["share_unknown"], r["ms_bound_one_wave"]))
    for r in (r for r in runs if r["leg"] == "effect"):
        lines += ["", "%d matches at %d simulations, the switch (max_depth %d, max_nodes %d) against the same network without it: %s, score %.3f, "
                  "ELO difference %s. Forced wins (depth >= 2) available / followed / missed: with the switch %d / %d / %d, without %d / %d / %d. "
                  "Opponent's forced wins faced / defended / blundered / hopeless: with the switch %d / %d / %d / %d, without %d / %d / %d / %d."
                  % ((r["matches"], r["sims"], r["max_depth"], r["max_nodes"], json.dumps(r["result"]), r["score"], r["elo_difference"])
                     + tuple(r["forced_wins"][s][k] for s in ("tactics", "plain") for k in ("forced_wins", "followed", "missed"))
                     + tuple(r["forced_defences"][s][k] for s in ("tactics", "plain") for k in ("threats", "defended", "blundered", "hopeless")))]
    lines += ["", "GPU: %s." % runs[0].get("gpu", "?"), END]
    path = os.path.join(REPO, "DESIGN.md")
    with open(path) as f:
        text = f.read()
    if BEGIN not in text or END not in text:
        raise SystemExit("DESIGN.md has no root_tactics_timing markers")
    head, rest = text.split(BEGIN, 1)
    with open(path, "w") as f:
        f.write(head + "\n".join(lines) + rest.split(END, 1)[1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--leg", choices=("cost", "effect"))
    ap.add_argument("--ckpt", default=CKPT)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--matches", type=int, default=64)
    ap.add_argument("--max-depth", type=int, default=6)
    ap.add_argument("--max-nodes", type=int, default=512)
    ap.add_argument("--warm-plies", type=int, default=10)
    ap.add_argument("--plies", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", default=None, help="write the result here")
    ap.add_argument("--update-design", nargs="+", metavar="JSON", default=None)
    a = ap.parse_args()
    if a.update_design:
        update_design(a.update_design)
        return
    if not a.leg:
        ap.error("--leg or --update-design")
    import torch
    res = leg_cost(a) if a.leg == "cost" else leg_effect(a)
    res.update(gpu=torch.cuda.get_device_name(0))
    print(json.dumps({k: v for k, v in res.items() if k != "rows"}))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
