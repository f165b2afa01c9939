#!/usr/bin/env python
"""Measures what early stop (Engine.search(early_stop=...), k_settle) saves with the committed trained 9x9 4-block checkpoint:
the share of simulations saved, the share of searches settled, wall time and move decisions per second -- the switch off, then
on, same seeds, one process per configuration.

    python tools/time_early_stop.py --leg evaluate  --settle-every 0  --json off.json     evaluate_batched, 64 matches at 400 simulations
    python tools/time_early_stop.py --leg evaluate  --settle-every 16 --json on.json
    python tools/time_early_stop.py --leg self_play --settle-every 0|1|4|16|64 --json ...  self_play of 4096 games, oversubscribe 1.25
    python tools/time_early_stop.py --update-design a.json b.json ...

--settle-every 0 is the switch off (the plain search). A move decision searched with fewer simulations is not the unit of the
README's tables: the rate printed here is labelled `move_decisions_per_s_early_stop` when the switch is on and must not be set
beside those rows as a speed-up of them. --update-design rewrites the block between the early_stop_timing markers of DESIGN.md
section 6 from the JSON files."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
CKPT = os.path.join(REPO, "profiles", "r4_trained_9x9_4block.pt")
BEGIN, END = "<!-- early_stop_timing:begin -->", "<!-- early_stop_timing:end -->"
B, BLOCKS, PLANES = 9, 4, 128


def model(ckpt):
    import torch
    from alpha_omok_amd.pvnet import PVNet
    m = PVNet(BLOCKS, 5, PLANES, B)
    m.load_state_dict(torch.load(ckpt, map_location="cpu"))
    return m.cuda().eval()


def leg_evaluate(a):
    import torch
    import alpha_omok_amd.engine as engine
    from alpha_omok_amd import evaluate
    on = a.settle_every > 0
    if on:
        engine.SETTLE_EVERY = a.settle_every
    net = model(a.ckpt)
    evaluate.evaluate_batched(net, net, B, 16, n_match=4, seed=1, early_stop=on)        # warm-up: library, kernels, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    result, _, games = evaluate.evaluate_batched(net, net, B, a.sims, n_match=a.matches, seed=a.seed, early_stop=on)
    torch.cuda.synchronize()
    s = time.perf_counter() - t0
    tot = dict(evaluate.last_search_totals)
    return dict(leg="evaluate", matches=a.matches, sims=a.sims, result=result, plies=sum(len(g[1]) for g in games), seconds=round(s, 3),
                **rates(tot["searches"], tot["simulations"], tot["settled"], tot["saved"], tot["searches"], s, on))


def leg_self_play(a):
    import torch
    import alpha_omok_amd.engine as engine
    import alpha_omok_amd.main as m
    on = a.settle_every > 0
    if on:
        engine.SETTLE_EVERY = a.settle_every
    m.configure(board_size=B, n_mcts=a.sims, n_blocks=BLOCKS, out_planes=PLANES, seed=a.seed, model=model(a.ckpt), device_replay=True,
                carry_over=False, oversubscribe=a.oversubscribe, early_stop=on)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = m.self_play(a.games)
    torch.cuda.synchronize()
    s = time.perf_counter() - t0
    ran = m._engine.sims_run()
    tau0 = out["moves"] - min(out["moves"], m.TAU_THRES * a.games)     # searches with tau == 0 (every game here is longer than TAU_THRES)
    return dict(leg="self_play", games=a.games, sims=a.sims, oversubscribe=a.oversubscribe, slots=m._engine.G, seconds=round(s, 3),
                play_seconds=round(m.phase_seconds["play"], 3), searches_calls=m.search_totals["searches"],
                **rates(out["moves"], out["moves"] * a.sims, ran["settled_total"], ran["saved_total"], tau0, s, on))


def rates(searches, simulations, settled, saved, tau0_searches, seconds, on):
    key = "move_decisions_per_s_early_stop" if on else "move_decisions_per_s"
    return {"searches": int(searches), "tau0_searches": int(tau0_searches), "simulations_asked": int(simulations), "searches_settled": int(settled),
            "simulations_saved": int(saved), "share_simulations_saved": round(saved / max(simulations, 1), 4),
            "share_searches_settled": round(settled / max(searches, 1), 4), key: round(searches / seconds, 1)}


def update_design(paths):
    runs = []
    for p in paths:
        with open(p) as f:
            runs.append(json.load(f))
    lines = [BEGIN, "Early stop with the trained 9×9 4-block checkpoint (`python tools/time_early_stop.py`; one process per row, same seeds; "
             "a move decision searched with fewer simulations is not the unit of the tables above -- the last column is no speed-up of them):", "",
             "| workload | settle_every | searches | simulations saved | searches settled | wall s | move decisions/s (early-stopped ones where the switch is on) |",
             "|---|---|---|---|---|---|---|"]
    for r in sorted(runs, key=lambda r: (r["leg"], r["settle_every"])):
        what = ("`evaluate_batched`, %d matches, %d sims" % (r["matches"], r["sims"]) if r["leg"] == "evaluate"
                else "`self_play(%d)`, %d sims, oversubscribe %.2f" % (r["games"], r["sims"], r["oversubscribe"]))
        rate = r.get("move_decisions_per_s_early_stop", r.get("move_decisions_per_s"))
        lines.append("| %s | %s | %d | %.1f %% | %.1f %% | %.1f | %.0f |" % (what, r["settle_every"] or "off", r["searches"], 100 * r["share_simulations_saved"],
                                                                           100 * r["share_searches_settled"], r["seconds"], rate))
    lines += ["", "GPU: %s." % runs[0].get("gpu", "?"), END]
    path = os.path.join(REPO, "DESIGN.md")
    with open(path) as f:
        text = f.read()
    if BEGIN not in text or END not in text:
        raise SystemExit("DESIGN.md has no early_stop_timing markers")
    head, rest = text.split(BEGIN, 1)
    with open(path, "w") as f:
        f.write(head + "\n".join(lines) + rest.split(END, 1)[1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--leg", choices=("evaluate", "self_play"))
    ap.add_argument("--settle-every", type=int, default=0, help="0: early stop off")
    ap.add_argument("--ckpt", default=CKPT)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--matches", type=int, default=64)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--oversubscribe", type=float, default=1.25)
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
    res = leg_evaluate(a) if a.leg == "evaluate" else leg_self_play(a)
    res.update(settle_every=a.settle_every, gpu=torch.cuda.get_device_name(0))
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
