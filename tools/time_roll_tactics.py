#!/usr/bin/env python
"""Measures the rolling search with the forced-win solver beside its loop (main.configure(rolling=True, roll_tactics=...),
Engine.roll_begin(tactics=...)) with the committed trained 9x9 4-block checkpoint: self_play(4096) at 400 simulations with early
stop, the same seeds, the four legs one after the other in ONE process:

    roll            rolling, no solver
    roll_tactics    rolling + the solver (512 nodes, no cap)
    roll_solved32   rolling + the solver with solved_sims = 32
    sync_tactics    the synchronous search with tactics= (512 nodes, no cap)

    python tools/time_roll_tactics.py --json DIR/legs.json
    python tools/time_roll_tactics.py --update-design DIR/legs.json --raw profiles/NAME.txt

Per leg: move decisions per second, simulations run, and for the rolling legs roll_tactics_stats -- the share of the game-turns
(turns x slots) that games spent waiting for a verdict, and the times the host had to wait for a batch. No speed is promised: what is
written down is each tactics leg's rate over the plain rolling leg's and over the synchronous tactics leg's, as measured.
--update-design rewrites the block between the roll_tactics_timing markers of DESIGN.md section 6 and writes the raw JSON to --raw."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
CKPT = os.path.join(REPO, "profiles", "r4_trained_9x9_4block.pt")
BEGIN, END = "<!-- roll_tactics_timing:begin -->", "<!-- roll_tactics_timing:end -->"
B, BLOCKS, PLANES = 9, 4, 128
LIMITS = dict(max_depth=6, max_nodes=512)
# leg -> configure keywords
LEGS = {"roll": dict(rolling=True), "roll_tactics": dict(rolling=True, roll_tactics=dict(LIMITS)),
        "roll_solved32": dict(rolling=True, roll_tactics=dict(LIMITS, solved_sims=32)), "sync_tactics": dict(tactics=dict(LIMITS))}
ORDER = list(LEGS)


def model(ckpt):
    import torch
    from alpha_omok_amd.pvnet import PVNet
    m = PVNet(BLOCKS, 5, PLANES, B)
    m.load_state_dict(torch.load(ckpt, map_location="cpu"))
    return m.cuda().eval()


def run_leg(a, name):
    import torch
    import alpha_omok_amd.main as m
    kw = dict(LEGS[name])
    if kw.get("rolling"):
        kw["turn_every"] = a.turn_every
    m.configure(board_size=B, n_mcts=a.sims, n_blocks=BLOCKS, out_planes=PLANES, seed=a.seed, model=model(a.ckpt), device_replay=True,
                carry_over=False, early_stop=True, **kw)
    before = dict(m.search_totals)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = m.self_play(a.games)
    torch.cuda.synchronize()
    s = time.perf_counter() - t0
    sims = sum(m.search_totals[k] - before[k] for k in ("evaluated", "terminal"))
    res = dict(leg=name, games=a.games, sims=a.sims, slots=m._engine.G, seconds=round(s, 3), searches=int(out["moves"]),
               move_decisions_per_s=round(out["moves"] / s, 1), simulations_run=int(sims), gpu=torch.cuda.get_device_name(0))
    if kw.get("rolling"):
        res["turn_every"] = a.turn_every
        res["roll"] = m._engine.roll_stats()
    if kw.get("roll_tactics"):
        st = m._engine.roll_tactics_stats()
        res["tactics"] = st
        res["waited_share"] = round(st["waited_turns"] / max(res["roll"]["turns"] * res["slots"], 1), 4)
    m.release_engine()
    return res


def update_design(path_json, raw):
    with open(path_json) as f:
        legs = {r["leg"]: r for r in json.load(f)}
    first = next(iter(legs.values()))
    lines = [BEGIN, "The rolling search with the solver beside its loop, trained 9×9 4-block checkpoint (`python tools/time_roll_tactics.py`; "
             "`self_play(%d)`, %d simulations, early stop, the four legs in one process, same seeds; solver limits depth 6 / 512 nodes):"
             % (first["games"], first["sims"]), "",
             "| leg | searches | simulations run | wall s | move decisions/s | × roll | × sync_tactics | batches | waited share of game-turns | host waits |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    base, sync = legs.get("roll"), legs.get("sync_tactics")
    for name in ORDER:
        if name not in legs:
            continue
        r = legs[name]
        t = r.get("tactics")
        lines.append("| %s | %d | %d | %.1f | %.0f | %s | %s | %s | %s | %s |" % (
            name, r["searches"], r["simulations_run"], r["seconds"], r["move_decisions_per_s"],
            "%.3f" % (r["move_decisions_per_s"] / base["move_decisions_per_s"]) if base else "—",
            "%.3f" % (r["move_decisions_per_s"] / sync["move_decisions_per_s"]) if sync else "—",
            t["batches"] if t else "—", "%.4f" % r["waited_share"] if t else "—", t["host_blocks"] if t else "—"))
    lines += ["", "GPU: %s." % first.get("gpu", "?"), END]
    path = os.path.join(REPO, "DESIGN.md")
    with open(path) as f:
        text = f.read()
    if BEGIN not in text or END not in text:
        raise SystemExit("DESIGN.md has no roll_tactics_timing markers")
    head, rest = text.split(BEGIN, 1)
    with open(path, "w") as f:
        f.write(head + "\n".join(lines) + rest.split(END, 1)[1])
    if raw:
        with open(raw, "w") as f:
            for name in ORDER:
                if name in legs:
                    f.write(json.dumps(legs[name]) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--legs", nargs="+", choices=ORDER, default=ORDER)
    ap.add_argument("--ckpt", default=CKPT)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--turn-every", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", default=None, help="write the legs' results here")
    ap.add_argument("--update-design", metavar="JSON", default=None)
    ap.add_argument("--raw", default=None, help="with --update-design: write the legs' JSON lines here (profiles/...)")
    a = ap.parse_args()
    if a.update_design:
        update_design(a.update_design, a.raw)
        return
    out = []
    for name in a.legs:
        out.append(run_leg(a, name))
        print(json.dumps(out[-1]), flush=True)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as f:
                json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
