#!/usr/bin/env python
"""Measures the rolling search (main.configure(rolling=True), Engine.roll_*) against the synchronous one with the committed trained
9x9 4-block checkpoint: self_play(4096) at 400 simulations, oversubscribe 1.25, the same seeds, one process per row.

    python tools/time_rolling.py --row sync_off --json a.json          one row, in this process
    python tools/time_rolling.py --all --out DIR                       every row, a fresh child process each, under its own time limit
    python tools/time_rolling.py --update-design DIR/*.json --raw profiles/NAME.txt

Rows: sync_off, sync_es16 (early stop, settle_every 16), roll_off16 (rolling, turn_every 16), roll_es4 / roll_es8 / roll_es16 /
roll_es32 (rolling with early stop), sync_cap / roll_cap16 (playout cap: fast_sims 50, full_prob 0.25, no early stop), and
sync_es16_over / roll_es16_over (early stop with 5120 episodes on 5120 slots and 4096 rows: the rows where over-subscription binds).
Per row: searches (move decisions), simulations saved by early stop, wall seconds, move decisions per second and
rows_live / rows_launched of ao_row_stats. A move decision searched with fewer simulations is not the unit of the README's tables:
the rolling rows with early stop are read against sync_es16 of the same run, the others against sync_off / sync_cap.
--update-design rewrites the block between the rolling_timing markers of DESIGN.md section 6 and writes the raw JSON lines to --raw."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
CKPT = os.path.join(REPO, "profiles", "r4_trained_9x9_4block.pt")
BEGIN, END = "<!-- rolling_timing:begin -->", "<!-- rolling_timing:end -->"
B, BLOCKS, PLANES = 9, 4, 128
# row -> (rolling, early stop, settle_every / turn_every, playout cap, games in place of --games)
# (self_play(4096) fills 4096 slots -- never more slots than episodes -- so oversubscribe 1.25 binds in no row above the last two:
# those play 5120 episodes on 5120 slots and 4096 rows)
ROWS = {"sync_off": (False, False, None, False, None), "sync_es16": (False, True, 16, False, None), "roll_off16": (True, False, 16, False, None),
        "roll_es4": (True, True, 4, False, None), "roll_es8": (True, True, 8, False, None), "roll_es16": (True, True, 16, False, None),
        "roll_es32": (True, True, 32, False, None), "sync_cap": (False, False, None, True, None), "roll_cap16": (True, False, 16, True, None),
        "sync_es16_over": (False, True, 16, False, 5120), "roll_es16_over": (True, True, 16, False, 5120)}
ORDER = list(ROWS)


def model(ckpt):
    import torch
    from alpha_omok_amd.pvnet import PVNet
    m = PVNet(BLOCKS, 5, PLANES, B)
    m.load_state_dict(torch.load(ckpt, map_location="cpu"))
    return m.cuda().eval()


def run_row(a):
    import torch
    import alpha_omok_amd.engine as engine
    import alpha_omok_amd.main as m
    rolling, early, every, cap, games = ROWS[a.row]
    games = games or a.games
    if early and not rolling:
        engine.SETTLE_EVERY = every
    kw = dict(fast_sims=50, full_prob=0.25) if cap else {}
    m.configure(board_size=B, n_mcts=a.sims, n_blocks=BLOCKS, out_planes=PLANES, seed=a.seed, model=model(a.ckpt), device_replay=True,
                carry_over=False, oversubscribe=a.oversubscribe, early_stop=early, rolling=rolling, turn_every=every if rolling else None, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = m.self_play(games)
    torch.cuda.synchronize()
    s = time.perf_counter() - t0
    ran, rows = m._engine.sims_run(), m._engine.row_stats()
    res = dict(row=a.row, path="rolling" if rolling else "synchronous", early_stop=early, every=every, playout_cap=cap, games=games, sims=a.sims,
               oversubscribe=a.oversubscribe, slots=m._engine.G, seconds=round(s, 3), play_seconds=round(m.phase_seconds["play"], 3),
               searches=int(out["moves"]), samples=int(out.get("samples", 0)), searches_settled=int(ran["settled_total"]),
               simulations_saved=int(ran["saved_total"]), move_decisions_per_s=round(out["moves"] / s, 1), launches=rows["launches"],
               rows_live=rows["rows_live"], rows_launched=rows["rows_launched"], waits=rows["waits"],
               playout=dict(m.playout_totals), gpu=torch.cuda.get_device_name(0))
    if rolling:
        res["roll"] = m._engine.roll_stats()
    return res


def run_all(a):
    """Every row in a child process of its own, under its own time limit; stops at the first row that fails or runs out of time."""
    os.makedirs(a.out, exist_ok=True)
    for row in (a.rows or ORDER):
        path = os.path.join(a.out, row + ".json")
        cmd = [sys.executable, os.path.abspath(__file__), "--row", row, "--json", path, "--games", str(a.games), "--sims", str(a.sims),
               "--oversubscribe", str(a.oversubscribe), "--seed", str(a.seed), "--ckpt", a.ckpt]
        try:
            rc = subprocess.run(cmd, timeout=a.row_timeout).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit("row %s ran out of its %d s: stopping here" % (row, a.row_timeout))
        if rc != 0:
            raise SystemExit("row %s failed with exit status %d: stopping here" % (row, rc))


def update_design(paths, raw):
    runs = {}
    for p in paths:
        with open(p) as f:
            r = json.load(f)
        runs[r["row"]] = r
    lines = [BEGIN, "The rolling search against the synchronous one with the trained 9×9 4-block checkpoint (`python tools/time_rolling.py`; "
             "`self_play(%d)` (5120 in the `_over` rows), %d simulations, oversubscribe %.2f, one process per row, same seeds; a move decision searched with fewer "
             "simulations is not the unit of the tables above):" % (next(iter(runs.values()))["games"], next(iter(runs.values()))["sims"],
                                                                   next(iter(runs.values()))["oversubscribe"]), "",
             "| row | path | games / slots | early stop | playout cap | settle / turn every | searches | simulations saved | wall s | move decisions/s | rows live / launched | waits |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name in ORDER:
        if name not in runs:
            continue
        r = runs[name]
        budget = r["searches"] * r["sims"] if not r["playout_cap"] else r["playout"]["full"] * r["sims"] + r["playout"]["fast"] * 50
        lines.append("| %s | %s | %d / %d | %s | %s | %s | %d | %.1f %% | %.1f | %.0f | %.3f | %d |" % (
            name, r["path"], r["games"], r["slots"], "on" if r["early_stop"] else "off", "50 / 0.25" if r["playout_cap"] else "off", r["every"] or "—", r["searches"],
            100.0 * r["simulations_saved"] / max(budget, 1), r["seconds"], r["move_decisions_per_s"], r["rows_live"] / max(r["rows_launched"], 1), r["waits"]))
    lines += ["", "GPU: %s." % next(iter(runs.values())).get("gpu", "?"), END]
    path = os.path.join(REPO, "DESIGN.md")
    with open(path) as f:
        text = f.read()
    if BEGIN not in text or END not in text:
        raise SystemExit("DESIGN.md has no rolling_timing markers")
    head, rest = text.split(BEGIN, 1)
    with open(path, "w") as f:
        f.write(head + "\n".join(lines) + rest.split(END, 1)[1])
    if raw:
        with open(raw, "w") as f:
            for name in ORDER:
                if name in runs:
                    f.write(json.dumps(runs[name]) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--row", choices=ORDER)
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--rows", nargs="+", choices=ORDER, default=None, help="with --all: these rows only")
    ap.add_argument("--out", default="build/time_rolling", help="with --all: where the rows' JSON files go")
    ap.add_argument("--row-timeout", type=int, default=240, help="with --all: seconds a row's process may take")
    ap.add_argument("--ckpt", default=CKPT)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--oversubscribe", type=float, default=1.25)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", default=None, help="write the result here")
    ap.add_argument("--update-design", nargs="+", metavar="JSON", default=None)
    ap.add_argument("--raw", default=None, help="with --update-design: write the rows' JSON lines here (profiles/...)")
    a = ap.parse_args()
    if a.update_design:
        update_design(a.update_design, a.raw)
        return
    if a.all:
        run_all(a)
        return
    if not a.row:
        ap.error("--row, --all or --update-design")
    res = run_row(a)
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
