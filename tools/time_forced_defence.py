#!/usr/bin/env python
"""Times PositionBatch.forced_defences, and its host definition utils.forced_defences, on the 9x9 and 15x15 positions of the
test fixture (tests/test_forced_defence_host.py: every prefix of the fixture games, max_depth 6, max_nodes 2000).

    python tools/time_forced_defence.py --device --json device.json     on a machine with the GPU
    python tools/time_forced_defence.py --host --json host.json         on any CPU (one core; minutes)
    python tools/time_forced_defence.py --update-design device.json host.json

Device: one call per board over all its positions, the host clock round the call (staging, both kernels and the download
included), median of --repeats calls after a warm-up call. Host: one pass. positions/s counts every id of the call, the
terminal ones included; searches/s the forced_win searches behind them (empty cells + 1 per open position).
--update-design rewrites the block between the forced_defence_timing markers of DESIGN.md section 6 from the JSON files."""
import argparse
import json
import os
import platform
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
BEGIN, END = "<!-- forced_defence_timing:begin -->", "<!-- forced_defence_timing:end -->"
BOARDS = (9, 15)


def workload(B):
    import test_forced_defence_host as T
    ids = T.ids_of(B)
    g = T.golden_fixture()[B]
    searches = int(g["counts"][:, 0].sum() + (g["status"] == 0).sum())
    return T, ids, g, searches


def time_device(repeats, device):
    from alpha_omok_amd.positions import PositionBatch
    out = {}
    for B in BOARDS:
        T, ids, g, searches = workload(B)
        with PositionBatch(B, win_mark=T.MARK[B], device=device) as pb:
            d = pb.forced_defences(ids, T.DEPTH, T.NODES)                      # warm-up: allocates the workspace
            for key in T.KEYS:
                assert (d[key] == g[key]).all(), "board %d: %s differs from the recorded host result" % (B, key)
            ms = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                pb.forced_defences(ids, T.DEPTH, T.NODES)
                ms.append(1e3 * (time.perf_counter() - t0))
        med = statistics.median(ms)
        out[str(B)] = dict(positions=len(ids), searches=searches, nodes=int(g["nodes"].sum()), repeats=repeats, ms_median=round(med, 3),
                           ms_min=round(min(ms), 3), ms_max=round(max(ms), 3), positions_per_s=round(1e3 * len(ids) / med, 1),
                           searches_per_s=round(1e3 * searches / med, 1))
    import torch
    return dict(kind="device", gpu=torch.cuda.get_device_name(device), boards=out)


def cpu_name():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def time_host():
    from alpha_omok_amd import utils
    out = {}
    for B in BOARDS:
        T, ids, g, searches = workload(B)
        t0 = time.perf_counter()
        nodes = sum(utils.forced_defences(rid[1:], B, T.MARK[B], T.DEPTH, T.NODES)["nodes"] for rid in ids)
        s = time.perf_counter() - t0
        assert nodes == int(g["nodes"].sum())
        out[str(B)] = dict(positions=len(ids), searches=searches, nodes=nodes, seconds=round(s, 2), positions_per_s=round(len(ids) / s, 2),
                           searches_per_s=round(searches / s, 1))
    return dict(kind="host", cpu=cpu_name(), boards=out)


def update_design(paths):
    runs = {}
    for p in paths:
        with open(p) as f:
            r = json.load(f)
        runs[r["kind"]] = r
    lines = [BEGIN, "`forced_defences` on the fixture positions of the tests, `max_depth` 6, `max_nodes` 2000 (`python tools/time_forced_defence.py "
             "--device`, `--host`; one run each, no performance claim beyond it):", "",
             "| board | positions | searches | nodes | device: ms per call (median; min – max) | positions/s | searches/s | host, one core: s | positions/s | searches/s |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for B in BOARDS:
        d = runs.get("device", {}).get("boards", {}).get(str(B))
        h = runs.get("host", {}).get("boards", {}).get(str(B))
        any_ = d or h
        dev = ("%.1f (%.1f – %.1f) | %.0f | %.0f" % (d["ms_median"], d["ms_min"], d["ms_max"], d["positions_per_s"], d["searches_per_s"])
               if d else "not measured | | ")
        host = "%.1f | %.2f | %.0f" % (h["seconds"], h["positions_per_s"], h["searches_per_s"]) if h else "not measured | | "
        lines.append("| %d×%d | %d | %d | %d | %s | %s |" % (B, B, any_["positions"], any_["searches"], any_["nodes"], dev, host))
    lines += ["", "Device: %s, host clock round the call, staging and download included, %s calls after a warm-up. Host: `utils.forced_defences`, %s."
              % (runs.get("device", {}).get("gpu", "not measured"), next(iter(runs["device"]["boards"].values()))["repeats"] if "device" in runs else "no",
                 runs.get("host", {}).get("cpu", "not measured")), END]
    path = os.path.join(REPO, "DESIGN.md")
    with open(path) as f:
        text = f.read()
    if BEGIN not in text or END not in text:
        raise SystemExit("DESIGN.md has no forced_defence_timing markers")
    head, rest = text.split(BEGIN, 1)
    tail = rest.split(END, 1)[1]
    with open(path, "w") as f:
        f.write(head + "\n".join(lines) + tail)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", action="store_true", help="time PositionBatch.forced_defences")
    ap.add_argument("--host", action="store_true", help="time utils.forced_defences")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--json", default=None, help="write the result here")
    ap.add_argument("--update-design", nargs="+", metavar="JSON", default=None)
    a = ap.parse_args()
    if a.update_design:
        update_design(a.update_design)
        return
    if a.device == a.host:
        ap.error("one of --device, --host or --update-design")
    res = time_device(a.repeats, a.gpu) if a.device else time_host()
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
