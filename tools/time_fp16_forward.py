#!/usr/bin/env python
"""Measures the opt-in fp16 forward (Net.precision("fp16"), ao_net_precision) against the fp32-equivalent kernels: the THREE-, TWO- and
ONE-product forms of the trunk kernel on the same box, in ONE process, alternating.

    python tools/time_fp16_forward.py [--rounds 3] [--json out.json]
    python tools/time_fp16_forward.py --update-design out.json

Legs (each form: a warm-up ply, then --rounds windows of --plies plies, the forms alternating inside a round):
  * 4096 x 9x9, 4 blocks, 400 simulations per move with the committed trained checkpoints -- profiles/r4_trained_9x9_4block.pt
    (arbitrary fp32 weights: three products and one) and profiles/r6j_trained_fp16grid_9x9_4block.pt (weights on the fp16 grid:
    three, two and one);
  * 1024 x 15x15, 10 blocks, 100 simulations, seeded He-initialised weights on the fp16 grid (k_boardh; no trained checkpoint of
    that shape is committed).
Per form: the trunk launch time from Net.conv_timing (HIP events around the launches of the dominant kernel, every 4th forward)
and move decisions/s of the search leg (host clock around Engine.search + play, which end in a synchronise). The three- and
two-product kernels are the code of the parent commit, unchanged by the fp16 forward; they are the baseline, measured here beside
it. For the trained networks also max / mean |dp|, |dv| and top-1 agreement of fp16 against the default forward on 1024 positions of
the leg's own games, and a 64-game evaluate_batched match of the fp16 side against the default side of the same checkpoint
(AO_FORCE_RESIDENT=1 for these two networks, so that 64 boards run the resident trunk -- without it a 64-board batch is planned
onto k_row16hk and both sides would be the same arithmetic).

--update-design rewrites the block between the fp16_forward_timing markers of DESIGN.md section 6 from the JSON file."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
CKPTS = {"trained fp32 weights": os.path.join(REPO, "profiles", "r4_trained_9x9_4block.pt"),
         "trained fp16-grid weights": os.path.join(REPO, "profiles", "r6j_trained_fp16grid_9x9_4block.pt")}
BEGIN, END = "<!-- fp16_forward_timing:begin -->", "<!-- fp16_forward_timing:end -->"


def trained(path):
    import torch
    from alpha_omok_amd.pvnet import PVNet
    m = PVNet(4, 5, 128, 9)
    m.load_state_dict(torch.load(path, map_location="cpu"))
    return m.eval()


def wide_model():
    import torch
    from alpha_omok_amd.pvnet import PVNet
    torch.manual_seed(0)
    m = PVNet(10, 5, 128, 15).eval()
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 4 and p.shape[2] == 3:
                p.copy_(p.half().float())
    return m


def set_form(net, form):
    """form: 3 / 2 / 1 products per multiply-add"""
    net.precision("fp16" if form == 1 else "fp32")
    net.products(3 if form == 3 else 0)


def search_leg(net, forms, B, games, sims, plies, rounds, seed):
    """Per form: {kernel, trunk_ms: [per round], decisions_per_s: [per round]}; and the positions (move lists) its games reached."""
    import numpy as np
    import torch
    from alpha_omok_amd.engine import Engine
    out = {f: dict(kernel=None, trunk_ms=[], decisions_per_s=[]) for f in forms}
    seeds = np.arange(seed, seed + games, dtype=np.uint32)
    tau = np.ones(games, np.int8)
    positions = None
    for _ in range(rounds):
        for f in forms:                     # alternating: a drift of the box hits every form alike
            set_form(net, f)
            eng = Engine(B, sims, 5, games=games, noise=True)      # (one engine at a time: its tree arenas take a large share of the HBM)
            eng.seed_all(seeds)
            eng.search(net, tau=tau)        # warm-up ply: code objects, workspace, tree arenas; every window then times plies 2 .. of the same games
            eng.play()
            net.conv_timing(4)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(plies):
                eng.search(net, tau=tau)
                eng.play()
            torch.cuda.synchronize()
            s = time.perf_counter() - t0
            ms, cnt = net.conv_timing(False)
            out[f]["kernel"] = net.dominant_kernel(games)[0].split(" (")[0]
            out[f]["trunk_ms"].append(round(ms / max(cnt, 1), 4))
            out[f]["decisions_per_s"].append(round(games * plies / s, 1))
            if positions is None:
                positions = [[0] + eng.get_moves(g) for g in range(min(games, 1024))]
            eng.close()
    assert net.status() == 0, "an activation left the fp16 range during the timed searches"
    return out, positions


def accuracy(net, positions, B):
    """fp16 against the default forward on the positions (padded by repetition to 4096 boards: the resident trunk's batch)."""
    import numpy as np
    import torch
    from alpha_omok_amd import utils
    x = np.stack([utils.get_state_pt(tuple(p), B, 5) for p in positions]).astype(np.float32)
    reps = (4096 + len(x) - 1) // len(x)
    xt = torch.from_numpy(np.concatenate([x] * reps)[:4096]).cuda()
    res = {}
    for prec in ("fp32", "fp16"):
        net.precision(prec)
        net.products(0)
        p, v = net(xt)
        torch.cuda.synchronize()
        res[prec] = (p[:len(x)].double().cpu().numpy(), v[:len(x)].double().cpu().numpy(), net.dominant_kernel(4096)[0].split(" (")[0])
    dp = np.abs(res["fp32"][0] - res["fp16"][0])
    dv = np.abs(res["fp32"][1] - res["fp16"][1])
    return dict(positions=len(x), kernel_default=res["fp32"][2], kernel_fp16=res["fp16"][2], max_dp=float(dp.max()), mean_dp=float(dp.mean()),
                max_dv=float(dv.max()), mean_dv=float(dv.mean()),
                top1_agreement=float((res["fp32"][0].argmax(axis=1) == res["fp16"][0].argmax(axis=1)).mean()))


def match(model, sims, n_match, seed):
    """fp16 side (player) against the default side (enemy) of the same checkpoint; AO_FORCE_RESIDENT=1 so that both run the
    resident trunk at 64 boards."""
    from alpha_omok_amd import evaluate
    os.environ["AO_FORCE_RESIDENT"] = "1"
    try:
        a, b = model.to_native(0), model.to_native(0)
    finally:
        del os.environ["AO_FORCE_RESIDENT"]
    a.precision("fp16")
    t0 = time.perf_counter()
    result, _, games = evaluate.evaluate_batched(a, b, 9, sims, n_match=n_match, seed=seed)
    s = time.perf_counter() - t0
    out = dict(matches=n_match, sims=sims, fp16_side=result["Player"], default_side=result["Enemy"], draws=result["Draw"],
               kernel_fp16=a.dominant_kernel(n_match)[0].split(" (")[0], kernel_default=b.dominant_kernel(n_match)[0].split(" (")[0],
               plies=sum(len(g[1]) for g in games), seconds=round(s, 1))
    a.close()
    b.close()
    return out


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def update_design(path):
    with open(path) as f:
        r = json.load(f)
    lines = [BEGIN, "The fp16 forward against the fp32-equivalent kernels (`python tools/time_fp16_forward.py`; one process, the forms alternating, "
             "median of %d windows with [min .. max]; raw output: `%s`):" % (r["rounds"], r.get("raw", "profiles/")), "",
             "| workload | products | kernel | trunk launch ms | move decisions/s | launch vs the default form |", "|---|---|---|---|---|---|"]
    for leg in r["legs"]:
        forms = leg["forms"]
        default = med(forms[str(leg["default_form"])]["trunk_ms"])
        for f in sorted(forms, reverse=True):
            t, d = forms[f]["trunk_ms"], forms[f]["decisions_per_s"]
            lines.append("| %s | %s%s | `%s` | %.3f [%.3f .. %.3f] | %.0f [%.0f .. %.0f] | x%.2f |" % (
                leg["what"], f, " (default)" if int(f) == leg["default_form"] else " (fp16 forward)" if f == "1" else "", forms[f]["kernel"],
                med(t), min(t), max(t), med(d), min(d), max(d), default / med(t)))
    lines += ["", "fp16 against the default forward of the same checkpoint, on positions of the leg's own games, and a match of the two "
              "(fp16 side : default side : draws):", "", "| network | positions | max / mean abs dp | max / mean abs dv | top-1 agreement | match |", "|---|---|---|---|---|---|"]
    for leg in r["legs"]:
        if "accuracy" in leg:
            a, m = leg["accuracy"], leg.get("match")
            lines.append("| %s | %d | %.1e / %.1e | %.1e / %.1e | %.2f %% | %s |" % (
                leg["network"], a["positions"], a["max_dp"], a["mean_dp"], a["max_dv"], a["mean_dv"], 100 * a["top1_agreement"],
                "%d : %d : %d over %d games at %d sims" % (m["fp16_side"], m["default_side"], m["draws"], m["matches"], m["sims"]) if m else "--"))
    lines += ["", "GPU: %s." % r.get("gpu", "?"), END]
    p = os.path.join(REPO, "DESIGN.md")
    with open(p) as f:
        text = f.read()
    if BEGIN not in text or END not in text:
        raise SystemExit("DESIGN.md has no fp16_forward_timing markers")
    head, rest = text.split(BEGIN, 1)
    with open(p, "w") as f:
        f.write(head + "\n".join(lines) + rest.split(END, 1)[1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--plies", type=int, default=2, help="plies per timed window")
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--wide-games", type=int, default=1024)
    ap.add_argument("--wide-sims", type=int, default=100)
    ap.add_argument("--matches", type=int, default=64)
    ap.add_argument("--match-sims", type=int, default=100)
    ap.add_argument("--no-match", action="store_true")
    ap.add_argument("--no-wide", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", default=None)
    ap.add_argument("--raw", default=None, help="where the raw output is kept (named in the DESIGN.md block)")
    ap.add_argument("--update-design", metavar="JSON", default=None)
    a = ap.parse_args()
    if a.update_design:
        update_design(a.update_design)
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures, it does not fall back")
    legs = []
    for name, path in CKPTS.items():
        model = trained(path)
        net = model.to_native(0)
        forms = [3, 2, 1] if net.products()[1] else [3, 1]
        res, positions = search_leg(net, forms, 9, a.games, a.sims, a.plies, a.rounds, 4000 + a.seed)
        leg = dict(what="%d x 9x9, 4 blocks, %d sims, %s" % (a.games, a.sims, name), network=name, default_form=forms[1] if len(forms) == 3 else 3,
                   forms={str(f): res[f] for f in forms}, accuracy=accuracy(net, positions, 9))
        net.close()
        if not a.no_match:
            leg["match"] = match(model, a.match_sims, a.matches, a.seed)
        print("LEG " + json.dumps(leg), flush=True)
        legs.append(leg)
    if not a.no_wide:
        net = wide_model().to_native(0)
        res, _ = search_leg(net, [3, 2, 1], 15, a.wide_games, a.wide_sims, a.plies, a.rounds, 9000 + a.seed)
        leg = dict(what="%d x 15x15, 10 blocks, %d sims, seeded weights on the fp16 grid" % (a.wide_games, a.wide_sims), network="15x15 seeded",
                   default_form=2, forms={str(f): res[f] for f in (3, 2, 1)})
        net.close()
        print("LEG " + json.dumps(leg), flush=True)
        legs.append(leg)
    out = dict(rounds=a.rounds, plies=a.plies, legs=legs, gpu=torch.cuda.get_device_name(0), raw=a.raw)
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
