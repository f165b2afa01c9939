#!/usr/bin/env python
"""Measures the fp16 forward at every batch size (Net.precision("fp16-all"), k_layer16h_f16) against what the SAME batch runs under
"fp32" on the same net: the fp32-equivalent kernel it displaces (the per-board path, k_row16hk, k_layer16hk or k_layer16h), in
ONE process, the two forms alternating inside every round.

    python tools/time_fp16_all.py [--rounds 3] [--json out.json] [--raw profiles/...txt]
    python tools/time_fp16_all.py --update-design out.json

Legs:
  * forward: both committed 9x9 4-block checkpoints (profiles/r4_trained_9x9_4block.pt: arbitrary fp32 weights, three products;
    profiles/r6j_trained_fp16grid_9x9_4block.pt: weights on the fp16 grid, two products) at 1, 16, 64, 300, 1024 and 2048 boards,
    and 15x15 with 10 blocks (seeded weights on the fp16 grid) at 16 and 32 boards. Per form and round: a warm-up, then --forwards
    forwards of the same planes; the TRUNK time per forward = the HIP-event time of the dominant kernel's launches (Net.conv_timing,
    every forward timed: all convs behind conv1) / forwards, and the whole forward by the host clock around the window (conv1, heads
    and the layout kernel included; it ends in a synchronise);
  * search: evaluate_batched of a checkpoint against itself, 64 matches at 400 simulations, forward_precision "fp32" against
    "fp16-all" (seconds, plies, move decisions/s), and one ZeroAgent game (one tree, --agent-plies moves at 400 simulations).
The baseline is never an earlier number of the new kernel: it is the parent commit's kernel, untouched by this feature, measured
beside it here. A ratio below 1 means "fp16-all" is SLOWER than what it displaces.

--update-design rewrites the block between the fp16_all_timing markers of DESIGN.md section 6 from the JSON file."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from time_fp16_forward import CKPTS, med, trained, wide_model  # noqa: E402

BEGIN, END = "<!-- fp16_all_timing:begin -->", "<!-- fp16_all_timing:end -->"
FORMS = ("fp32", "fp16-all")


def forward_leg(net, B, boards, forwards, rounds, seed):
    """{form: {kernel, trunk_ms: [per round], forward_ms: [per round]}} for one batch size."""
    import numpy as np
    import torch
    rs = np.random.RandomState(seed + boards)
    x = (rs.rand(boards, 5, B, B) < 0.3).astype(np.float32)
    x[:, 4] = (rs.rand(boards, 1, 1) < 0.5)
    xt = torch.from_numpy(x).cuda()
    out = {f: dict(kernel=None, trunk_ms=[], forward_ms=[]) for f in FORMS}
    for _ in range(rounds):
        for f in FORMS:                         # alternating: a drift of the box hits both forms alike
            net.precision(f)
            for _ in range(5):
                net(xt)
            net.conv_timing(1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(forwards):
                net(xt)
            torch.cuda.synchronize()
            s = time.perf_counter() - t0
            ms, _ = net.conv_timing(False)
            out[f]["kernel"] = net.dominant_kernel(boards)[0].split(" (")[0]
            out[f]["trunk_ms"].append(round(ms / forwards, 5))
            out[f]["forward_ms"].append(round(1e3 * s / forwards, 5))
    assert net.status() == 0, "an activation left the fp16 range during the timed forwards"
    net.precision("fp32")
    return out


def match_leg(model, sims, n_match, rounds, seed):
    from alpha_omok_amd import evaluate
    out = {f: dict(seconds=[], plies=[], decisions_per_s=[], result=None) for f in FORMS}
    for r in range(rounds):
        for f in FORMS:
            t0 = time.perf_counter()
            result, _, games = evaluate.evaluate_batched(model, model, 9, sims, n_match=n_match, seed=seed, forward_precision=f)
            s = time.perf_counter() - t0
            plies = sum(len(g[1]) for g in games)
            out[f]["seconds"].append(round(s, 2))
            out[f]["plies"].append(plies)
            out[f]["decisions_per_s"].append(round(plies / s, 1))
            out[f]["result"] = [result["Player"], result["Enemy"], result["Draw"]]
    return out


def agent_leg(model, sims, plies, rounds, seed):
    """One ZeroAgent game: one tree, a forward of ONE board per simulation."""
    import numpy as np
    from alpha_omok_amd.agents import ZeroAgent
    out = {f: dict(seconds_per_move=[], kernel=None) for f in FORMS}
    for r in range(rounds):
        for f in FORMS:
            np.random.seed(seed)
            agent = ZeroAgent(9, sims, 5, noise=False)
            agent.model = model
            agent._evaluator.net_precision = f
            root = (0,)
            agent.get_pi(root, 0)               # warm-up: export, code objects, arena
            agent.reset()
            t0 = time.perf_counter()
            for _ in range(plies):
                pi = agent.get_pi(root, 0)
                root = root + (int(np.argmax(pi)),)
            s = time.perf_counter() - t0
            out[f]["seconds_per_move"].append(round(s / plies, 4))
            out[f]["kernel"] = agent._evaluator.native_net(model, 9, 5).dominant_kernel(1)[0].split(" (")[0]
    return out


def update_design(path):
    with open(path) as f:
        r = json.load(f)
    lines = [BEGIN, "`\"fp16-all\"` against what the same batch runs under `\"fp32\"` on the same net (`python tools/time_fp16_all.py`; one process, "
             "the two forms alternating, median of %d windows with [min .. max]; raw output: `%s`). Trunk = the launches of the dominant "
             "kernel per forward (HIP events), forward = host clock per `ao_net_forward`. A ratio below 1: fp16-all is SLOWER than the kernel "
             "it displaces." % (r["rounds"], r.get("raw", "profiles/")), "",
             "| network | boards | fp32 kernel | trunk ms | fp16-all kernel | trunk ms | trunk ratio | forward ms fp32 / fp16-all | forward ratio |",
             "|---|---|---|---|---|---|---|---|---|"]
    for leg in r["forward"]:
        a, b = leg["forms"]["fp32"], leg["forms"]["fp16-all"]
        lines.append("| %s | %d | `%s` | %.4f [%.4f .. %.4f] | `%s` | %.4f [%.4f .. %.4f] | x%.2f | %.4f / %.4f | x%.2f |" % (
            leg["network"], leg["boards"], a["kernel"], med(a["trunk_ms"]), min(a["trunk_ms"]), max(a["trunk_ms"]), b["kernel"],
            med(b["trunk_ms"]), min(b["trunk_ms"]), max(b["trunk_ms"]), med(a["trunk_ms"]) / med(b["trunk_ms"]),
            med(a["forward_ms"]), med(b["forward_ms"]), med(a["forward_ms"]) / med(b["forward_ms"])))
    lines += [""]
    for m in r.get("match", []):
        a, b = m["forms"]["fp32"], m["forms"]["fp16-all"]
        lines.append("`evaluate_batched`, %s against itself, %d matches at %d sims: fp32 %.0f move decisions/s [%.0f .. %.0f], fp16-all %.0f [%.0f .. %.0f] "
                     "(x%.2f)." % (m["network"], m["matches"], m["sims"], med(a["decisions_per_s"]), min(a["decisions_per_s"]), max(a["decisions_per_s"]),
                                   med(b["decisions_per_s"]), min(b["decisions_per_s"]), max(b["decisions_per_s"]),
                                   med(b["decisions_per_s"]) / med(a["decisions_per_s"])))
    for m in r.get("agent", []):
        a, b = m["forms"]["fp32"], m["forms"]["fp16-all"]
        lines.append("One `ZeroAgent` game, %s, %d sims, %d moves: fp32 %.3f s per move (`%s`), fp16-all %.3f s (`%s`) (x%.2f)." % (
            m["network"], m["sims"], m["plies"], med(a["seconds_per_move"]), a["kernel"], med(b["seconds_per_move"]), b["kernel"],
            med(a["seconds_per_move"]) / med(b["seconds_per_move"])))
    lines += ["", "GPU: %s." % r.get("gpu", "?"), END]
    p = os.path.join(REPO, "DESIGN.md")
    with open(p) as f:
        text = f.read()
    if BEGIN not in text or END not in text:
        raise SystemExit("DESIGN.md has no fp16_all_timing markers")
    head, rest = text.split(BEGIN, 1)
    with open(p, "w") as f:
        f.write(head + "\n".join(lines) + rest.split(END, 1)[1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--forwards", type=int, default=50, help="forwards per timed window")
    ap.add_argument("--boards", type=int, nargs="+", default=[1, 16, 64, 300, 1024, 2048])
    ap.add_argument("--wide-boards", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--matches", type=int, default=64)
    ap.add_argument("--match-sims", type=int, default=400)
    ap.add_argument("--match-rounds", type=int, default=1)
    ap.add_argument("--agent-plies", type=int, default=8)
    ap.add_argument("--no-match", action="store_true")
    ap.add_argument("--no-agent", action="store_true")
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
    fwd, match, agent = [], [], []
    nets = [(name, trained(path), 9) for name, path in CKPTS.items()]
    if not a.no_wide:
        nets.append(("15x15, 10 blocks, seeded fp16-grid weights", wide_model(), 15))
    for name, model, B in nets:
        net = model.to_native(0)
        for boards in (a.boards if B == 9 else a.wide_boards):
            leg = dict(network=name, board=B, boards=boards, forms=forward_leg(net, B, boards, a.forwards, a.rounds, a.seed))
            print("FORWARD " + json.dumps(leg), flush=True)
            fwd.append(leg)
        net.close()
    name, model, _ = nets[1]
    model = model.cuda()
    if not a.no_match:
        m = dict(network=name, matches=a.matches, sims=a.match_sims, forms=match_leg(model, a.match_sims, a.matches, a.match_rounds, a.seed))
        print("MATCH " + json.dumps(m), flush=True)
        match.append(m)
    if not a.no_agent:
        m = dict(network=name, sims=a.match_sims, plies=a.agent_plies, forms=agent_leg(model, a.match_sims, a.agent_plies, a.match_rounds, a.seed))
        print("AGENT " + json.dumps(m), flush=True)
        agent.append(m)
    out = dict(rounds=a.rounds, forwards=a.forwards, forward=fwd, match=match, agent=agent, gpu=torch.cuda.get_device_name(0), raw=a.raw)
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
