"""-m gpu: what an over-subscribed ao_search QUEUES, pinned. 24 games of 9x9 on 16 rows per simulation, 16 simulations, the
trained 2-block network on the split-fp16 kernels (mode 6), fixed seeds, four plies of search + play. The number of selection
launches, the rows that did work, the rows launched and the leaves that waited (ao_row_stats) are a function of the seeds alone:
the sit-out window, the planned extra launches and the catch-up rounds decide them. The same with settling (early_stop,
settle_every=4) on a second engine, where the simulations run and saved are pinned too (ao_search_sims).

The constants were recorded on the library of commit 56cadc9 (the search driver as one function, before it was split into
MoveSearch's phases and search_schedule.hpp); two runs of that library gave the same numbers in every field."""
import os
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

B, G, ROWS, S, PLIES = 9, 24, 16, 16, 4

# per ply, cumulative: (launches, rows_live, rows_launched, waits)
ROW_STATS = [(34, 408, 544, 0), (66, 792, 1056, 0), (98, 1176, 1568, 0), (130, 1560, 2080, 0)]
# the settling engine: the same, then per ply (simulations run over the 24 games, games settled), then settled_total / saved_total
ROW_STATS_SETTLING = [(31, 372, 496, 0), (63, 756, 1008, 0), (95, 1140, 1520, 0), (124, 1488, 1984, 0)]
SIMS_SETTLING = [(348, 24), (384, 0), (384, 0), (348, 24)]
SETTLED_TOTAL, SAVED_TOTAL = 48, 72


def run():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from make_trained_fixture import load
    from alpha_omok_amd.engine import Engine, Net
    net = Net(2, 5, 128, B, 0)
    net.load_state_dict(load(os.path.join(REPO, "tests", "golden", "trained_2block_9x9.npz")))
    net.set_mode(6)

    def engine():
        e = Engine(B, S, 5, games=G, noise=True)
        e.seed_all([4100 + g for g in range(G)])
        e.set_row_cap(ROWS)
        return e

    def stats(e):
        r = e.row_stats()
        return (r["launches"], r["rows_live"], r["rows_launched"], r["waits"])

    plain, settling = engine(), engine()
    out = dict(rows=[], rows_settling=[], sims_settling=[])
    for ply in range(PLIES):
        _, vis, _ = plain.search(net, tau=np.ones(G, np.int8))
        assert np.all(vis.sum(axis=1) >= S)
        plain.play()
        out["rows"].append(stats(plain))
        settling.search(net, tau=np.zeros(G, np.int8), early_stop=True, settle_every=4)
        ran = settling.sims_run()
        settling.play()
        out["rows_settling"].append(stats(settling))
        out["sims_settling"].append((int(ran["sims"].sum()), int(ran["settled"].sum())))
        out["settled_total"], out["saved_total"] = ran["settled_total"], ran["saved_total"]
    return out


def test_the_launches_of_an_over_subscribed_search_are_the_recorded_ones():
    got = run()
    print(got)
    assert got["rows"] == ROW_STATS
    assert got["rows_settling"] == ROW_STATS_SETTLING
    assert got["sims_settling"] == SIMS_SETTLING
    assert (got["settled_total"], got["saved_total"]) == (SETTLED_TOTAL, SAVED_TOTAL)
