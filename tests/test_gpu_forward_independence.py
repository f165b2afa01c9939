"""-m gpu: a board's (policy, value) depends on the board and on the kernel that ran it -- not on its row, not on the boards around
it, not on how ragged the last group is. Equality of bits; no reference is evaluated and there is no tolerance.

1. Every kernel name of the forward (the smallest case of each (kernel, weights on the fp16 grid or not) of net_reference.CASES,
   a second one with a ragged last group where the smallest is a multiple of 16, and the 14 one-product names): the five checks
   of tests/forward_independence.py -- twins, constant, permutation, neighbours, tail. tests/test_forward_independence_host.py
   shows on the CPU that they pass on a forward that is independent by construction and see five small defects.
2. Mode 6, "one arithmetic for every batch size": six probe boards at row 0 and on the last row of a ladder of batch sizes must
   have the bits of their batch-of-one evaluation.
3. The bit-plane conv1 forms, which only ao_search reaches: games that share a seed are the same search, so their records in the
   evaluation log (Engine.set_eval_log) must be equal launch by launch, and stay what they were when every game between them
   searches something else.

With AO_INDEPENDENCE_REPORT=<file> every case appends a JSON line (profiles/r32a_forward_independence.txt keeps a copy)."""
import json
import os

import numpy as np
import pytest

import forward_independence as FI
import net_reference as R
from test_gpu_memory_guard import F16_CASES

pytestmark = pytest.mark.gpu

# {kernel head: reason}: families whose arithmetic legitimately changes with the number of groups, excluded from the TAIL check
# alone (a reason is a place in the kernel's code). None of mode 6's kernels (k_layer16h, k_layer16h_w16, k_layer16h_f16) and
# no head kernel may be listed.
SIZE_DEPENDENT = {
    "k_conv_cells": "the per-board fp32 path (networks of other than 128 planes) is two instantiations under one reported name: "
                    "net_forward_il (csrc/net.hip, `const int nw = (boards <= 4 || ...) ? 9 : 3`) launches k_conv_cells<W, Q, 9>, one "
                    "tap per wave and a nine-way sum through LDS, for up to four boards and k_conv_cells<W, Q, 3>, three taps "
                    "accumulated in one wave's MFMA chain, from five boards on: another summation order (found by this test at 5 "
                    "against 4 boards: 1 - 2 ulp in p on every row). Inside either form the arithmetic does not depend on the size",
}
# ... and the one batch size whose n - 1 is on the other side of that seam: everywhere else the family's tail check runs
SIZE_SEAM = {"k_conv_cells": 5}


def _report(rec):
    print("INDEPENDENCE " + json.dumps(rec))
    if os.environ.get("AO_INDEPENDENCE_REPORT"):
        with open(os.environ["AO_INDEPENDENCE_REPORT"], "a") as f:
            f.write(json.dumps(rec) + "\n")


# ----------------------------------------------------------------------------------------------------------------------------
# 1. every kernel name
# ----------------------------------------------------------------------------------------------------------------------------
def _cost(c):
    return c.batch * max(c.nb, 1)            # as tests/test_gpu_memory_guard.py picks its smallest case per name


def _kernel_cases():
    best, ragged = {}, {}
    for c in R.CASES:
        key = (c.kernel, c.grid)
        if key not in best or _cost(c) < _cost(best[key]):
            best[key] = c
        if c.batch % 16 and (key not in ragged or _cost(c) < _cost(ragged[key])):
            ragged[key] = c
    out = []
    for key, c in best.items():
        out.append(c)
        if c.batch % 16 == 0 and key in ragged:
            out.append(ragged[key])
    return list(best), out


KERNEL_NAMES, KERNEL_CASES = _kernel_cases()


def batch_sizes():
    """Every batch size a permutation is made for."""
    return {c.batch for c in KERNEL_CASES} | {c[4] for c in F16_CASES}


def test_the_cases_cover_every_kernel_name():
    assert len(KERNEL_NAMES) == len({(c.kernel, c.grid) for c in R.CASES}) == 105
    assert {(c.kernel, c.grid) for c in KERNEL_CASES} == set(KERNEL_NAMES)
    assert len(F16_CASES) == len({c[5] for c in F16_CASES}) == 14
    for key in KERNEL_NAMES:                 # a ragged last group wherever a case of the name has one
        if any((c.kernel, c.grid) == key and c.batch % 16 for c in R.CASES):
            assert any((c.kernel, c.grid) == key and c.batch % 16 for c in KERNEL_CASES), key
    for head in SIZE_DEPENDENT:
        assert head.startswith("k_") and "<" not in head and head not in ("k_layer16h", "k_layer16h_w16", "k_layer16h_f16") and "head" not in head


def _forward_of(net):
    import torch

    def fwd(x):
        p, v = net(torch.from_numpy(x).cuda())
        torch.cuda.synchronize()
        return p.cpu().numpy(), v.cpu().numpy()
    return fwd


def _five_checks(net, kernel, n, B, C, tag):
    """The five checks on `net` at n boards; the kernel name is asserted first, the tail check runs where the library names the
    same kernel for n - 1 boards and the family is not in SIZE_DEPENDENT."""
    name = net.dominant_kernel(n)[0]
    assert name.startswith(kernel), (name, kernel)
    if R.is_split_fp16(kernel):
        assert ("2 products" if "_w16<" in kernel else "3 products") in name, name
    same = n > 1 and net.dominant_kernel(n - 1)[0] == name
    head = kernel.split("<")[0]
    excluded = head in SIZE_DEPENDENT and SIZE_SEAM.get(head, n) == n
    ck = FI.Checker(_forward_of(net), kernel, n, B, C)
    ran = ck.run(tail=same and not excluded)
    assert ran[:4] == list(FI.CHECKS[:4]) and (("tail" in ran) == (same and not excluded))
    assert net.status() == 0
    _report(dict(tag, kernel=name.split(" (")[0], B=B, C=C, batch=n, checks=ran,
                 tail="run" if "tail" in ran else "SIZE_DEPENDENT" if same and excluded else "another kernel at n - 1" if n > 1 else "one board",
                 permutation_coverage=round(FI.coverage(FI.permutation(n)), 4), result="equal bits"))


@pytest.mark.parametrize("case", KERNEL_CASES, ids=[c.id for c in KERNEL_CASES])
def test_every_kernel_name(case, monkeypatch):
    from alpha_omok_amd.engine import Net
    from alpha_omok_amd.pvnet import native_width, pad_state_dict
    sd = R.case_network(*case.net_key())
    width = native_width(case.planes)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    net = Net(case.nb, case.C, width, case.B, 0)
    for k in case.env:
        monkeypatch.delenv(k)
    try:
        net.load_state_dict(sd if width == case.planes else pad_state_dict(sd, width))
        net.set_mode(case.mode)
        if width == 128 and case.nb >= 1:
            assert net.products() == (case.products, case.grid), net.products()
        _five_checks(net, case.kernel, case.batch, case.B, case.C,
                     dict(id=case.id, family=case.family, nb=case.nb, planes=case.planes, mode=case.mode, grid=case.grid, precision="fp32"))
    finally:
        net.close()


@pytest.mark.parametrize("precision,mode,nb,B,batch,kernel", F16_CASES, ids=[c[5].replace(" ", "") for c in F16_CASES])
def test_every_one_product_kernel_name(precision, mode, nb, B, batch, kernel):
    """The one-product kernels on the conditioned network with weights on the fp16 grid (what the fp16 forward computes with),
    whose activations are no fp16 numbers: every stored activation is rounded, in every row."""
    from alpha_omok_amd.engine import Net
    net = Net(nb, 5, 128, B, 0)
    try:
        net.set_mode(mode)
        net.load_state_dict(R.case_network(nb, B, 128, True))
        assert net.precision(precision) == precision
        _five_checks(net, kernel, batch, B, 5, dict(id="%s-nb%d-B%d-%d-m%d" % (precision, nb, B, batch, mode), family=kernel.split("<")[0][2:],
                                                      nb=nb, planes=128, mode=mode, grid=True, precision=precision))
    finally:
        net.close()


# ----------------------------------------------------------------------------------------------------------------------------
# 2. mode 6: one arithmetic for every batch size
# ----------------------------------------------------------------------------------------------------------------------------
LADDER_9 = (1, 2, 15, 16, 17, 33, 64, 65, 257, 768, 1040, 3073)
LADDER = (1, 17, 63, 64, 65, 130)
LADDERS = [(9, 5, False, "fp32"), (9, 5, True, "fp32"), (9, 5, False, "fp16-all"), (9, 3, False, "fp32"), (9, 9, False, "fp32")] + \
          [(B, 5, grid, "fp32") for B in (4, 8, 13, 15) for grid in (False, True)]


def probe_boards(B, C):
    """Six pool boards: full, empty, a float-plane board and three random ones."""
    ns = R.n_structured(B, C)
    names = R.structured_boards(B, C)[1]
    return [names.index("full"), names.index("empty, colour 0"), FI.lively_board(B, C), ns, ns + 1, ns + 2]


@pytest.mark.parametrize("B,C,grid,precision", LADDERS,
                         ids=["B%d-C%d-%s-%s" % (B, C, "w16grid" if grid else "w32", precision) for B, C, grid, precision in LADDERS])
def test_mode_6_is_one_arithmetic_for_every_batch_size(B, C, grid, precision):
    from alpha_omok_amd.engine import Net
    net = Net(2, C, 128, B, 0)
    try:
        net.load_state_dict(R.case_network(2, B, 128, grid, C))
        net.set_mode(6)
        assert net.precision(precision) == precision
        kernel = "k_layer16h%s<%d>" % ("_f16" if precision == "fp16-all" else "_w16" if grid else "", B)
        fwd = _forward_of(net)
        pool = R.pool(B, C)
        probes = probe_boards(B, C)
        assert len(set(probes)) == 6
        alone = {}
        for b in probes:
            assert net.dominant_kernel(1)[0].startswith(kernel), net.dominant_kernel(1)[0]
            alone[b] = FI.bits(fwd(pool[[b]]))
        sizes = LADDER_9 if B == 9 else LADDER
        for n in sizes:
            assert net.dominant_kernel(n)[0].startswith(kernel), (n, net.dominant_kernel(n)[0])
            for k in range(6 if n > 1 else 0):
                m = np.array(R.batch_indices(n, B, C))
                first, last = probes[k], probes[(k + 1) % 6]           # each probe once at row 0 and once on the last row
                m[0], m[n - 1] = first, last
                out = FI.bits(fwd(pool[m]))
                for row, b in ((0, first), (n - 1, last)):
                    FI.same_rows("mode 6 ladder", kernel, out, [row], alone[b], [0], [b], " of %d boards" % n, " of a batch of one")
        assert net.status() == 0
        _report(dict(id="ladder-B%d-C%d-%s-%s" % (B, C, "w16grid" if grid else "w32", precision), kernel=kernel, B=B, C=C, batches=list(sizes),
                     checks=["mode 6 ladder"], probes=probes, result="equal bits"))
    finally:
        net.close()


# ----------------------------------------------------------------------------------------------------------------------------
# 3. the bit-plane forms, through ao_search and the evaluation log
# ----------------------------------------------------------------------------------------------------------------------------
SEARCHES = [(9, 3072, 8, 0, "k_trunk16hb<9, 4, 0>"), (10, 64, 8, 0, "k_boardh<10, 2>"), (15, 65, 6, 0, "k_boardh<15, 2>"),
            (9, 768, 8, 0, "k_layer16hk<9, 4>"), (9, 70, 8, 6, "k_layer16h<9>"), (9, 48, 8, 0, "k_row16hk<9>"),
            (9, 5, 16, 0, "k_conv_cells_h<9, 8>")]           # (5 games: the per-board path and the fused per-game step)
SEARCH_CASES = [s + (grid, "fp32") for s in SEARCHES for grid in (False, True)] + [s + (True, "fp16") for s in SEARCHES[:2]]


def _logged_search(net, B, G, S, seeds):
    """One search (noise on, no leaf symmetry, tau = 1) of a fresh engine with every game in the evaluation log ->
    (records uint32 [launches, G, A + 3], visit [G, A])."""
    import torch
    from alpha_omok_amd.engine import Engine
    A = B * B
    eng = Engine(B, S, 5, games=G, noise=True)
    try:
        eng.seed_all(np.asarray(seeds, np.uint32))
        log = torch.zeros(((S + 8) * G * (A + 3),), dtype=torch.float32, device="cuda")
        eng.set_eval_log(range(G), log.data_ptr(), log.numel())
        pi, vis, pol = eng.search(net, tau=np.ones(G, np.int8))
        n_rec = eng.eval_log_count()
        assert S <= n_rec <= S + 8, n_rec
        rec = log[:n_rec * G * (A + 3)].cpu().numpy().reshape(n_rec, G, A + 3)
        eng.set_eval_log([])
        assert eng.fp16_range_events()[0] == 0
        assert (vis.sum(axis=1) == S).all()
    finally:
        eng.close()
    return rec, vis


def _same_records(check, kernel, a, games_a, b, games_b, seeds, A):
    """records [launches, G, A + 3] float32: a[:, games_a[k]] and b[:, games_b[k]] bit-equal -- policy row, value, simulations
    done and leaf status -- launch by launch"""
    ua, ub = a.view(np.uint32), b.view(np.uint32)
    for s in range(len(a)):
        if np.array_equal(ua[s, games_a], ub[s, games_b]):
            continue
        bad = np.flatnonzero((ua[s, games_a] != ub[s, games_b]).any(axis=1))
        k = int(bad[0])
        ga, gb = int(games_a[k]), int(games_b[k])
        cell = int(np.flatnonzero(ua[s, ga] != ub[s, gb])[0])
        where = ("policy cell %d" % cell) if cell < A else ("value", "simulations done", "leaf status")[cell - A]
        raise AssertionError("%s, %s, launch %d: game %d (group %d, lane %d) and game %d (group %d, lane %d) share seed %d and differ, first at "
                             "%s: %r (0x%08x) against %r (0x%08x); status %r / %r; %d of %d compared games differ in this launch"
                             % (check, kernel, s, ga, ga // 16, ga % 16, gb, gb // 16, gb % 16, int(seeds[ga]), where, a[s, ga, cell],
                                int(ua[s, ga, cell]), b[s, gb, cell], int(ub[s, gb, cell]), a[s, ga, A + 2], b[s, gb, A + 2], bad.size, len(games_a)))


@pytest.mark.parametrize("B,G,S,mode,kernel,grid,precision", SEARCH_CASES,
                         ids=["%s-G%d-S%d-m%d-%s-%s" % (k.replace(" ", ""), G, S, mode, "w16grid" if grid else "w32", precision)
                              for B, G, S, mode, k, grid, precision in SEARCH_CASES])
def test_search_evaluations_of_games_that_share_a_seed(B, G, S, mode, kernel, grid, precision):
    from alpha_omok_amd.engine import Net, plan_kernel
    A = B * B
    K = 24 if G >= 24 else 2
    assert plan_kernel(2, 5, 128, B, G, in_kind=2, trunk_mode=mode)[0].startswith(kernel)
    net = Net(2, 5, 128, B, 0)
    try:
        net.load_state_dict(R.case_network(2, B, 128, grid))
        net.set_mode(mode)
        assert net.precision(precision) == precision
        head, _, tail = kernel.partition("<")
        form = "_f16" if precision == "fp16" else "_w16" if grid else ""
        float_plane_name = head.replace("k_trunk16hb", "k_trunk16h") + form + "<" + tail.replace(", 2>", ", 1>")
        assert net.dominant_kernel(G)[0].startswith(float_plane_name), (net.dominant_kernel(G)[0], float_plane_name)
        g = np.arange(G)
        seeds = 1000 + g % K
        rec, vis = _logged_search(net, B, G, S, seeds)
        evaluated = np.isin(rec[:, :, A + 2], (1, 2))
        assert evaluated.sum() >= S * G // 2 and len(np.unique(rec[:, :K, :A][evaluated[:, :K]], axis=0)) > K    # (the log is alive)
        twins = g[K:]
        _same_records("twins of a search", kernel, rec, twins % K, rec, twins, seeds, A)
        assert np.array_equal(vis[twins % K], vis[twins]), "visit counts of games that share a seed differ"
        kept = (g < K) | (g >= G - K)
        seeds2 = np.where(kept, seeds, 5000 + g)
        assert (~kept).any() or G <= 2 * K                                     # (48 games are the first 24 and the last 24)
        rec2, vis2 = _logged_search(net, B, G, S, seeds2)
        assert len(rec2) == len(rec)
        _same_records("neighbours of a search", kernel, rec2, g[kept], rec, g[kept], seeds, A)
        assert np.array_equal(vis2[kept], vis[kept])
        if (~kept).any():
            assert not np.array_equal(vis2[~kept], vis[~kept])                # (the games between them did search something else)
        assert net.status() == 0
        _report(dict(id="search-%s-G%d-%s-%s" % (kernel.replace(" ", ""), G, "w16grid" if grid else "w32", precision), kernel=kernel, B=B, C=5,
                     batch=G, sims=S, mode=mode, launches=len(rec), checks=["twins of a search", "neighbours of a search"], result="equal bits"))
    finally:
        net.close()
