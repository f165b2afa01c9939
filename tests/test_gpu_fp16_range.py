"""-m gpu: the fp16-range guard of the network forward, per kernel family -- every kernel that stores an activation as fp16
halves clamps a value above 65504 AND sets AO_NET_FP16_RANGE (ao_net_status), for one element as for all, and for live rows only.

The networks are those of tests/fp16_range_nets.py: one channel leaves the range, nothing reads it, the outputs stay ordinary
(tests/test_fp16_range_host.py asserts on the CPU that they are what this file takes them for). Per family (the kernel is
asserted by name, FAMILIES has the shapes: the smallest that reaches the kernel, its two-product and one-product forms, and
the widths 4 and 7 beside 9):

  1. the ordinary network reports nothing;
  2. each dead-channel network (inner, last, stem) on a batch with OVER boards: status(clear=False) == 1, finite outputs, the
     next status() is 1 and the one after 0;
  3. the same weights on UNDER boards alone (4x4 and 10x10, where the pool has them): status 0;
  4. the outputs with the flag raised are the float64 evaluation of the dead network in logit space, within the family's bound
     (16 x E32, net_reference.Case.mult; the one-product forms 3 x E_fast of the host emulation, tests/test_gpu_fp16_forward.py),
     E32 / E_fast measured on THIS network and these boards. profiles/r31a_fp16_range_by_family.txt keeps the measured figures;
  5. the stem detector puts ONE activation of 70000 (reported) or 60000 (not reported, outputs within the ordinary bound) at a
     chosen (row of the batch, cell, channel), one forward per point: fp16_range_nets.sweep_points;
  6. a detector board on the last live row of a ragged group, then a smaller batch on the same Net in which that row is no
     longer live and no live board has a stone in plane 0: status 0.

The kernels that read bit planes have no forward entry point: a search reaches them (SEARCH_FAMILIES), and counts one event."""
import json
import os
import warnings

import numpy as np
import pytest

import fp16_range_nets as N
import net_reference as R

pytestmark = pytest.mark.gpu


def _net(fam, sd, monkeypatch):
    from alpha_omok_amd.engine import Net
    for k, v in fam.env.items():
        monkeypatch.setenv(k, v)
    net = Net(fam.nb, 5, 128, fam.B, 0)
    for k in fam.env:
        monkeypatch.delenv(k)
    net.load_state_dict(sd)
    net.set_mode(fam.mode)
    if fam.f16:
        assert net.precision(fam.precision) == fam.precision
    assert net.products() == (2 if fam.grid else 3, fam.grid), net.products()
    return net


def _forward(net, fam, x, boards=None):
    """(p, v as float64 numpy, status word read WITHOUT clearing) of one forward; the kernel is checked by name"""
    import torch
    p, v = net(x)
    torch.cuda.synchronize()
    name = net.dominant_kernel(boards or fam.batch)[0]
    assert name.startswith(fam.kernel), (name, fam.kernel)
    assert ("%d product" % fam.products) in name, name
    return p.cpu().double().numpy(), v.cpu().double().numpy(), net.status(clear=False)


def _errors(p, v, ref_l, ref_z):
    assert np.isfinite(p).all() and np.isfinite(v).all() and p.min() > 0 and np.abs(v).max() < 1
    lp = np.log(p)
    return (float(np.abs(lp - lp.mean(axis=1, keepdims=True) - ref_l).max()), float(np.abs(np.arctanh(v) - ref_z).max()))


def _record(**rec):
    print("FP16_RANGE " + json.dumps(rec))
    if os.environ.get("AO_PRECISION_REPORT"):
        with open(os.environ["AO_PRECISION_REPORT"], "a") as f:
            f.write(json.dumps(rec) + "\n")


IDS = [f.id for f in N.FAMILIES]


@pytest.mark.parametrize("kind", N.KINDS)
@pytest.mark.parametrize("fam", N.FAMILIES, ids=IDS)
def test_dead_channel_beyond_the_range_is_clamped_and_reported(fam, kind, monkeypatch):
    import torch
    pool = R.pool(fam.B)
    m = N.batch(fam)
    over, under = N.kinds_of_pool(fam.nb, fam.B, kind, fam.grid)
    assert over[m].any()
    x = torch.from_numpy(pool[m]).cuda()
    net = _net(fam, R.case_network(fam.nb, fam.B, 128, fam.grid), monkeypatch)
    try:
        _, _, st = _forward(net, fam, x)
        assert st == 0 and net.status() == 0, "the ordinary network reports an activation beyond the fp16 range"
        net.load_state_dict(N.big_network(fam.nb, fam.B, kind, fam.grid))
        assert net.status() == 0
        p, v, st = _forward(net, fam, x)
        assert st == 1, "%s: %d boards of the batch are beyond the range (%s), nothing reported" % (fam.kernel, over[m].sum(), kind)
        assert net.status() == 1 and net.status() == 0
        ref = N.dead_reference(fam.nb, fam.B, kind, fam.grid, fam.f16)
        ul, uz = N.unit(ref, m, fam.f16)
        el, ez = _errors(p, v, ref["logits"][m], ref["z"][m])
        _record(test="dead channel", id=fam.id, kernel=fam.kernel, kind=kind, boards=fam.batch, over=int(over[m].sum()), mult=fam.mult,
                unit="E_fast" if fam.f16 else "E32", unit_l=ul, unit_z=uz, err_l=el, err_z=ez, ratio_l=el / ul, ratio_z=ez / uz)
        assert el <= fam.mult * ul and ez <= fam.mult * uz, \
            "%s, %s: centred logits off by %.2f units (%.2e), atanh v by %.2f units (%.2e); allowed %d" % (
                fam.kernel, kind, el / ul, el, ez / uz, ez, fam.mult)
        if N.has_under(fam.B, kind):
            mu = N.under_batch(fam, kind)
            assert under[mu].all()
            p, v, st = _forward(net, fam, torch.from_numpy(pool[mu]).cuda())
            assert st == 0 and net.status() == 0, "%s, %s: a batch of boards that stay below 65504 / 2 raised the flag" % (fam.kernel, kind)
            ul, uz = N.unit(ref, mu, fam.f16)
            el, ez = _errors(p, v, ref["logits"][mu], ref["z"][mu])
            assert el <= fam.mult * ul and ez <= fam.mult * uz, (el / ul, ez / uz)
    finally:
        net.close()


@pytest.mark.parametrize("fam", N.FAMILIES, ids=IDS)
def test_one_activation_beyond_the_range_is_reported_wherever_it_sits(fam, monkeypatch):
    """The detector sweep: rows {0, 15, 16, last} x the four corners and the centre x channels {0, 15, 16, 77, 127}, in full up to
    2000 boards and the 20-point Latin-square-style subset of fp16_range_nets.sweep_points at 3073; 70000 must be reported,
    60000 must not and leaves the outputs within the ordinary bound. Every other board of the batch has an empty plane 0."""
    import torch
    B, base = fam.B, R.case_network(fam.nb, fam.B, 128, fam.grid)
    m = N.batch(fam)
    x = torch.from_numpy(N.quiet_pool(B)[m]).cuda()
    pts = N.sweep_points(B, fam.batch)
    net = _net(fam, base, monkeypatch)
    worst = [0.0, 0.0]
    missed, false_alarm = [], []
    try:
        for c in N.CHANNELS:
            mine = [(r, q) for r, q, cc in pts if cc == c]
            ref = N.detector_reference(fam.nb, B, fam.grid, c, fam.f16)
            for k in (N.DETECT_OVER, N.DETECT_IN):
                net.load_state_dict(N.stem_detector(base, c, k))
                if k == N.DETECT_OVER:
                    _, _, st = _forward(net, fam, x)
                    assert st == 0 and net.status() == 0, "channel %d: reported with no stone in plane 0 anywhere" % c
                for r, q in mine:
                    keep = x[r].clone()
                    x[r] = torch.from_numpy(N.detector_board(B, q)).cuda()
                    p, v, st = _forward(net, fam, x)
                    x[r] = keep
                    assert net.status() == st and net.status() == 0
                    if k == N.DETECT_OVER:
                        if st != 1:
                            missed.append((r, q, c))
                        continue
                    if st != 0:
                        false_alarm.append((r, q, c))
                    rb = N.detector_board_reference(fam.nb, B, fam.grid, c, q, fam.f16)
                    ref_l, ref_z = ref["logits"][m].copy(), ref["z"][m].copy()
                    ref_l[r], ref_z[r] = rb["logits"][0], rb["z"][0]
                    ul, uz = N.unit(ref, np.delete(m, r) if len(m) > 1 else m, fam.f16)
                    ul, uz = max(ul, float(rb["ul"][0])), max(uz, float(rb["uz"][0]))
                    el, ez = _errors(p, v, ref_l, ref_z)
                    worst = [max(worst[0], el / ul), max(worst[1], ez / uz)]
                    assert el <= fam.mult * ul and ez <= fam.mult * uz, ((r, q, c), el / ul, ez / uz)
    finally:
        net.close()
    _record(test="detector", id=fam.id, kernel=fam.kernel, boards=fam.batch, points=len(pts), mult=fam.mult, ratio_l=worst[0], ratio_z=worst[1],
            missed=missed, false_alarm=false_alarm)
    assert not missed, "%s: one activation of 70000 at (row, cell, channel) %s was not reported" % (fam.kernel, missed)
    assert not false_alarm, "%s: one activation of 60000 at (row, cell, channel) %s was reported" % (fam.kernel, false_alarm)


# (family of FAMILIES by id, boards of the first batch, boards of the second): the detector sits on the last row of the first
# batch; the second batch still reaches into that 16-board group (that board's workgroup round for k_boardh) but not to that row
DEAD_ROWS = [("conv_cells_h-B9-5", 5, 4), ("row16hk-B9-33", 35, 33), ("layer16hk-B9-760", 760, 753), ("layer16h-B9-70", 70, 66),
             ("trunk16h-B9-3073-fmt0", 3075, 3073), ("trunk16h-B9-3073-fmt1", 3075, 3073), ("boardh-B10-65", 66, 65),
             ("layer16h-B10-63", 63, 60), ("row16hk_w16-B9-33", 35, 33), ("layer16hk_w16-B9-760", 760, 753), ("layer16h_w16-B9-70", 70, 66),
             ("trunk16h_w16-B9-3073-fmt0", 3075, 3073), ("boardh_w16-B10-65", 66, 65), ("trunk16h_f16-B9-3073", 3075, 3073),
             ("boardh_f16-B10-65", 66, 65), ("layer16h_f16-B9-70", 70, 66), ("layer16h-B4-2000", 2000, 1986), ("trunk16h-B7-3073-fmt0", 3075, 3073)]


@pytest.mark.parametrize("fid,first,second", DEAD_ROWS, ids=[d[0] for d in DEAD_ROWS])
def test_a_row_that_is_no_longer_live_does_not_raise_the_flag(fid, first, second, monkeypatch):
    import torch
    fam = N.FAMILIES[IDS.index(fid)]
    assert second < first and (second - 1) // 16 == (first - 1) // 16 or fam.kernel.startswith(("k_boardh", "k_conv_cells"))
    B, base = fam.B, R.case_network(fam.nb, fam.B, 128, fam.grid)
    quiet = N.quiet_pool(B)
    ok = np.nonzero(N.fp16_planes(quiet))[0]
    x = quiet[ok[np.arange(first) % len(ok)]].copy()
    x[first - 1] = N.detector_board(B, B * B - 1)
    x = torch.from_numpy(x).cuda()
    net = _net(fam, N.stem_detector(base, N.CH, N.DETECT_OVER), monkeypatch)
    try:
        _, _, st = _forward(net, fam, x, first)
        assert st == 1 and net.status() == 1, "the detector board on the last live row was not reported"
        _, _, st = _forward(net, fam, x[:second], second)
        assert st == 0 and net.status() == 0, "%s: a row beyond the batch raised the flag" % fam.kernel
    finally:
        net.close()


@pytest.mark.parametrize("B", (4, 6, 8))
def test_three_byte_trunk_format_at_even_widths(B, monkeypatch):
    """AO_TRUNK_FMT=1 (fp16 high half + one low byte, 19 significand bits) at the even widths. The first run of the family tests
    above found every board of it wrong there, ordinary network included (|dp| 0.11 .. 0.25): the resident kernel toggles the
    row-buffer parity per layer for every format, and the 3-byte format, which stages its own row 0 into buffer 0, read the other.
    The bound is the project's contract on (p, v), 1e-4 against float64 (TOL of tests/test_gpu_net_precision.py), for the
    ordinary network and for the clamped dead channel; the logit-space figures are printed, not asserted: the format's error is
    2^-19 of an activation whatever the board, and on 4 x 4, where E32 sits at its floor, that is 17 .. 21 x E32 (4 .. 9 x at
    6 x 6, 8 x 8 and 9 x 9; the family test above holds 9 x 9 to 16 x). profiles/r31a_fp16_range_by_family.txt has the figures."""
    import torch
    fam = N.Family("trunk16h_fmt1", "k_trunk16h<%d, 4, 1>" % B, B, 3073, env={"AO_TRUNK_FMT": "1"})
    m = N.batch(fam)
    x = torch.from_numpy(R.pool(B)[m]).cuda()
    net = _net(fam, R.case_network(2, B, 128), monkeypatch)
    try:
        r64, r32 = R.pool_reference(2, B, 128)
        p, v, st = _forward(net, fam, x)
        assert st == 0 and net.status() == 0
        dp, dv = float(np.abs(p - r64["p"][m]).max()), float(np.abs(v - r64["v"][m]).max())
        el, ez = _errors(p, v, r64["logits"][m], r64["z"][m])
        ul, uz = R.units(2, B, 128, False, m)
        _record(test="3-byte format, even width", id=fam.id, kernel=fam.kernel, kind="ordinary", boards=fam.batch, dp=dp, dv=dv,
                unit="E32", unit_l=ul, unit_z=uz, err_l=el, err_z=ez, ratio_l=el / ul, ratio_z=ez / uz)
        assert dp < 1e-4 and dv < 1e-4, (dp, dv)
        net.load_state_dict(N.big_network(2, B, "inner"))
        p, v, st = _forward(net, fam, x)
        assert st == 1 and net.status() == 1 and net.status() == 0
        ref = N.dead_reference(2, B, "inner")
        e = np.exp(ref["logits"][m] - ref["logits"][m].max(axis=1, keepdims=True))
        dp, dv = float(np.abs(p - e / e.sum(axis=1, keepdims=True)).max()), float(np.abs(v - np.tanh(ref["z"][m])).max())
        el, ez = _errors(p, v, ref["logits"][m], ref["z"][m])
        ul, uz = N.unit(ref, m)
        _record(test="3-byte format, even width", id=fam.id, kernel=fam.kernel, kind="inner", boards=fam.batch, dp=dp, dv=dv,
                unit="E32", unit_l=ul, unit_z=uz, err_l=el, err_z=ez, ratio_l=el / ul, ratio_z=ez / uz)
        assert dp < 1e-4 and dv < 1e-4, (dp, dv)
        if N.has_under(B, "inner"):
            _, _, st = _forward(net, fam, torch.from_numpy(R.pool(B)[N.under_batch(fam, "inner")]).cuda())
            assert st == 0 and net.status() == 0
    finally:
        net.close()


@pytest.mark.parametrize("B,G,S,kernel", N.SEARCH_FAMILIES, ids=[s[3].split("<")[0] + "-G%d" % s[1] for s in N.SEARCH_FAMILIES])
def test_search_on_bit_planes_counts_one_event(B, G, S, kernel):
    """k_trunk16hb, k_boardh<B, 2> and the fused per-game step (k_conv_cells_h under a handful of games) read the tree kernel's
    bit planes: ao_search is their only entry point. One ordinary move names the kernel and raises nothing; the same move with
    the inner dead channel is repeated once, and the status word is clear afterwards."""
    from alpha_omok_amd.engine import Engine, Net
    nb = 2
    net = Net(nb, 5, 128, B, 0)
    eng = Engine(B, S, 5, games=G, noise=True)
    try:
        net.load_state_dict(R.case_network(nb, B, 128))
        eng.seed_all(np.arange(G, dtype=np.uint32) + 900)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            eng.search(net, tau=1)
        name = net.dominant_kernel(G)[0]
        assert name.startswith(kernel), (name, kernel)
        assert eng.fp16_range_events() == (0, 0) and net.status() == 0
        eng.reset()
        net.load_state_dict(N.big_network(nb, B, "inner"))
        with pytest.warns(RuntimeWarning, match="fp16 range") as rec:
            pi, vis, pol = eng.search(net, tau=1)
        assert len([w for w in rec if "fp16 range" in str(w.message)]) == 1
        assert eng.fp16_range_events() == (1, G)
        assert net.status() == 0 and net.get_mode() == 0
        assert np.all(vis.sum(axis=1) == S) and np.isfinite(pi).all() and np.isfinite(pol).all()
    finally:
        eng.close()
        net.close()


def test_the_fp16_range_families_cover_every_kernel_name():
    """(tests/test_fp16_range_host.py checks the same list against ao_net_plan_kernel on the CPU)"""
    have = {f.kernel for f in N.FAMILIES}
    assert set(N.NAMED) <= have and len(IDS) == len(set(IDS)) and {d[0] for d in DEAD_ROWS} <= set(IDS)
