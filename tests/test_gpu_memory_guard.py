"""-m gpu: stray writes, stray reads and stale reads of the library's own device memory, seen through the guarded allocation mode
(AO_POOL_GUARD / AO_POOL_FILL, csrc/pool_guard.hpp and host_handle.hpp; DESIGN.md "Guarded device allocations").

1. The mode itself: a guarded block is filled, a byte written into a guard -- inside the library's own allocation, so nothing
   faults -- is reported once with the block's size, the offset and the value, damage outlives the handle until it is
   reported, and without the variables nothing is guarded.
2. Workloads. Every scenario runs three times: plain, under 262144 guard bytes with fill 0xFF (NaN as float and fp16, -1 as
   int32) and with fill 0x5A (1.5e16 as float, 203.25 as fp16, a large positive int32: the split-fp16 epilogues turn NaN into 0,
   so NaN alone would hide a stale read there). 262144 bytes are more than one board's widest activation (15 x 15 x 128 planes
   x 4 B = 115 KB): a write to "row + 1" of any per-board layout lands in a guard. The three runs must agree bit for bit -- the
   plain run is the reference, the rest of the suite ties it to float64 and to the oracle -- and no guard may be damaged,
   neither while the handles live nor when they are freed.
"""
import ctypes as C

import numpy as np
import pytest

import net_reference as R
from test_pool_guard_host import parse_report

pytestmark = pytest.mark.gpu

GUARD = 262144
RUNS = (("plain", None, None), ("guard-ff", GUARD, 255), ("guard-5a", GUARD, 0x5A))


# ----------------------------------------------------------------------------------------------------------------------------
# plumbing
# ----------------------------------------------------------------------------------------------------------------------------
def _env(monkeypatch, guard, fill):
    if guard is None:
        monkeypatch.delenv("AO_POOL_GUARD", raising=False)
        monkeypatch.delenv("AO_POOL_FILL", raising=False)
    else:
        monkeypatch.setenv("AO_POOL_GUARD", str(guard))
        monkeypatch.setenv("AO_POOL_FILL", str(fill))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype.kind in "fc" else a


def _same_bits(ref, out, tag):
    assert sorted(ref) == sorted(out), tag
    for k in ref:
        a, b = np.asarray(ref[k]), np.asarray(out[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (tag, k, a.shape, b.shape, a.dtype, b.dtype)
        if not np.array_equal(_bits(a), _bits(b)):
            bad = np.flatnonzero((_bits(a) != _bits(b)).reshape(a.size, -1).any(axis=1) if a.size else [])
            raise AssertionError("%s: %s differs from the plain run in %d of %d elements, first at %d: %r against %r"
                                 % (tag, k, bad.size, a.size, bad[0], b.reshape(-1)[bad[0]], a.reshape(-1)[bad[0]]))


def three_runs(monkeypatch, scenario, *args):
    """scenario(guarded, *args) is a generator: it creates its handles, yields a dict of arrays while they are alive, and
    closes them when it is closed. Returns the plain run's dict."""
    from alpha_omok_amd.engine import guard_check
    ref = None
    for name, guard, fill in RUNS:
        _env(monkeypatch, guard, fill)
        gen = scenario(guard is not None, *args)
        try:
            out = next(gen)
            if guard is not None:
                blocks, damaged, msg = guard_check()
                assert blocks > 0, "%s: no guarded block" % name
                assert damaged == 0, "%s: %s" % (name, msg)
        finally:
            gen.close()
            _env(monkeypatch, None, None)
        blocks, damaged, msg = guard_check()
        assert damaged == 0, "%s, found when the handles were freed: %s" % (name, msg)
        if ref is None:
            ref = out
        else:
            _same_bits(ref, out, name)
    return ref


# ----------------------------------------------------------------------------------------------------------------------------
# 1. the mode itself
# ----------------------------------------------------------------------------------------------------------------------------
_HIP = []
H2D, D2H = 1, 2


def _hip():
    """The HIP runtime the library and torch already share, through ctypes."""
    if not _HIP:
        import torch  # noqa: F401
        from alpha_omok_amd import _lib
        _lib.load()
        with open("/proc/self/maps") as f:
            path = next(line.split()[-1] for line in f if "libamdhip64" in line)
        h = C.CDLL(path)
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        h.hipMemcpy.restype = C.c_int
        _HIP.append(h)
    return _HIP[0]


def _peek(ptr, n):
    buf = (C.c_uint8 * n)()
    assert _hip().hipMemcpy(buf, C.c_void_p(ptr), n, D2H) == 0
    return np.frombuffer(buf, np.uint8).copy()


def _poke(ptr, value):
    b = (C.c_uint8 * 1)(value)
    assert _hip().hipMemcpy(C.c_void_p(ptr), b, 1, H2D) == 0


def _live_blocks():
    from alpha_omok_amd.engine import guard_block
    out = []
    while True:
        b = guard_block(len(out))
        if b is None:
            return out
        out.append(b)


def _fresh_replay(monkeypatch, fill=0x5A):
    """A DeviceReplay created under guards and the largest of its blocks (pointer, bytes, guard bytes)."""
    from alpha_omok_amd.replay import DeviceReplay
    before = {b[0] for b in _live_blocks()}
    _env(monkeypatch, GUARD, fill)
    mem = DeviceReplay(9, 5, 64)
    _env(monkeypatch, None, None)
    mine = [b for b in _live_blocks() if b[0] not in before]
    assert mine and all(b[2] == GUARD and b[0] % 256 == 0 for b in mine)
    return mem, max(mine, key=lambda b: b[1])


def test_guard_size_is_rounded_up_and_the_fill_defaults_to_255(monkeypatch):
    from alpha_omok_amd.engine import guard_mode
    _env(monkeypatch, None, None)
    assert guard_mode() == (0, 255)
    for text, want in (("0", 0), ("1", 4096), ("4095", 4096), ("4096", 4096), ("4097", 8192), ("262144", 262144)):
        monkeypatch.setenv("AO_POOL_GUARD", text)
        assert guard_mode() == (want, 255), text
    monkeypatch.setenv("AO_POOL_FILL", "90")
    assert guard_mode() == (262144, 90)


def test_a_guarded_block_is_filled_and_clean(monkeypatch):
    from alpha_omok_amd.engine import guard_check
    mem, (ptr, nbytes, guard) = _fresh_replay(monkeypatch)
    try:
        blocks, damaged, msg = guard_check()
        assert blocks > 0 and damaged == 0 and msg == "", (blocks, damaged, msg)
        assert nbytes == 64 * 5 * 81 * 4                       # the state ring: capacity x planes x cells floats
        assert (_peek(ptr, 64) == 0x5A).all()
        assert (_peek(ptr - 64, 64) == 0x5A).all() and (_peek(ptr + nbytes, 64) == 0x5A).all()
    finally:
        mem.close()
    assert guard_check()[1] == 0


@pytest.mark.parametrize("place", ("first byte after the block", "last byte of the rear guard", "a byte of the front guard"))
def test_one_byte_in_a_guard_is_reported_once(monkeypatch, place):
    from alpha_omok_amd.engine import guard_check
    mem, (ptr, nbytes, guard) = _fresh_replay(monkeypatch)
    try:
        assert guard_check()[1] == 0
        addr, side, off = {"first byte after the block": (ptr + nbytes, "end", 0),
                           "last byte of the rear guard": (ptr + nbytes + guard - 1, "end", guard - 1),
                           "a byte of the front guard": (ptr - 7, "start", 7)}[place]
        _poke(addr, 0x11)                                       # inside the library's own allocation
        blocks, damaged, msg = guard_check()
        assert blocks > 0 and damaged == 1, (damaged, msg)
        r = parse_report(msg)
        assert (r["bytes"], r["count"], r["side"], r["offset"], r["value"], r["fill"], r["freed"]) == (nbytes, 1, side, off, 0x11, 0x5A, False), msg
        assert guard_check()[1:] == (0, "")                     # reported once
        assert (_peek(addr, 1) == 0x5A).all()                   # ... and the guard is whole again
    finally:
        mem.close()
    assert guard_check()[1] == 0


def test_damage_outlives_the_handle_until_it_is_reported(monkeypatch):
    from alpha_omok_amd.engine import guard_check
    before = guard_check()[0]
    mem, (ptr, nbytes, guard) = _fresh_replay(monkeypatch, fill=255)
    _poke(ptr - 1, 0)
    mem.close()
    blocks, damaged, msg = guard_check()
    assert blocks == before and damaged == 1, (blocks, damaged, msg)
    r = parse_report(msg)
    assert (r["bytes"], r["count"], r["side"], r["offset"], r["value"], r["fill"], r["freed"]) == (nbytes, 1, "start", 1, 0, 255, True), msg
    assert guard_check() == (before, 0, "")


def test_without_the_variables_nothing_is_guarded(monkeypatch):
    from alpha_omok_amd.engine import Engine, Net, guard_check
    from alpha_omok_amd.positions import PositionBatch
    from alpha_omok_amd.replay import DeviceReplay
    from alpha_omok_amd.rollout import RolloutEngine
    from alpha_omok_amd.tictactoe import TttEngine
    _env(monkeypatch, None, None)
    before = guard_check()[0]
    hs = [DeviceReplay(9, 5, 64), Engine(9, 8, 5, games=2, node_cap=64), Net(1, 5, 32, 9, 0), RolloutEngine(9, 8, 0, games=2),
          TttEngine(8, games=2), PositionBatch(9, capacity=4)]
    assert guard_check()[0] == before
    monkeypatch.setenv("AO_POOL_GUARD", "0")
    hs.append(DeviceReplay(9, 5, 64))
    assert guard_check()[0] == before
    for h in hs:
        h.close()


def test_every_handle_type_is_guarded(monkeypatch):
    from alpha_omok_amd.engine import Engine, Net, guard_check
    from alpha_omok_amd.positions import PositionBatch
    from alpha_omok_amd.replay import DeviceReplay
    from alpha_omok_amd.rollout import RolloutEngine
    from alpha_omok_amd.tictactoe import TttEngine
    makers = (lambda: DeviceReplay(9, 5, 64), lambda: Engine(9, 8, 5, games=2, node_cap=64), lambda: _search_net(1, 5, 9),             # (a Net allocates with its parameters, not at create)
              lambda: RolloutEngine(9, 8, 0, games=2), lambda: TttEngine(8, games=2), lambda: PositionBatch(9, capacity=4))
    for make in makers:
        before = guard_check()[0]
        _env(monkeypatch, 4096, 255)
        h = make()
        _env(monkeypatch, None, None)
        assert guard_check()[0] > before
        h.close()
        assert guard_check()[:2] == (before, 0)


# ----------------------------------------------------------------------------------------------------------------------------
# 2a. forward: one case per kernel name
# ----------------------------------------------------------------------------------------------------------------------------
def _by_kernel():
    best = {}
    for c in R.CASES:
        if c.kernel not in best or c.batch * max(c.nb, 1) < best[c.kernel].batch * max(best[c.kernel].nb, 1):
            best[c.kernel] = c
    return list(best.values())


KERNEL_CASES = _by_kernel()


def _make_net(case, monkeypatch):
    """As tests/test_gpu_net_precision.py creates its nets: environment, padding, mode."""
    from alpha_omok_amd.engine import Net
    from alpha_omok_amd.pvnet import native_width, pad_state_dict
    sd = R.case_network(*case.net_key())
    width = native_width(case.planes)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    net = Net(case.nb, case.C, width, case.B, 0)
    for k in case.env:
        monkeypatch.delenv(k)
    net.load_state_dict(sd if width == case.planes else pad_state_dict(sd, width))
    net.set_mode(case.mode)
    return net, width


def _run(net, x, out, tag):
    import torch
    p, v = net(x)
    torch.cuda.synchronize()
    out[tag + "p"], out[tag + "v"] = p.cpu().numpy(), v.cpu().numpy()
    out[tag + "status"] = np.array([net.status()], np.int32)


def _forward_scenario(guarded, case, monkeypatch):
    import torch
    from alpha_omok_amd.engine import plan_kernel
    net, width = _make_net(case, monkeypatch)
    try:
        out = {}
        pool = R.pool(case.B, case.C)
        _run(net, torch.from_numpy(pool[case.boards()]).cuda(), out, "")
        name = net.dominant_kernel(case.batch)[0]
        assert name.startswith(case.kernel), (name, case.kernel)
        if case.batch % 16 == 0:            # a ragged last group, where the same kernel still carries it
            planned = plan_kernel(case.nb, case.C, width, case.B, case.batch + 1, in_kind=1, trunk_mode=case.mode)[0]
            if planned.startswith(case.kernel.replace("_w16<", "<")) or net.dominant_kernel(case.batch + 1)[0].startswith(case.kernel):
                _run(net, torch.from_numpy(pool[R.batch_indices(case.batch + 1, case.B, case.C)]).cuda(), out, "ragged ")
        yield out
    finally:
        net.close()


@pytest.mark.parametrize("case", KERNEL_CASES, ids=[c.kernel.replace(" ", "") for c in KERNEL_CASES])
def test_forward_of_every_kernel_name(case, monkeypatch):
    out = three_runs(monkeypatch, _forward_scenario, case, monkeypatch)
    assert np.isfinite(out["p"]).all() and np.isfinite(out["v"]).all()


def test_the_forward_cases_cover_every_kernel_name():
    assert {c.kernel for c in KERNEL_CASES} == {c.kernel for c in R.CASES} and len(KERNEL_CASES) >= 103
    assert "k_conv3x3<3>" in {c.kernel for c in KERNEL_CASES} and "k_trunk16h_w16<9, 4, 0>" in {c.kernel for c in KERNEL_CASES}


# the one-product kernels: the smallest batches of test_gpu_fp16_forward.py / test_gpu_fp16_all.py that reach each name
F16_CASES = [("fp16", 0, nb, B, n, "k_trunk16h_f16<%d, 4, 0>" % B) for nb, B, n in [(2, 9, 3073), (1, 7, 3104), (2, 4, 3073), (1, 3, 3072)]] + \
            [("fp16", 0, nb, B, n, "k_boardh_f16<%d, 1>" % B) for nb, B, n in [(2, 15, 65), (2, 10, 64), (1, 12, 65)]] + \
            [("fp16-all", 6, nb, B, n, "k_layer16h_f16<%d>" % B) for nb, B, n in [(2, 9, 17), (1, 7, 33), (2, 4, 17), (1, 3, 16), (2, 15, 17),
                                                                                   (2, 10, 33), (1, 12, 17)]]


def _f16_scenario(guarded, precision, mode, nb, B, batch, kernel):
    import torch
    import fp16_all_batches as fb
    import fp16_forward_nets as fn
    from alpha_omok_amd.engine import Net
    net = Net(nb, 5, 128, B, 0)
    try:
        net.set_mode(mode)
        net.load_state_dict(fn.exact_network(nb, B))
        assert net.precision(precision) == precision
        idx = fb.batch_of(B, batch) if precision == "fp16-all" else fn.batch_of(B, batch)
        out = {}
        _run(net, torch.from_numpy(fn.binary_pool(B)[idx]).cuda(), out, "")
        name = net.dominant_kernel(batch)[0]
        assert name.startswith(kernel), (name, kernel)
        yield out
    finally:
        net.close()


@pytest.mark.parametrize("precision,mode,nb,B,batch,kernel", F16_CASES, ids=[c[5].replace(" ", "") for c in F16_CASES])
def test_forward_of_every_one_product_kernel_name(precision, mode, nb, B, batch, kernel, monkeypatch):
    three_runs(monkeypatch, _f16_scenario, precision, mode, nb, B, batch, kernel)


# ----------------------------------------------------------------------------------------------------------------------------
# 2b. workspace reuse: a larger batch of other boards first, on the same net
# ----------------------------------------------------------------------------------------------------------------------------
FAMILY_KERNELS = ("k_conv_cells_h<9, 8>", "k_row16hk<9>", "k_layer16hk<9, 4>", "k_layer16h<9>", "k_trunk16h<9, 4, 0>", "k_boardh<10, 1>",
                  "k_layer16<9>", "k_trunk16<9>")
FAMILY_CASES = [c for c in KERNEL_CASES if c.kernel in FAMILY_KERNELS]


def _reuse_scenario(guarded, case, monkeypatch):
    import torch
    net, _ = _make_net(case, monkeypatch)
    try:
        pool = R.pool(case.B, case.C)
        if guarded:
            larger = case.batch + 37 if case.batch >= 1024 else 2 * case.batch + 5
            other = torch.from_numpy(pool[R.batch_indices(larger, case.B, case.C, seed=1)]).cuda()
            net(other)
            torch.cuda.synchronize()
        out = {}
        _run(net, torch.from_numpy(pool[case.boards()]).cuda(), out, "")
        assert net.dominant_kernel(case.batch)[0].startswith(case.kernel)
        yield out
    finally:
        net.close()


@pytest.mark.parametrize("case", FAMILY_CASES, ids=[c.kernel.replace(" ", "") for c in FAMILY_CASES])
def test_forward_after_a_larger_batch_on_the_same_net(case, monkeypatch):
    assert len(FAMILY_CASES) == len(FAMILY_KERNELS)
    three_runs(monkeypatch, _reuse_scenario, case, monkeypatch)


# ----------------------------------------------------------------------------------------------------------------------------
# 2c. search
# ----------------------------------------------------------------------------------------------------------------------------
def _streams(eng):
    from test_gpu_rolling import _streams as streams
    return streams(eng)


def _search_net(nb, C, B):
    import pvnet_weights
    from alpha_omok_amd.engine import Net
    net = Net(nb, C, 128, B, 0)
    net.load_state_dict(pvnet_weights.make_state_dict(nb, C, 128, B, 7))
    return net


def _read_trees(eng, out, tag, games):
    """lookup of the roots and of each root's first child, PV lines and stats of the listed games"""
    mask = np.zeros(eng.G, np.uint8)
    mask[games] = 1
    roots = [(0,) + tuple(eng.get_moves(g)) for g in games]
    look = eng.tree_lookup(roots, games)
    kids = [r + (int(look["child_action"][i, 0]),) if look["nchild"][i] > 0 else r for i, r in enumerate(roots)]
    look2 = eng.tree_lookup(kids, games)
    for k, v in look.items():
        out[tag + "lookup " + k] = v
    for k, v in look2.items():
        out[tag + "lookup child " + k] = v
    for k, v in eng.principal_variations(8, mask).items():
        out[tag + "pv " + k] = v
    for k, v in eng.tree_stats(mask).items():
        out[tag + "stats " + k] = v


def _plies(eng, net, out, plies=3, sample=None, **kw):
    G = eng.G
    sample = list(range(min(G, 8))) if sample is None else sample
    for t in range(plies):
        pi, vis, pol = eng.search(net, tau=np.ones(G, np.int8), **kw)
        for g in sample:
            for k, v in eng.root_children(g).items():
                out["ply %d game %d child %s" % (t, g, k)] = v
        if t == plies - 1:
            _read_trees(eng, out, "ply %d " % t, sample)
        act, win = eng.play()
        out.update({"ply %d pi" % t: pi, "ply %d visits" % t: vis, "ply %d priors" % t: pol, "ply %d action" % t: act, "ply %d win" % t: win})
    out["mt"], out["mt pos"] = _streams(eng)


def _search_scenario(guarded, B, G, S, nb, Cn):
    from alpha_omok_amd.engine import Engine
    net = _search_net(nb, Cn, B)
    eng = Engine(B, S, Cn, games=G, noise=True, node_cap=4 * (S + 1))
    try:
        eng.seed_all(np.arange(3100, 3100 + G, dtype=np.uint32))
        out = {}
        _plies(eng, net, out)
        assert net.status() == 0
        yield out
    finally:
        eng.close()
        net.close()


@pytest.mark.parametrize("B,G,S,nb,Cn", [(9, 5, 48, 2, 5), (9, 64, 24, 2, 5), (15, 3, 24, 1, 5), (5, 7, 20, 1, 3), (9, 3072, 12, 1, 5)])
def test_search_three_plies_with_noise(B, G, S, nb, Cn, monkeypatch):
    out = three_runs(monkeypatch, _search_scenario, B, G, S, nb, Cn)
    assert (out["ply 0 visits"].sum(axis=1) == S).all()


def _stepwise_scenario(guarded, B, G, S, oracle):
    from alpha_omok_amd.engine import Engine
    from gpu_helpers import HostEvalRunner
    eng = Engine(B, S, 5, games=G, noise=True, node_cap=4 * (S + 1))
    try:
        eng.seed_all(np.arange(500, 500 + G, dtype=np.uint32))
        run = HostEvalRunner(eng)
        out = {}
        for t in range(3):
            pi, vis, pol = run.move(lambda g, sim, pl: oracle.stub_eval(pl, 0), tau=np.ones(G, np.int8))
            for g in range(G):
                for k, v in eng.root_children(g).items():
                    out["ply %d game %d child %s" % (t, g, k)] = v
            act, win = eng.play()
            out.update({"ply %d pi" % t: pi, "ply %d visits" % t: vis, "ply %d priors" % t: pol, "ply %d action" % t: act, "ply %d win" % t: win,
                        "ply %d planes" % t: run.planes.cpu().numpy()})
        out["mt"], out["mt pos"] = _streams(eng)
        yield out
    finally:
        eng.close()


@pytest.mark.parametrize("B,G,S", [(9, 5, 24), (15, 3, 24)])
def test_stepwise_search_with_the_oracle_stub(B, G, S, oracle, monkeypatch):
    three_runs(monkeypatch, _stepwise_scenario, B, G, S, oracle)


def _feature_scenario(guarded, feature):
    """One feature of the search each, on the trained 2-block 9x9 network and the openings of its own GPU test."""
    from alpha_omok_amd.engine import Engine, Net
    from test_gpu_fused_parity import _trained_state_dict
    from test_gpu_search_early_stop import BUDGETS, OPENINGS, SEEDS
    G, S = 8, 40
    net = Net(2, 5, 128, 9, 0)
    eng = Engine(9, S, 5, games=G, noise=True, node_cap=4 * (S + 1))
    other = None
    try:
        net.load_state_dict(_trained_state_dict())
        eng.seed_all(SEEDS)
        out = {}
        if feature == "root tactics":
            # black has an open three-and-one: a forced win for the mover in games 0..3, a threat to answer in games 4..7
            four = (0, 37, 0, 38, 8, 39, 72)
            assert (eng.set_roots([four if g < 4 else four + (80,) for g in range(G)]) == 0).all()
        else:
            assert (eng.set_roots(OPENINGS) == 0).all()
        if feature == "leaf symmetry":
            eng.set_leaf_symmetry(0x5EED1234)
            _plies(eng, net, out, 2)
        elif feature == "root tactics":
            pi, vis, pol = eng.search(net, tau=np.zeros(G, np.int8), tactics=dict(max_depth=6, max_nodes=512, solved_sims=4))
            out.update(pi=pi, visits=vis, priors=pol, **{"tactics " + k: np.asarray(v) for k, v in eng.last_tactics().items()})
            out["action"], out["win"] = eng.play()
        elif feature == "early stop":
            for t, every in enumerate((8, 1)):
                pi, vis, pol = eng.search(net, tau=np.zeros(G, np.int8), early_stop=True, settle_every=every)
                ran = eng.sims_run()
                act, win = eng.play()
                out.update({"ply %d pi" % t: pi, "ply %d visits" % t: vis, "ply %d priors" % t: pol, "ply %d action" % t: act,
                            "ply %d sims" % t: ran["sims"], "ply %d settled" % t: ran["settled"]})
        elif feature == "budgets":
            _plies(eng, net, out, 2, sims=BUDGETS, noise=np.arange(G) % 2 == 0)
        elif feature == "rolling with a refill":
            _rolling(eng, net, out)
        elif feature == "export and import":
            _plies(eng, net, out, 2)
            snap = eng.export_trees()
            for k in ("hdr", "gauss", "mt", "moves", "nchild", "parent", "parent_edge", "act", "n", "w", "q", "p", "child"):
                out["snapshot " + k] = getattr(snap, k)
            other = Engine(9, S, 5, games=G, noise=True, node_cap=4 * (S + 1))      # guarded like the first
            other.import_trees(snap)
            pi, vis, pol = other.search(net, tau=np.ones(G, np.int8))
            out.update({"resumed pi": pi, "resumed visits": vis, "resumed priors": pol})
            _read_trees(other, out, "resumed ", list(range(G)))
            out["resumed action"], out["resumed win"] = other.play()
            out["resumed mt"], out["resumed mt pos"] = _streams(other)
        out["mt"], out["mt pos"] = _streams(eng)
        yield out
    finally:
        if other is not None:
            other.close()
        eng.close()
        net.close()


def _rolling(eng, net, out):
    """8 games, tau 0; the first three start one move from a win, end, and their slots are refilled while the others go on
    (the protocol of test_gpu_leaf_symmetry.test_rolling_search_with_refills_equals_search_and_play). A game's records do
    not depend on the return order, so they are kept per slot and episode."""
    G = eng.G
    four = (0, 37, 0, 38, 8, 39, 72, 40, 80)
    eng.reset()
    assert (eng.set_roots([four if g < 3 else (0,) for g in range(G)]) == 0).all()
    net.set_mode(6)
    eng.roll_begin(net, tau_plies=0, visit=True, policy=True, turn_every=2)
    recs, refills, next_seed, drained = {g: [] for g in range(G)}, 0, 9100, False
    for _ in range(10000):
        r = eng.roll_run()
        refill = []
        for b in range(len(r["game"])):
            g = int(r["game"][b])
            recs[g].append({k: r[k][b] for k in r})
            if r["win"][b] != 0 and not drained:
                refill.append(g)
        if refill:
            refill.sort()
            mask = np.zeros(G, np.uint8)
            mask[refill] = 1
            eng.reset(mask)
            eng.seed_games(refill, [next_seed + g for g in refill])     # by slot: independent of which launch ended the game
            refills += len(refill)
            eng.roll_join(active=mask, tau_plies=0)
        if not drained and all(len(v) >= 3 for v in recs.values()):
            eng.roll_drain()
            drained = True
        if drained and len(r["game"]) == 0:
            break
    else:
        raise AssertionError("the roll did not run dry")
    eng.roll_end()
    assert refills >= 1
    for g, rows in recs.items():
        for k in ("ply", "action", "win", "tau", "sims", "settled", "pi", "visit", "policy"):
            out["roll game %d %s" % (g, k)] = np.stack([np.asarray(r[k]) for r in rows])


@pytest.mark.parametrize("feature", ("leaf symmetry", "root tactics", "early stop", "budgets", "rolling with a refill", "export and import"))
def test_search_features(feature, monkeypatch):
    three_runs(monkeypatch, _feature_scenario, feature)


# ----------------------------------------------------------------------------------------------------------------------------
# 2d. PositionBatch
# ----------------------------------------------------------------------------------------------------------------------------
def _position_ids(B, rs):
    A = B * B
    ids = []
    for k in range(17):
        n = int(rs.randint(0, A + 1)) if k else A        # a board played full first
        ids.append((0,) + tuple(int(m) for m in rs.permutation(A)[:n]))
    ids.append((0, 0, A))                                # a move off the board
    ids.append((0, 1, 2, 1))                             # an occupied cell
    ids.append((0,) + tuple(range(A)) + (0,))            # more moves than cells
    ids.append((0,))
    return ids


def _positions_scenario(guarded, B):
    import pvnet_weights
    from alpha_omok_amd.engine import Net
    from alpha_omok_amd.positions import PositionBatch
    rs = np.random.RandomState(40 + B)
    ids = _position_ids(B, rs)
    boards = rs.randint(-1, 2, size=(20, B, B)).astype(np.int8)
    net = Net(1, 5, 128, B, 0)
    pb = PositionBatch(B, capacity=7)
    pb16 = PositionBatch(B, capacity=16)
    try:
        net.load_state_dict(pvnet_weights.make_state_dict(1, 5, 128, B, 7))
        out = {"check_win": pb.check_win(boards)}
        out.update({"describe " + k: v for k, v in pb.describe(ids).items()})
        out["planes"] = pb.planes(ids).cpu().numpy()
        for tag, res in (("evaluate", pb.evaluate(net, ids)), ("evaluate sym", pb16.evaluate(net, ids, symmetries=8))):
            out.update({"%s %d" % (tag, i): a for i, a in enumerate(res)})
        for tag, res in (("win_cells", pb.win_cells(ids)), ("audit", pb.audit(ids)), ("forced_wins", pb.forced_wins(ids, 4, 200)),
                         ("forced_defences", pb.forced_defences(ids, 3, 60))):
            out.update({tag + " " + k: v for k, v in res.items()})
        yield out
    finally:
        pb.close()
        pb16.close()
        net.close()


@pytest.mark.parametrize("B", (3, 9, 15))
def test_position_batch(B, monkeypatch):
    out = three_runs(monkeypatch, _positions_scenario, B)
    assert sorted(set(out["describe err"].tolist())) == [0, 1, 2, 3]


# ----------------------------------------------------------------------------------------------------------------------------
# 2e. DeviceReplay
# ----------------------------------------------------------------------------------------------------------------------------
def _dump(mem, out, tag):
    s, pi, z = mem.read(0, len(mem))
    out.update({tag + " states": s, tag + " pi": pi, tag + " z": z, tag + " len": np.array([len(mem)])})
    idx = np.random.RandomState(len(mem)).randint(0, len(mem), size=19)
    for k, t in zip(("states", "pi", "z"), mem.batch(idx)):
        out["%s batch %s" % (tag, k)] = t.cpu().numpy()
    snap = mem.export_snapshot()
    for k in ("kind", "z", "bits", "pi_mask", "pi_val", "raw"):
        out["%s snapshot %s" % (tag, k)] = getattr(snap, k)
    return snap


def _replay_scenario(guarded, kind, shape):
    from alpha_omok_amd.replay import DeviceReplay
    from test_gpu_replay import _samples
    mems, out = [], {}
    try:
        if kind == "samples":
            B, cap = shape
            rs = np.random.RandomState(B * 1000 + cap)
            mem = DeviceReplay(B, 5, cap)
            mems.append(mem)
            for n in (3, 1, 7, 0, 11, 2):                                  # through wraps
                mem.extend_augmented(_samples(rs, n, B))
            mem.extend(_samples(rs, 5, B))
        elif kind == "arrays":
            B, cap, n = shape
            rs = np.random.RandomState(cap + n)
            mem = DeviceReplay(B, 5, cap)
            mems.append(mem)
            for k in (3, n, 2, n):                                         # n alone overfills: the skip path
                smp = _samples(rs, k, B)
                mem.extend_augmented_arrays(np.stack([m[0] for m in smp]), np.stack([m[1] for m in smp]), np.array([m[2] for m in smp]))
        else:
            B, Cn, cap, E = shape
            A = B * B
            rs = np.random.RandomState(B * 100 + Cn)
            mem = DeviceReplay(B, Cn, cap)
            mems.append(mem)
            for rnd in range(2):
                lens = rs.randint(1, A + 1, E)
                lens[0] = A
                moves = np.full((E, A), -1, np.int32)
                for e in range(E):
                    moves[e, :lens[e]] = rs.permutation(A)[:lens[e]]
                ep_of = np.repeat(np.arange(E), lens)
                ply_of = np.concatenate([np.arange(n) for n in lens])
                mem.extend_augmented_moves(moves, ep_of, ply_of, rs.dirichlet(np.ones(A), ep_of.size), rs.choice([-1.0, 0.0, 1.0], ep_of.size))
        snap = _dump(mem, out, "memory")
        twin = DeviceReplay(mem.B, mem.C, mem.maxlen + 3)                  # the snapshot into a second guarded memory
        mems.append(twin)
        twin.import_snapshot(snap)
        _dump(twin, out, "imported")
        yield out
    finally:
        for m in mems:
            m.close()


@pytest.mark.parametrize("kind,shape", [("samples", (15, 37)), ("samples", (3, 8)), ("arrays", (9, 97, 13)), ("moves", (13, 5, 600, 8))])
def test_device_replay(kind, shape, monkeypatch):
    three_runs(monkeypatch, _replay_scenario, kind, shape)


# ----------------------------------------------------------------------------------------------------------------------------
# 2f. rollout agents
# ----------------------------------------------------------------------------------------------------------------------------
def _rollout_scenario(guarded, mode):
    from alpha_omok_amd.rollout import RolloutEngine
    G = 4
    eng = RolloutEngine(9, 40, mode, games=G)
    try:
        roots = [(0,), (0, 40), (0, 40, 41, 31), (0, 3, 77, 12, 60, 44)]
        out = {}
        for g in range(G):
            eng.seed(g, 1000 + g)
        for step in range(2):
            pi, stat, act = eng.search(roots)
            out.update({"step %d pi" % step: pi, "step %d stat" % step: stat, "step %d action" % step: act})
            roots = [r + (int(a),) for r, a in zip(roots, act)]
        st = [eng.get_rng_state(g) for g in range(G)]
        out["mt"], out["mt pos"] = np.stack([s[0] for s in st]), np.array([s[1] for s in st])
        yield out
    finally:
        eng.close()


@pytest.mark.parametrize("mode", (0, 1))
def test_rollout_engine(mode, monkeypatch):
    three_runs(monkeypatch, _rollout_scenario, mode)


def _ttt_scenario(guarded):
    from alpha_omok_amd.tictactoe import TttEngine
    G = 8
    eng = TttEngine(200, games=G, board_size=3)
    try:
        rs = np.random.RandomState(12)
        boards = np.zeros((G, 3, 3), np.int8)
        turns = np.zeros(G, np.int32)
        for g in range(1, G):                         # game 0: the empty board; the others: one or two stones each
            cells = rs.permutation(9)[:1 + g % 2]
            boards[g].reshape(-1)[cells[0]] = 1
            if len(cells) > 1:
                boards[g].reshape(-1)[cells[1]] = -1
            turns[g] = len(cells) % 2
        for g in range(G):
            eng.seed(g, 70 + g)
        act, q, n = eng.search(boards, turns)
        st = [eng.get_rng_state(g) for g in range(G)]
        yield {"action": act, "q": q, "n": n, "mt": np.stack([s[0] for s in st]), "mt pos": np.array([s[1] for s in st])}
    finally:
        eng.close()


def test_ttt_engine(monkeypatch):
    three_runs(monkeypatch, _ttt_scenario)
