"""No GPU, no compiled library: the float64 reference of tests/net_reference.py checks itself, every network and batch of
tests/test_gpu_net_precision.py is shown to be a case on which an error can be seen, and a catalogue of small defects,
applied to the float64 reference, is shown to pass the bound of every such case at least twice over. The cases run every
number of conv1 input planes of net_reference.INPLANES beside 5; the catalogue's conv1 defects act per input plane.

The saturation of the golden-vector weights that made this necessary (float64, the batches of
test_gpu_net.test_forward_vs_torch_fp32; `net_reference.saturation_table()`):

    (nb, B, planes, batch)   distinct v    1 - |v|                        share of p < 1e-6   median max p
    (4, 9, 128, 70)          1 of 70       0.83 (value ReLU passes 0 %)   0.50                0.73
    (10, 9, 128, 33)         1 of 33       <= 1.9e-8 (tanh saturated)     0.75                0.85
    (1, 3, 128, 3)           2 of 3        --                             0                   0.69
    (3, 9, 64, 32)           32 of 32      down to 1.1e-3                 0.18                0.96
    the other four           all distinct  healthy                        0                   0.07 .. 0.14
"""
import numpy as np
import pytest

import net_reference as R
import pvnet_weights


def _module(sd, nb, planes, B):
    import torch
    from alpha_omok_amd.pvnet import PVNet
    m = PVNet(nb, 5, planes, B)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.eval().double()


@pytest.mark.parametrize("conditioned", [False, True])
@pytest.mark.parametrize("nb,B,planes", [(4, 9, 128), (10, 9, 128), (2, 15, 128), (3, 9, 64), (1, 3, 32), (2, 7, 96), (0, 5, 32)])
def test_reference_is_the_torch_module_in_float64(nb, B, planes, conditioned):
    """conv2d + affine BatchNorm + ReLU + matmul, written out, against alpha_omok_amd.pvnet.PVNet(...).double(): (p, v) within
    1e-12, on the boards of the pool (structured and float-plane boards included)."""
    import torch
    sd = R.conditioned_state_dict(nb, 5, planes, B, 11) if conditioned else pvnet_weights.make_state_dict(nb, 5, planes, B, 11)
    x = R.pool(B)[:24]
    o = R.forward(sd, x)
    with torch.no_grad():
        p, v = _module(sd, nb, planes, B)(torch.from_numpy(np.array(x)).double())
    assert (torch.softmax(o["logits"], dim=1) - p).abs().max().item() <= 1e-12
    assert (torch.tanh(o["z"]) - v).abs().max().item() <= 1e-12
    # the partial evaluations used by the defect catalogue are the same function
    o2 = R.forward(sd, x, resume=o["last_in"])
    o3 = R.forward(sd, x, trunk=o["trunk"])
    for k in ("logits", "z"):
        assert torch.equal(o[k], o2[k]) and torch.equal(o[k], o3[k])
    assert o["trunk"].shape == (24, planes, B, B) and o["hp"].shape == (24, 2 * B * B) and o["hv"].shape == (24, B * B)


def test_golden_vector_weights_hide_the_value_head():
    """The reason for the second generator, kept as an assertion: on the two 9x9 / 128-plane batches of
    test_forward_vs_torch_fp32 make_state_dict's value head is dead (its ReLU passes nothing at 4 blocks, its tanh is saturated at 10): v is one number
    for the whole batch, whatever the trunk returns."""
    rows = {r["case"]: r for r in R.saturation_table()}
    for case in ((4, 9, 128, 70), (10, 9, 128, 33)):
        assert rows[case]["distinct_v"] == 1 and rows[case]["share_p_below_1e6"] >= 0.45, rows[case]
    assert rows[(4, 9, 128, 70)]["hv_live"] == 0.0                   # the value head's ReLU passes nothing
    assert rows[(10, 9, 128, 33)]["one_minus_absv_max"] < 1e-7       # the tanh is saturated
    assert rows[(3, 9, 64, 32)]["median_max_p"] > 0.9
    for case in ((2, 15, 128, 40), (1, 3, 32, 5), (2, 7, 96, 64), (2, 7, 128, 20)):
        assert rows[case]["distinct_v"] == case[3] and rows[case]["share_p_below_1e6"] == 0.0


def test_conditioned_generator_keeps_the_wire_format_and_is_deterministic():
    a = R.conditioned_state_dict(2, 5, 128, 9, 3)
    b = R.conditioned_state_dict(2, 5, 128, 9, 3)
    base = pvnet_weights.make_state_dict(2, 5, 128, 9, 3)
    assert list(a) == list(base)
    for k in base:
        assert a[k].shape == base[k].shape and a[k].dtype == base[k].dtype, k
        assert np.array_equal(a[k], b[k]), k
    for k in base:                                           # the trunk is make_state_dict's but for the scaled second BatchNorms
        if "head" not in k and ".bn2." not in k:
            assert np.array_equal(a[k], base[k]), k
    g = R.conditioned_state_dict(2, 5, 128, 9, 3, grid=True)
    for k, v in g.items():
        if v.ndim == 4 and v.shape[2] == 3:
            assert np.array_equal(v.astype(np.float16).astype(np.float32), v) and not np.array_equal(v, a[k]), k


NETS = sorted({c.net_key() for c in R.CASES})


@pytest.mark.parametrize("nb,B,planes,grid,C", NETS, ids=["nb%d-B%d-p%d-%s%s" % (k[0], k[1], k[2], "w16grid" if k[3] else "w32",
                                                                                "" if k[4] == 5 else "-C%d" % k[4]) for k in NETS])
def test_every_network_of_the_gpu_cases_is_conditioned(nb, B, planes, grid, C):
    """The conditions under which a forward error is visible, asserted on the float64 reference alone, on the pool every
    batch of that network is drawn from."""
    sd = R.case_network(nb, B, planes, grid, C)
    assert sd["conv1.weight"].shape == (planes, C, 3, 3)
    r = R.conditioning_report(sd, R.pool(B, C))
    assert 0.3 <= r["trunk_rms"] <= 4.0 and r["trunk_max"] < 100.0, r          # nowhere near the fp16 range
    assert 1.0 <= r["logit_std"] <= 1.6 and r["p_min"] >= 1e-8, r              # log p of an fp32 p is well conditioned
    assert r["z_absmax"] <= 1.5 and r["z_std"] >= 0.3, r                       # atanh of an fp32 v costs at most ~3e-7
    assert 0.4 <= r["hp_live"] <= 0.8 and 0.4 <= r["hv_live"] <= 0.8 and 0.3 <= r["h1_live"] <= 0.7, r
    for i in range(nb):                                                        # the BatchNorm fold is part of what is tested
        for bn in ("layers.%d.bn1" % i, "layers.%d.bn2" % i):
            for f in ("weight", "bias", "running_mean", "running_var"):
                a = sd[bn + "." + f]
                assert len(np.unique(a)) == planes and np.abs(a).max() > 0.01, (bn, f)
            assert np.abs(sd[bn + ".running_var"] - 1).max() > 0.3 and np.abs(sd[bn + ".weight"] - 1).max() > 0.3
    if grid:
        assert all(np.array_equal(v.astype(np.float16).astype(np.float32), v) for v in sd.values() if v.ndim == 4 and v.shape[2] == 3)


@pytest.mark.parametrize("case", R.CASES, ids=[c.id for c in R.CASES])
def test_every_batch_of_the_gpu_cases_is_conditioned_and_reaches_the_edges(case):
    """Per case, on the boards of its own batch: the bounds (min p, max |z|) hold for any subset of the pool and are asserted
    again; the spreads are asserted wherever the batch has the boards to have one (16 on); the structured boards sit at
    index 0, across the 15 / 16 seam and in the last group."""
    m = case.boards()
    assert len(m) == case.batch
    r64, r32 = R.pool_reference(*case.net_key())
    assert r64["p"][m].min() >= 1e-8 and np.abs(r64["z"][m]).max() <= 1.5
    if case.batch >= 16:
        # (the logits are compared centred per board, so their spread is taken of the centred logits)
        assert 1.0 <= r64["logits"][m].std() <= 1.6 and r64["z"][m].std() >= 0.3, (r64["logits"][m].std(), r64["z"][m].std())
        assert len(np.unique(np.round(r64["z"][m], 6))) >= 8
    ns = R.n_structured(case.B, case.C)
    last = case.batch - (case.batch % 16 or 16)
    if case.batch >= 8:
        assert np.all(m[:5] < ns) and {2, 0, 3, 11} <= set(m.tolist())       # full, empty, a corner stone, float planes
        assert np.any(m >= ns)                                               # ... and never structured boards only
    else:
        assert m[0] == ns - 2 and (case.batch < 2 or m[1] == 2) and (case.batch < 7 or m[6] >= ns)
    if case.batch >= 9:
        assert np.all(m[case.batch - 3:] < ns)
    if case.batch >= 22:
        assert np.all(m[13:22] < ns)
    if case.batch > 32:
        assert np.all(m[last:] < ns) and set(range(ns)) <= set(m.tolist())
    el, ez = R.units(case.nb, case.B, case.planes, case.grid, m, case.C)
    assert R.E32_FLOOR <= el < 2e-5 and R.E32_FLOOR <= ez < 2e-5, (el, ez)  # the unit is fp32 rounding, not something larger
    if case.C > 1:
        # the colour plane C - 1 is one number per board: a conv1 that dropped it, or read it as padding, shows only if the batch
        # holds more than one colour. From 8 boards on both 0 and 1 are there; a handful of boards has the float-plane boards'
        # colours (0.37 ..) beside 0. The float-plane boards are in every batch.
        x = R.pool(case.B, case.C)[m]
        colours = set(x[:, case.C - 1, 0, 0].tolist())
        assert np.all(x[:, case.C - 1] == x[:, case.C - 1, :1, :1])
        assert ({0.0, 1.0} <= colours) if case.batch >= 8 else (case.batch < 2 or (len(colours) >= 2 and max(colours) > 0)), colours
    if case.batch >= 2:
        assert set(m.tolist()) & {ns - 3, ns - 2, ns - 1}                   # a board whose planes are neither 0 nor 1


@pytest.mark.parametrize("B", [9, 15])
@pytest.mark.parametrize("C", sorted(set(R.INPLANES) | {5}))
def test_pool_has_a_stone_on_every_plane_and_no_two_planes_alike(B, C):
    """What a swapped, dropped or doubled input plane needs to show: over the pool every stone plane 0 .. C - 2 is occupied on
    some 0/1 board, the colour plane takes both colours, and no two planes agree on every board -- neither over the whole
    pool nor over the boards the whole-forward defects of the catalogue are evaluated on."""
    x = R.pool(B, C)
    assert x.shape == (R.POOL if B <= 9 else R.WIDE_POOL, C, B, B)
    ns = R.n_structured(B, C)
    binary = np.array([set(np.unique(b)) <= {0.0, 1.0} for b in x])
    assert binary[ns:].all() and not binary[ns - 3:ns].any()
    for c in range(max(C - 1, 1)):
        assert (x[binary, c].reshape(binary.sum(), -1).sum(axis=1) > 0).sum() >= 8, c
    if C > 1:
        assert {0.0, 1.0} <= set(x[binary, C - 1, 0, 0].tolist())
    for rows in (slice(None), slice(0, SUBSET)):
        for a in range(C):
            for b in range(a + 1, C):
                assert not np.array_equal(x[rows, a], x[rows, b]), (a, b)


# ------------------------------------------------------------------------------------------------------------------
# 5. proof that the bound bites: defects of the float64 reference
# ------------------------------------------------------------------------------------------------------------------
SUBSET = 24      # the defects that need a whole forward are evaluated on the first boards of the pool (all structured boards
                 # and ten random ones): the effect over fewer boards is a lower bound of the effect over a case's batch


def _fp16(a):
    return a.astype(np.float16).astype(np.float32)


def _defects(nb, B, planes, grid, C=5):
    """name -> (|d centred logits| max over moves, |dz|) per pool board (NaN where the defect was not evaluated)."""
    import torch
    sd = R.case_network(nb, B, planes, grid, C)
    x = R.pool(B, C)
    n = len(x)
    ref = R.forward(sd, x)
    last = "layers.%d.conv2.weight" % (nb - 1)

    def delta(o, rows):
        dl = np.full(n, np.nan)
        dz = np.full(n, np.nan)
        dl[rows] = (R.centred(o["logits"]) - R.centred(ref["logits"][rows])).abs().max(dim=1).values.numpy()
        dz[rows] = (o["z"] - ref["z"][rows]).abs().numpy()
        return dl, dz

    def changed(f):
        s2 = {k: v.copy() for k, v in sd.items()}
        f(s2)
        return s2

    every = np.arange(n)
    sub = np.arange(min(SUBSET, n))
    out = {}

    def whole(name, f=lambda s: None, act_round=None):
        out[name] = delta(R.forward(changed(f), x[:len(sub)], act_round=act_round), sub)

    def last_block(name, f):
        out[name] = delta(R.forward(changed(f), x, resume=ref["last_in"]), every)

    def heads(name, f):
        out[name] = delta(R.forward(changed(f), x, trunk=ref["trunk"]), every)

    if not grid:      # (on fp16-grid weights there is no low half to lose: the two-product kernels leave it out by right)
        def w16_last(s):
            s[last][:16] = _fp16(s[last][:16])
        last_block("last conv, 16 couts: weights rounded to fp16 (a low-half product lost)", w16_last)

        def w16_all(s):
            for k in s:
                if s[k].ndim == 4 and s[k].shape[2] == 3:
                    s[k] = _fp16(s[k])
        whole("every conv: weights rounded to fp16", w16_all)
    whole("activations stored as one fp16 between layers", act_round=lambda t: t.half().to(t.dtype))

    def tap(s):
        s[last][7, :, 0, 0] = 0
    last_block("last conv: cout 7 loses tap (0, 0)", tap)

    def one_weight(s):
        s["layers.0.conv1.weight"][7, 3, 2, 2] = 0
    whole("first block, conv1: one (cout, cin, tap) zeroed", one_weight)

    def value_cin(s):
        s["value_head.value_head.weight"][0, planes - 1] = 0
    heads("value 1x1 conv: last input channel dropped", value_cin)

    def policy_cin(s):
        s["policy_head.policy_head.weight"][:, planes - 1] = 0
    heads("policy 1x1 conv: last input channel dropped", policy_cin)

    def fc_weight(s):
        s["policy_head.policy_fc.weight"][B * B // 2, B * B // 2] = 0
    heads("policy_fc: one weight zeroed (centre move, centre cell of channel 0)", fc_weight)

    def fc1_row(s):
        s["value_head.value_fc1.weight"][0, :] = 0
    heads("value_fc1: row 0 zeroed", fc1_row)

    def shift(s):
        s["layers.%d.bn2.bias" % (nb - 1)] = s["layers.%d.bn2.bias" % (nb - 1)] + np.float32(1e-3)
    last_block("last BatchNorm: shift off by 1e-3", shift)

    # conv1, the one layer whose packing and kernel text depend on the number of input planes. A single (cout, plane, tap)
    # weight can sit behind a dead ReLU on a small batch, so the per-plane defects span a 16-cout tile.
    for c in range(C):
        def plane_tap(s, c=c):
            s["conv1.weight"][0:16, c, 0, 0] = 0
        whole("conv1: plane %d loses tap (0, 0) in couts 0 .. 15 (a mis-indexed quad, a wrong bit)" % c, plane_tap)

    def drop_last(s):
        s["conv1.weight"][:, C - 1] = 0
    whole("conv1: plane C - 1 dropped (a ragged last quad read as padding)", drop_last)
    if C >= 2:
        def swap_last(s):
            s["conv1.weight"][:, [C - 2, C - 1]] = s["conv1.weight"][:, [C - 1, C - 2]]
        whole("conv1: planes C - 2 and C - 1 swapped", swap_last)
    return out, ref


_DEFECTS = {}


@pytest.mark.parametrize("case", R.CASES, ids=[c.id for c in R.CASES])
def test_every_defect_passes_twice_the_bound_of_every_gpu_case(case):
    """Each defect of the catalogue, applied to the float64 reference (nothing on the GPU is made to fail), moves the centred
    logits or z of the case's own boards by more than 2 x the case's bound (16 x E32 on the split-fp16 kernels, 4 x E32 on
    the fp32 ones). A defect that did not would mean the case is too insensitive to be a test of its kernel."""
    key = case.net_key()
    if key not in _DEFECTS:
        _DEFECTS.clear()                                   # cases of one network are adjacent: keep one network's tensors
        _DEFECTS[key] = _defects(*key)
    defects, ref = _DEFECTS[key]
    m = case.boards()
    u = np.unique(m)
    el, ez = R.units(case.nb, case.B, case.planes, case.grid, m, case.C)
    bl, bz = 2 * case.mult * el, 2 * case.mult * ez
    weak = []
    for name, (dl, dz) in defects.items():
        rows = u[~np.isnan(dl[u])]
        assert len(rows), name
        rl, rz = dl[rows].max() / bl, dz[rows].max() / bz
        if not (rl > 1 or rz > 1):
            weak.append("%s: %.2f / %.2f of twice the bound" % (name, rl, rz))
    if case.batch >= 2:
        # the stones of board k seen by board k + 1 (a group seam read one board off): board k + 1 gets board k's result
        lg, z = R.centred(ref["logits"]).numpy(), ref["z"].numpy()
        rl = max(np.abs(lg[m[i]] - lg[m[i + 1]]).max() for i in range(case.batch - 1)) / bl
        rz = max(abs(z[m[i]] - z[m[i + 1]]) for i in range(case.batch - 1)) / bz
        if not (rl > 1 or rz > 1):
            weak.append("board k + 1 sees the stones of board k: %.2f / %.2f" % (rl, rz))
    assert not weak, weak
