"""-m gpu: the fp16 forward at every batch size (ao_net_precision(AO_NET_PRECISION_FP16_ALL) / Net.precision("fp16-all")).

"fp16-all" is the arithmetic of "fp16" (tests/test_gpu_fp16_forward.py: the weight operand fp16(w * 2^s), every stored trunk
activation rounded ONCE to fp16, to nearest even, after ReLU and clamp; fp32 accumulation, BatchNorm, residual add and heads) for
EVERY forward of a net: the batches that are planned onto neither the resident trunk nor k_boardh run the one-product per-layer
kernel k_layer16h_f16<B, XT, 4, KIND> for every layer, conv1 included, and heads that read the high half alone.

The bit comparisons build the Net in mode 6, so both sides run the per-layer trunk (k_layer16h_w16 against k_layer16h_f16) and the
same head kernels. Shapes (blocks, board, boards) and the tiling the planner's cost function (net.hip, 256 CUs) gives them --
grid = groups x row chunks x column tiles:
    (2, 9, 17)      two groups, one ragged; nine single-row chunks: halo rows on both sides
    (2, 9, 1041)    66 groups; three chunks of three rows
    (2, 9, 3073)    193 groups (mode 6); one chunk = the whole board: first and last row in one workgroup
    (1, 7, 33), (2, 4, 17), (1, 3, 16)    small boards
    (2, 15, 17)     XT = 4, four column tiles, the last ragged (3 columns)
    (2, 10, 33)     XT = 4, three column tiles, the last ragged (2 columns); with AO_XT=5 (read at create) the XT = 5 form
    (1, 12, 17)     a wide board below the k_boardh threshold

  1. on the EXACT network rounding is the identity: "fp16-all" returns the default forward's bits, both are the float64
     reference to 1e-5;
  2. on the PERTURBED twin "fp16-all" rounds the 2^-12 away and returns the unperturbed network's bits, after a default forward
     of the same Net has left non-zero low halves in the activation buffers: a head or residual that still read them fails;
  3. ao_search on bit planes and live rows (mode 5): same pi, visits, priors, moves and results as "fp32" on the exact network;
  4. on realistic weights the device is within 3 x E_fast of float64 (the rule of test_gpu_fp16_forward.py);
  5. in mode 6 a board's bits do not depend on the size of the batch around it;
  6. the switch.
"""
import json

import numpy as np
import pytest

import fp16_all_batches as fb
import fp16_forward_nets as fn
import net_reference as nr

pytestmark = pytest.mark.gpu

# (blocks, board, boards, AO_XT or None)
EXACT = [(2, 9, 17, None), (2, 9, 1041, None), (2, 9, 3073, None), (1, 7, 33, None), (2, 4, 17, None), (1, 3, 16, None),
         (2, 15, 17, None), (2, 10, 33, None), (1, 12, 17, None), (2, 10, 33, 5)]
TWIN = [(2, 9, 17), (2, 9, 1041), (2, 15, 17), (2, 10, 33), (1, 7, 33)]


def _net(sd, nb, B, mode):
    from alpha_omok_amd.engine import Net
    net = Net(nb, 5, 128, B, 0)
    net.set_mode(mode)
    net.load_state_dict(sd)
    return net


def _forward(net, x, batch, kernel):
    import torch
    p, v = net(x)
    torch.cuda.synchronize()
    name = net.dominant_kernel(batch)[0]
    assert name.startswith(kernel), (name, kernel)
    if name.startswith("k_layer16h_f16"):
        assert len(name) < 255 and name.endswith(")"), name     # (the name buffer of Net.dominant_kernel holds 256 bytes: not cut)
    return p, v, name


@pytest.mark.parametrize("nb,B,batch,xt", EXACT, ids=["nb%d-B%d-%d%s" % (c[0], c[1], c[2], "-xt5" if c[3] else "") for c in EXACT])
def test_fp16_all_returns_the_default_bits_where_rounding_is_exact(nb, B, batch, xt, monkeypatch):
    import torch
    if xt:
        monkeypatch.setenv("AO_XT", str(xt))
    sd = fn.exact_network(nb, B)
    idx = fb.batch_of(B, batch)
    x = torch.from_numpy(fn.binary_pool(B)[idx]).cuda()
    net = _net(sd, nb, B, 6)
    assert net.precision() == "fp32" and net.products() == (2, True)
    p0, v0, name0 = _forward(net, x, batch, "k_layer16h_w16<%d>" % B)
    f0 = net.dominant_kernel(batch)[1]
    assert net.precision("fp16-all") == "fp16-all"
    p1, v1, name1 = _forward(net, x, batch, "k_layer16h_f16<%d>" % B)
    assert "1 product: the opt-in fp16 forward" in name1 and "_w16" not in name1
    assert net.dominant_kernel(batch)[1] == pytest.approx(f0)    # algorithmic FLOPs: unchanged
    assert net.status() == 0
    net.close()
    rp, rv = fn.exact_reference(nb, B)
    dp0 = float(np.abs(p0.cpu().double().numpy() - rp[idx]).max())
    dv0 = float(np.abs(v0.cpu().double().numpy() - rv[idx]).max())
    dp1 = float(np.abs(p1.cpu().double().numpy() - rp[idx]).max())
    dv1 = float(np.abs(v1.cpu().double().numpy() - rv[idx]).max())
    nbad = int((p0 != p1).any(dim=1).sum() + (v0 != v1).sum())
    print("FP16_ALL_EXACT " + json.dumps(dict(nb=nb, B=B, batch=batch, xt=xt, dp_default=dp0, dv_default=dv0, dp_fp16=dp1, dv_fp16=dv1,
                                              rows_differing=nbad)))
    assert torch.equal(p0, p1) and torch.equal(v0, v1), "%d rows of the fp16-all forward differ from the default forward" % nbad
    assert dp0 < 1e-5 and dv0 < 1e-5 and dp1 < 1e-5 and dv1 < 1e-5, (dp0, dv0, dp1, dv1)


@pytest.mark.parametrize("nb,B,batch", TWIN, ids=["nb%d-B%d-%d" % c for c in TWIN])
def test_fp16_all_rounds_every_stored_activation_and_reads_no_stale_low_half(nb, B, batch):
    """In this order on ONE Net: the default forward of the twin, the default forward of the perturbed network (which leaves
    non-zero low halves in act_x / act_t), "fp16-all" of the perturbed network. The bound on the gap is the one of
    test_fp16_forward_rounds_every_stored_activation_to_nearest, for its reason (float64 reference: 2e-3 .. 3e-2 in a logit)."""
    import torch
    twin, pert = fn.perturbed_pair(nb, B)
    idx = fb.batch_of(B, batch)
    x = torch.from_numpy(fn.binary_pool(B)[idx]).cuda()
    net = _net(twin, nb, B, 6)
    pt, vt, _ = _forward(net, x, batch, "k_layer16h_w16<%d>" % B)
    net.load_state_dict(pert)
    pd, vd, _ = _forward(net, x, batch, "k_layer16h_w16<%d>" % B)
    net.precision("fp16-all")
    pf, vf, _ = _forward(net, x, batch, "k_layer16h_f16<%d>" % B)
    assert net.status() == 0
    net.close()
    lt, ld = torch.log(pt.double()), torch.log(pd.double())
    gap = float((nr.centred(ld) - nr.centred(lt)).abs().max())
    nbad = int((pf != pt).any(dim=1).sum() + (vf != vt).sum())
    print("FP16_ALL_ROUNDING " + json.dumps(dict(nb=nb, B=B, batch=batch, default_vs_twin_logit_gap=gap, rows_differing=nbad)))
    assert torch.equal(pf, pt) and torch.equal(vf, vt), "%d rows: the fp16-all forward of the perturbed network is not the twin's" % nbad
    assert not torch.equal(pd, pt), "the default forward lost the perturbation: the test network does not perturb what it stores"
    assert gap >= 5e-4, gap


@pytest.mark.parametrize("B,S,G,nb", [(9, 12, 48, 2), (15, 8, 16, 2)])
def test_search_on_bit_planes_and_live_rows_is_the_same_under_fp16_all_on_the_exact_network(B, S, G, nb):
    from alpha_omok_amd.engine import Engine
    net = _net(fn.exact_network(nb, B), nb, B, 5)
    seeds = np.arange(4000, 4000 + G, dtype=np.uint32)
    out = {}
    for precision in ("fp32", "fp16-all"):
        net.precision(precision)
        eng = Engine(B, S, 5, games=G, noise=True)
        eng.seed_all(seeds)
        rec = []
        for ply in range(2):
            pi, vis, pol = eng.search(net, tau=np.ones(G, np.int8))
            act, win = eng.play()
            rec.append((pi, vis, pol, act, win))
        out[precision] = rec
        kname = net.dominant_kernel(G)[0]
        if precision == "fp16-all":
            assert kname.startswith("k_layer16h_f16<%d>" % B) and "KIND 2" in kname, kname
        else:
            assert "_f16" not in kname, kname
        eng.close()
    for a, b in zip(out["fp32"], out["fp16-all"]):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    assert np.all(out["fp16-all"][0][1].sum(axis=1) == S)            # every visit row of the first ply sums to S ...
    assert np.all(out["fp16-all"][1][1].sum(axis=1) >= S)            # ... and of the second to S + what its subtree inherited
    assert net.status() == 0
    net.close()


def _fp16_planes(x):
    return np.all(x.astype(np.float16).astype(np.float32) == x, axis=(1, 2, 3))


def _fp16_batch(B, batch):
    """Pool indices of a batch whose planes are fp16 numbers (test_gpu_fp16_forward.py's replacement rule)."""
    ok = _fp16_planes(nr.pool(B))
    m = nr.batch_indices(batch, B)
    repl = np.random.RandomState(batch).choice(np.nonzero(ok)[0], size=batch)
    return np.where(ok[m], m, repl)


@pytest.mark.parametrize("nb,B,batch,grid", [(nb, B, batch, grid) for nb, B, batch in [(4, 9, 300), (2, 7, 33), (2, 15, 17)] for grid in (False, True)])
def test_fp16_all_on_realistic_weights_is_within_three_e_fast_of_float64(nb, B, batch, grid):
    """The rule, the margin and its derivation are those of test_fp16_forward_on_realistic_weights_is_within_three_e_fast_of_float64:
    E_fast is the distance of the arithmetic's definition (fp16 conv weights, every stored activation rounded once, all else
    float64) from the exact float64 evaluation over the boards of the batch; the device differs from that emulation only by
    roundings that flip with the summation order (<= 1.9 x E_fast expected, 3 x leaves room for another order). Mode 0: these
    are batches "fp16" leaves on k_row16hk (300 boards of 9x9), the per-board path (33 of 7x7) and k_layer16h (17 of 15x15)."""
    import torch
    sd = nr.case_network(nb, B, 128, grid)
    pool = nr.pool(B)
    m = _fp16_batch(B, batch)
    u = np.unique(m)
    exact = nr.forward(sd, pool[u])
    emul = nr.forward(nr.project_to_fp16_grid(sd), pool[u], act_round=fn.r16)
    e_l, e_z = nr.distances(emul, exact)
    net = _net(sd, nb, B, 0)
    net.precision("fp16-all")
    p, v, _ = _forward(net, torch.from_numpy(pool[m]).cuda(), batch, "k_layer16h_f16<%d>" % B)
    status = net.status()
    net.close()
    p, v = p.cpu().double().numpy(), v.cpu().double().numpy()
    assert np.isfinite(p).all() and p.min() > 0 and np.abs(v).max() < 1
    pos = np.searchsorted(u, m)
    lp = np.log(p)
    ref_l = nr.centred(exact["logits"]).numpy()[pos]
    err_l = float(np.abs(lp - lp.mean(axis=1, keepdims=True) - ref_l).max())
    err_z = float(np.abs(np.arctanh(v) - exact["z"].numpy()[pos]).max())
    print("FP16_ALL_CONTRACT " + json.dumps(dict(nb=nb, B=B, batch=batch, grid=grid, E_fast_l=e_l, E_fast_z=e_z, err_l=err_l, err_z=err_z,
                                                 ratio_l=err_l / e_l, ratio_z=err_z / e_z)))
    assert status == 0
    assert err_l <= 3 * e_l and err_z <= 3 * e_z, (err_l / e_l, err_z / e_z)


@pytest.mark.parametrize("nb,B,small,larger", [(2, 9, 17, (1041, 3073)), (2, 15, 17, (65,))])
def test_fp16_all_in_mode_6_is_one_arithmetic_for_every_batch_size(nb, B, small, larger):
    import torch
    sd = nr.case_network(nb, B, 128, False)
    pool = nr.pool(B)
    first = nr.batch_indices(small, B)
    net = _net(sd, nb, B, 6)
    net.precision("fp16-all")
    p0, v0, _ = _forward(net, torch.from_numpy(pool[first]).cuda(), small, "k_layer16h_f16<%d>" % B)
    assert len(np.unique(first)) >= 12 and not torch.equal(p0[0], p0[1])
    for batch in larger:
        m = nr.batch_indices(batch, B, seed=1).copy()
        m[:small] = first
        p, v, _ = _forward(net, torch.from_numpy(pool[m]).cuda(), batch, "k_layer16h_f16<%d>" % B)
        assert torch.equal(p[:small], p0) and torch.equal(v[:small], v0), batch
    assert net.status() == 0
    net.close()


def test_fp16_all_switch_semantics():
    import torch
    from alpha_omok_amd.engine import EngineError, Net
    sd = nr.project_to_fp16_grid(nr.case_network(2, 9, 128, True))
    net = _net(sd, 2, 9, 0)
    assert Net.PRECISIONS == ("fp32", "fp16", "fp16-all")
    assert net.precision() == "fp32" and net.precision("fp16-all") == "fp16-all" and net.precision() == "fp16-all"
    assert net.products() == (2, True)                                   # products() keeps answering for the fp32-equivalent kernels
    assert net.products(3) == (3, True) and net.precision() == "fp16-all" and net.products(0) == (2, True)
    net.load_state_dict(sd)                                              # survives a re-export
    assert net.precision() == "fp16-all"
    assert net.dominant_kernel(4096)[0].startswith("k_trunk16h_f16<9, 4, 0>")
    assert net.dominant_kernel(1)[0].startswith("k_layer16h_f16<9>")
    x = torch.from_numpy(nr.pool(9)[nr.batch_indices(300, 9)]).cuda()
    pa, va, _ = _forward(net, x, 300, "k_layer16h_f16<9>")
    p1, v1, _ = _forward(net, x[:1], 1, "k_layer16h_f16<9>")
    assert torch.isfinite(p1).all() and abs(float(p1.sum()) - 1.0) < 1e-4
    # "fp16" and "fp32" keep their meaning: a batch planned elsewhere runs what it runs anyway
    assert net.precision("fp16") == "fp16"
    p16, v16, name = _forward(net, x, 300, "k_row16hk_w16<9>")
    assert "_f16" not in name and "_f16" in net.dominant_kernel(4096)[0]
    assert net.precision("fp32") == "fp32"
    p32, v32, _ = _forward(net, x, 300, "k_row16hk_w16<9>")
    assert torch.equal(p16, p32) and torch.equal(v16, v32)
    assert not torch.equal(pa, p32)                                      # (realistic weights: the fp16 arithmetic is another one)
    for boards in (1, 300, 4096):
        assert "_f16" not in net.dominant_kernel(boards)[0]
    with pytest.raises(ValueError):
        net.precision("bf16")
    net.close()
    wide = _net(fn.exact_network(2, 15), 2, 15, 0)
    wide.precision("fp16-all")
    assert wide.dominant_kernel(64)[0].startswith("k_boardh_f16<15")
    assert wide.dominant_kernel(17)[0].startswith("k_layer16h_f16<15>")
    wide.close()
    import pvnet_weights
    small = Net(2, 5, 64, 9, 0)
    small.load_state_dict(pvnet_weights.make_state_dict(2, 5, 64, 9, 3))
    with pytest.raises(EngineError, match="fp16"):
        small.precision("fp16-all")
    assert small.precision() == "fp32"
    small.close()


def test_evaluator_applies_fp16_all_after_every_export():
    import torch
    from alpha_omok_amd.evaluator import Evaluator
    from alpha_omok_amd.pvnet import PVNet
    torch.manual_seed(0)
    model = PVNet(1, 5, 128, 5).cuda()
    ev = Evaluator(0)
    ev.net_precision = "fp16-all"
    net = ev.native_net(model, 5, 5)
    assert net.precision() == "fp16-all"
    with torch.no_grad():
        model.bn1.bias.add_(0.5)
    assert ev.native_net(model, 5, 5).precision() == "fp16-all"
    assert net.dominant_kernel(1)[0].startswith("k_layer16h_f16<5>")
    net.close()
