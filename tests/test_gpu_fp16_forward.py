"""-m gpu: the opt-in fp16 forward (ao_net_precision / Net.precision; net_f16.hip).

"fp16" = one MFMA product per multiply-add: the weight operand fp16(w * 2^s), the activation operand the activation rounded ONCE
to fp16 (to nearest even, after ReLU and clamp), fp32 accumulation; BatchNorm, residual add, ReLU and the heads fp32; everything
downstream of a layer reads the rounded activation. On the host: net_reference.forward(project_to_fp16_grid(sd), x, act_round=r16).
It runs where the resident trunk (k_trunk16h / k_trunk16hb, boards up to 9x9, >= 192 groups) or the board-resident trunk
(k_boardh, wider boards, >= 64 boards) is planned; everything else keeps its fp32-equivalent kernel.

  1. on the EXACT network (tests/fp16_forward_nets.py: every stored activation is an fp16 number) rounding is the identity: the
     fp16 forward returns the default forward's bits -- a dropped tap, a wrong residual source, a wrong handed row or a stale low
     fragment would show -- and both are the float64 reference to 1e-5;
  2. on the PERTURBED twin the activations of 32 channels per layer sit 2^-12 off an fp16 number: the fp16 forward rounds them
     back and returns the unperturbed network's bits, the default forward (which keeps its low halves) does not. Truncation, or a
     kernel that silently kept low halves, fails;
  3. ao_search through the bit-plane kernels: same pi, visits, priors, moves and results as the default search on the exact network;
  4. on realistic weights the device is within 3 x E_fast of the float64 reference, E_fast being the distance of the host
     emulation from it, computed here;
  5. the switch: round trip, survives a re-export, refused by networks the kernels do not cover, no effect on batches planned
     elsewhere, independent of products().
"""
import json

import numpy as np
import pytest

import fp16_forward_nets as fn
import net_reference as nr

pytestmark = pytest.mark.gpu

# (blocks, board, boards of the batch, kernel of the default forward, kernel under "fp16"): a ragged 193rd group, the smallest and
# an even board of the resident trunk; a ragged and a whole round of the board-resident trunk, an even wide board
RESIDENT = [(2, 9, 3073), (1, 7, 3104), (2, 4, 3073), (1, 3, 3072)]
WIDE = [(2, 15, 65), (2, 10, 64), (1, 12, 65)]
EXACT_CASES = [(nb, B, n, "k_trunk16h_w16<%d, 4, 0>" % B, "k_trunk16h_f16<%d, 4, 0>" % B) for nb, B, n in RESIDENT] + \
              [(nb, B, n, "k_boardh_w16<%d, 1>" % B, "k_boardh_f16<%d, 1>" % B) for nb, B, n in WIDE]


def _net(sd, nb, B):
    from alpha_omok_amd.engine import Net
    net = Net(nb, 5, 128, B, 0)
    net.load_state_dict(sd)
    return net


def _forward(net, x, batch, kernel):
    import torch
    p, v = net(x)
    torch.cuda.synchronize()
    name = net.dominant_kernel(batch)[0]
    assert name.startswith(kernel), (name, kernel)
    return p, v, name


@pytest.mark.parametrize("nb,B,batch,k_default,k_fp16", EXACT_CASES, ids=["nb%d-B%d-%d" % c[:3] for c in EXACT_CASES])
def test_fp16_forward_returns_the_default_bits_where_rounding_is_exact(nb, B, batch, k_default, k_fp16):
    import torch
    sd = fn.exact_network(nb, B)
    idx = fn.batch_of(B, batch)
    x = torch.from_numpy(fn.binary_pool(B)[idx]).cuda()
    net = _net(sd, nb, B)
    assert net.precision() == "fp32" and net.products() == (2, True)
    p0, v0, name0 = _forward(net, x, batch, k_default)
    assert "2 products" in name0
    assert net.precision("fp16") == "fp16"
    p1, v1, name1 = _forward(net, x, batch, k_fp16)
    assert "1 product" in name1 and "_w16" not in name1
    assert net.dominant_kernel(batch)[1] == pytest.approx(_flops(net, batch, "fp32"))     # algorithmic FLOPs: unchanged
    net.precision("fp16")
    assert net.status() == 0
    rp, rv = fn.exact_reference(nb, B)
    dp0 = float(np.abs(p0.cpu().double().numpy() - rp[idx]).max())
    dv0 = float(np.abs(v0.cpu().double().numpy() - rv[idx]).max())
    dp1 = float(np.abs(p1.cpu().double().numpy() - rp[idx]).max())
    dv1 = float(np.abs(v1.cpu().double().numpy() - rv[idx]).max())
    nbad = int((p0 != p1).any(dim=1).sum() + (v0 != v1).sum())
    print("FP16_EXACT " + json.dumps(dict(nb=nb, B=B, batch=batch, dp_default=dp0, dv_default=dv0, dp_fp16=dp1, dv_fp16=dv1, rows_differing=nbad)))
    assert torch.equal(p0, p1) and torch.equal(v0, v1), "%d rows of the fp16 forward differ from the default forward" % nbad
    assert dp0 < 1e-5 and dv0 < 1e-5 and dp1 < 1e-5 and dv1 < 1e-5, (dp0, dv0, dp1, dv1)
    net.close()


def _flops(net, batch, precision):
    was = net.precision()
    net.precision(precision)
    f = net.dominant_kernel(batch)[1]
    net.precision(was)
    return f


@pytest.mark.parametrize("nb,B,batch,k_default,k_fp16", [EXACT_CASES[0], EXACT_CASES[1], EXACT_CASES[4], EXACT_CASES[5]],
                         ids=["nb2-B9-3073", "nb1-B7-3104", "nb2-B15-65", "nb2-B10-64"])
def test_fp16_forward_rounds_every_stored_activation_to_nearest(nb, B, batch, k_default, k_fp16):
    import torch
    twin, pert = fn.perturbed_pair(nb, B)
    idx = fn.batch_of(B, batch)
    x = torch.from_numpy(fn.binary_pool(B)[idx]).cuda()
    net = _net(twin, nb, B)
    pt, vt, _ = _forward(net, x, batch, k_default)            # default forward of the unperturbed network
    net.load_state_dict(pert)
    pd, vd, _ = _forward(net, x, batch, k_default)            # default forward of the perturbed one: keeps the 2^-12
    net.precision("fp16")
    pf, vf, _ = _forward(net, x, batch, k_fp16)               # fp16 forward of the perturbed one: rounds it away
    assert net.status() == 0
    net.close()
    lt, ld = torch.log(pt.double()), torch.log(pd.double())
    gap = float((nr.centred(ld) - nr.centred(lt)).abs().max())
    nbad = int((pf != pt).any(dim=1).sum() + (vf != vt).sum())
    print("FP16_ROUNDING " + json.dumps(dict(nb=nb, B=B, batch=batch, default_vs_twin_logit_gap=gap, rows_differing=nbad)))
    assert torch.equal(pf, pt) and torch.equal(vf, vt), "%d rows: the fp16 forward of the perturbed network is not the twin's" % nbad
    assert not torch.equal(pd, pt), "the default forward lost the perturbation: the test network does not perturb what it stores"
    assert gap >= 5e-4, gap                                   # (float64 reference: 2e-3 .. 3e-2 in a logit)


@pytest.mark.parametrize("B,S,G,nb,kernel", [(9, 12, 3072, 2, "k_trunk16hb_f16<9, 4, 0>"), (15, 8, 64, 2, "k_boardh_f16<15, 2>")])
def test_search_on_bit_planes_is_the_same_under_fp16_on_the_exact_network(B, S, G, nb, kernel):
    from alpha_omok_amd.engine import Engine
    net = _net(fn.exact_network(nb, B), nb, B)
    seeds = np.arange(4000, 4000 + G, dtype=np.uint32)
    out = {}
    for precision in ("fp32", "fp16"):
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
        assert kname.startswith(kernel if precision == "fp16" else kernel.replace("_f16", "_w16")), kname
        eng.close()
    for a, b in zip(out["fp32"], out["fp16"]):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    assert np.all(out["fp16"][0][1].sum(axis=1) == S)
    assert net.status() == 0
    net.close()


def _fp16_planes(x):
    return np.all(x.astype(np.float16).astype(np.float32) == x, axis=(1, 2, 3))


@pytest.mark.parametrize("nb,B,batch,grid", [(nb, B, batch, grid) for nb, B, batch in [(4, 9, 3073), (2, 7, 3104), (2, 15, 65)] for grid in (False, True)])
def test_fp16_forward_on_realistic_weights_is_within_three_e_fast_of_float64(nb, B, batch, grid):
    """E_fast: the distance of the arithmetic's DEFINITION (fp16 conv weights, every stored activation rounded once, all else
    float64) from the exact float64 evaluation, over the boards of the batch. The device differs from that emulation only by
    roundings that flip with the summation order: on the CPU a float32-accumulate emulation sits 0.2 .. 0.9 x E_fast from the
    float64-accumulate one (7 networks), so <= 1.9 x E_fast is expected and 3 x leaves room for another order."""
    import torch
    sd = nr.case_network(nb, B, 128, grid)
    pool = nr.pool(B)
    ok = _fp16_planes(pool)
    m = nr.batch_indices(batch, B)
    repl = np.random.RandomState(batch).choice(np.nonzero(ok)[0], size=batch)
    m = np.where(ok[m], m, repl)
    u = np.unique(m)
    exact = nr.forward(sd, pool[u])
    emul = nr.forward(nr.project_to_fp16_grid(sd), pool[u], act_round=fn.r16)
    e_l, e_z = nr.distances(emul, exact)
    net = _net(sd, nb, B)
    net.precision("fp16")
    kernel = ("k_trunk16h_f16<%d, 4, 0>" if B <= 9 else "k_boardh_f16<%d, 1>") % B
    p, v, _ = _forward(net, torch.from_numpy(pool[m]).cuda(), batch, kernel)
    status = net.status()
    net.close()
    p, v = p.cpu().double().numpy(), v.cpu().double().numpy()
    assert np.isfinite(p).all() and p.min() > 0 and np.abs(v).max() < 1
    pos = np.searchsorted(u, m)
    lp = np.log(p)
    ref_l = nr.centred(exact["logits"]).numpy()[pos]
    err_l = float(np.abs(lp - lp.mean(axis=1, keepdims=True) - ref_l).max())
    err_z = float(np.abs(np.arctanh(v) - exact["z"].numpy()[pos]).max())
    print("FP16_CONTRACT " + json.dumps(dict(nb=nb, B=B, batch=batch, grid=grid, E_fast_l=e_l, E_fast_z=e_z, err_l=err_l, err_z=err_z,
                                             ratio_l=err_l / e_l, ratio_z=err_z / e_z)))
    assert status == 0
    assert err_l <= 3 * e_l and err_z <= 3 * e_z, (err_l / e_l, err_z / e_z)


def test_precision_switch_semantics():
    import torch
    from alpha_omok_amd.engine import EngineError, Net
    sd = nr.project_to_fp16_grid(nr.case_network(2, 9, 128, True))
    net = _net(sd, 2, 9)
    assert net.precision() == "fp32" and net.precision("fp16") == "fp16" and net.precision() == "fp16"
    assert net.products() == (2, True)                                   # products() keeps answering for the fp32-equivalent kernels
    assert net.products(3) == (3, True) and net.precision() == "fp16" and net.products(0) == (2, True)
    net.load_state_dict(sd)                                              # survives a re-export
    assert net.precision() == "fp16"
    assert "k_trunk16h_f16<9, 4, 0>" in net.dominant_kernel(4096)[0]
    with pytest.raises(ValueError):
        net.precision("bf16")
    # a batch planned elsewhere runs what it runs anyway, to the bit
    x = torch.from_numpy(nr.pool(9)[nr.batch_indices(300, 9)]).cuda()
    p1, v1, name = _forward(net, x, 300, "k_row16hk_w16<9>")
    assert "_f16" not in name
    assert net.precision("fp32") == "fp32"
    p0, v0, _ = _forward(net, x, 300, "k_row16hk_w16<9>")
    assert torch.equal(p0, p1) and torch.equal(v0, v1)
    assert "_f16" not in net.dominant_kernel(4096)[0]
    net.close()
    import pvnet_weights
    small = Net(2, 5, 64, 9, 0)
    small.load_state_dict(pvnet_weights.make_state_dict(2, 5, 64, 9, 3))
    assert small.precision() == "fp32"
    with pytest.raises(EngineError, match="fp16"):
        small.precision("fp16")
    assert small.precision() == "fp32"
    small.close()


def test_evaluator_applies_its_precision_after_every_export():
    """main.configure(forward_precision="fp16") -> Evaluator.net_precision -> Net.precision beside net_mode; what ZeroAgent,
    evaluate_batched and PositionBatch.evaluate inherit."""
    import torch
    from alpha_omok_amd.evaluator import Evaluator
    from alpha_omok_amd.pvnet import PVNet
    torch.manual_seed(0)
    model = PVNet(1, 5, 128, 5).cuda()
    ev = Evaluator(0)
    ev.net_precision = "fp16"
    net = ev.native_net(model, 5, 5)
    assert net.precision() == "fp16"
    with torch.no_grad():
        model.bn1.bias.add_(0.5)
    assert ev.native_net(model, 5, 5).precision() == "fp16"
    net.close()
