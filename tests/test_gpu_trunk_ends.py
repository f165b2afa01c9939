"""-m gpu: the two ends of the resident split-fp16 trunk (k_trunk16h / k_trunk16hb, net_trunk_h16.hpp).

conv1 on the engine's bit planes builds the high-half fragments of the whole board in LDS once and then runs all rows without a
row barrier; one barrier stands between the last read of that board and the two rows handed to the first trunk layer, which
overwrite it. The last trunk layer hands its last two output rows to the heads through the LDS row buffers and does not store
them; trunk_heads takes those cells first (weights from global memory, sums in registers), before s_w3 / s_h overwrite the row
buffers. Weight slabs whose MFMAs are skipped (output row off the board, prefetch past the last row) are not fetched.

What can go wrong is at the two ends only, so the shapes are those of tests/test_gpu_trunk_handoff.py: board widths 9 and 7
(odd) and 8 (even: the row buffers swapped, and the last layer reached with the other parity), 1 and 2 ResBlocks, 16 boards
(one group) and 17 (a second group with one real board). AO_FORCE_RESIDENT=1 (read when the Net is created) plans the resident
kernel for any batch in mode 5. Networks, boards, references and bounds are those of that file: (p, v) within 1e-4 of the torch
fp32 forward, centred log p and atanh v within 16 x E32 of the float64 reference.

(There is no test that mode 5 equals the per-layer kernels of mode 6 bit for bit: the resident kernel walks every other layer
from the last row to the first, so its accumulators add the input rows in the other order -- see profiles/r22a_trunk_ends.txt.)"""
import numpy as np
import pytest

import net_reference as R

pytestmark = pytest.mark.gpu
TOL = 1e-4       # on (p, v) against torch fp32, as tests/test_gpu_trunk_handoff.py
MULT = 16        # x E32 in logit space: net_reference.Case.mult of the split-fp16 families

WIDTHS = (9, 7, 8)
SHAPES = [(nb, B, batch) for B in WIDTHS for nb in (1, 2) for batch in (16, 17)]


def _resident_net(monkeypatch, nb, B, grid):
    from alpha_omok_amd.engine import Net
    monkeypatch.setenv("AO_FORCE_RESIDENT", "1")
    net = Net(nb, 5, 128, B, 0)
    monkeypatch.delenv("AO_FORCE_RESIDENT")
    net.load_state_dict(R.case_network(nb, B, 128, grid))
    net.set_mode(5)
    return net


@pytest.mark.parametrize("nb,B,G", SHAPES)
def test_fused_search_on_bit_planes_through_resident_conv1_equals_stepwise_on_float_planes(nb, B, G, monkeypatch):
    """The fused search feeds k_trunk16hb the leaf planes as bits (conv1 as one pass over the LDS-resident board); the stepwise
    protocol feeds k_trunk16h the same planes as floats (conv1 on the row loop). The planes are 0/1, so both see the same
    operands in the same order: visits, priors, pi and moves must be equal bit for bit."""
    import torch
    from alpha_omok_amd.engine import Engine
    from gpu_helpers import HostEvalRunner
    S = 8
    net = _resident_net(monkeypatch, nb, B, False)
    seeds = np.arange(40, 40 + G, dtype=np.uint32)
    e1 = Engine(B, S, 5, games=G, noise=True)
    e2 = Engine(B, S, 5, games=G, noise=True)
    e1.seed_all(seeds)
    e2.seed_all(seeds)
    run = HostEvalRunner(e2)
    for t in range(2):
        tau = np.full(G, 1 if t < 1 else 0, np.int8)
        pi1, vis1, pol1 = e1.search(net, tau=tau)
        name = net.dominant_kernel(G)[0]
        assert name.startswith("k_trunk16hb<%d, 4, 0>" % B), name
        e2.begin_move()
        while e2.sims_left() > 0:
            e2.collect_leaves(run.planes.data_ptr())
            e2.sync()
            p, v = net(run.planes)
            torch.cuda.synchronize()
            e2.apply_evals(p.data_ptr(), v.data_ptr())
        assert net.dominant_kernel(G)[0].startswith("k_trunk16h<%d, 4, 0>" % B)
        pi2, vis2, pol2 = e2.end_move(tau)
        np.testing.assert_array_equal(vis1, vis2)
        np.testing.assert_array_equal(pol1, pol2)
        np.testing.assert_array_equal(pi1, pi2)
        a1, w1 = e1.play()
        a2, w2 = e2.play()
        np.testing.assert_array_equal(a1, a2)
        np.testing.assert_array_equal(w1, w2)
    assert net.status() == 0
    e1.close()
    e2.close()
    net.close()


@pytest.mark.parametrize("nb,B,batch", SHAPES)
def test_heads_fed_from_lds_against_float64_in_logit_space(nb, B, batch, monkeypatch):
    import torch
    m = R.batch_indices(batch, B)
    x = torch.from_numpy(R.pool(B)[m]).cuda()
    net = _resident_net(monkeypatch, nb, B, False)
    assert net.products() == (3, False)
    p, v = net(x)
    torch.cuda.synchronize()
    name = net.dominant_kernel(batch)[0]
    assert name.startswith("k_trunk16h<%d, 4, 0>" % B) and "3 products" in name, name
    assert net.status() == 0
    net.close()
    p, v = p.cpu().double().numpy(), v.cpu().double().numpy().reshape(-1)
    assert p.shape == (batch, B * B) and v.shape == (batch,)
    assert np.isfinite(p).all() and np.isfinite(v).all() and p.min() > 0 and np.abs(v).max() < 1
    r64, r32 = R.pool_reference(nb, B, 128, False)
    el, ez = R.units(nb, B, 128, False, m)
    lp = np.log(p)
    err_l = float(np.abs(lp - lp.mean(axis=1, keepdims=True) - r64["logits"][m]).max())
    err_z = float(np.abs(np.arctanh(v) - r64["z"][m]).max())
    dp = float(np.abs(p - r32["p"][m]).max())
    dv = float(np.abs(v - r32["v"][m]).max())
    print("ENDS nb=%d B=%d batch=%d: centred logits %.2f x E32 (%.2e), atanh v %.2f x E32 (%.2e), dp %.1e, dv %.1e"
          % (nb, B, batch, err_l / el, err_l, err_z / ez, err_z, dp, dv))
    assert dp < TOL and dv < TOL, (dp, dv)
    assert err_l <= MULT * el and err_z <= MULT * ez, \
        "centred logits off by %.2f x E32 (%.2e), atanh v by %.2f x E32 (%.2e); allowed %d x" % (err_l / el, err_l, err_z / ez, err_z, MULT)


@pytest.mark.parametrize("nb,B,batch", SHAPES)
def test_heads_fed_from_lds_two_products_are_the_three_product_bits(nb, B, batch, monkeypatch):
    """On conv weights that are fp16 numbers k_trunk16h_w16 returns the bits of k_trunk16h; both hand the heads their last two
    rows in LDS, and both are the float32-equivalent result."""
    import torch
    m = R.batch_indices(batch, B)
    x = torch.from_numpy(R.pool(B)[m]).cuda()
    net = _resident_net(monkeypatch, nb, B, True)
    assert net.products() == (2, True)
    p2, v2 = (t.clone() for t in net(x))
    torch.cuda.synchronize()
    name = net.dominant_kernel(batch)[0]
    assert name.startswith("k_trunk16h_w16<%d, 4, 0>" % B) and "2 products" in name, name
    assert net.products(3) == (3, True)
    p3, v3 = (t.clone() for t in net(x))
    torch.cuda.synchronize()
    name = net.dominant_kernel(batch)[0]
    assert name.startswith("k_trunk16h<%d, 4, 0>" % B) and "3 products" in name, name
    assert torch.equal(p2, p3) and torch.equal(v2, v3), "the two-product kernel differs from the three-product kernel on fp16 weights"
    assert net.status() == 0
    net.close()
    r64, r32 = R.pool_reference(nb, B, 128, True)
    el, ez = R.units(nb, B, 128, True, m)
    p, v = p2.cpu().double().numpy(), v2.cpu().double().numpy().reshape(-1)
    lp = np.log(p)
    err_l = float(np.abs(lp - lp.mean(axis=1, keepdims=True) - r64["logits"][m]).max())
    err_z = float(np.abs(np.arctanh(v) - r64["z"][m]).max())
    dp = float(np.abs(p - r32["p"][m]).max())
    dv = float(np.abs(v - r32["v"][m]).max())
    assert dp < TOL and dv < TOL, (dp, dv)
    assert err_l <= MULT * el and err_z <= MULT * ez, (err_l / el, err_z / ez)


@pytest.mark.parametrize("B", WIDTHS)
def test_rows_handed_to_the_heads_do_not_leak_from_the_previous_forward(B, monkeypatch):
    """The last layer's last two output rows exist in LDS only: their place in HBM keeps the ResBlock's input, or whatever an
    earlier forward left there. Two forwards in a row return the same bits; so does a forward after the per-layer kernels
    (mode 6, which store every row) ran on OTHER boards in the same workspace, and one after a larger batch."""
    import torch
    nb, batch = 2, 17
    m = R.batch_indices(batch, B)
    pool = R.pool(B)
    x = torch.from_numpy(pool[m]).cuda()
    other = torch.from_numpy(pool[(m + 29) % len(pool)]).cuda()
    big = torch.from_numpy(pool[np.arange(48) % len(pool)]).cuda()
    net = _resident_net(monkeypatch, nb, B, False)
    p0, v0 = (t.clone() for t in net(x))
    p1, v1 = (t.clone() for t in net(x))
    torch.cuda.synchronize()
    assert net.dominant_kernel(batch)[0].startswith("k_trunk16h<%d, 4, 0>" % B)
    assert torch.equal(p0, p1) and torch.equal(v0, v1), "two forwards in a row differ"
    net.set_mode(6)
    net(other)
    net.set_mode(5)
    p2, v2 = (t.clone() for t in net(x))
    torch.cuda.synchronize()
    assert torch.equal(p0, p2) and torch.equal(v0, v2), "a forward depends on what the per-layer kernels left in the activation buffers"
    net(big)
    p3, v3 = (t.clone() for t in net(x))
    torch.cuda.synchronize()
    assert torch.equal(p0, p3) and torch.equal(v0, v3), "a forward depends on what a larger batch left in the activation buffers"
    assert net.status() == 0
    net.close()
