"""-m gpu: the layer boundary of the resident split-fp16 trunk (k_trunk16h, net_trunk_h16.hpp).

A layer of the resident trunk leaves its last two output rows in the LDS row buffers, where the next layer -- which walks the
board in the opposite direction -- finds them as its input rows 0 and 1; it neither stages them from HBM nor, for the output of
a ResBlock's first conv (which nothing else reads), are they stored to HBM at all. What can go wrong is at the boundary only:
the wrong buffer (an even board width swaps the two), the wrong direction (conv1 does not flip, the first trunk layer does), a
row that is read before it is written, a stale row of the previous forward read where a store was skipped. So the shapes are
the smallest that have every kind of boundary:

  * board widths 9 and 7 (odd: rows BW-1 / BW-2 land in buffers 0 / 1) and 8 (even: swapped, and swapped back by the next layer);
  * 1 and 2 ResBlocks: conv1 -> first conv, first conv -> second conv (intermediate tensor: no HBM store of the handed rows),
    second conv -> first conv of the next block (block output: stored), last layer -> heads (no hand-off), both directions;
  * 16 boards (one full 16-board group) and 17 (a second group with one real board).

The kernel is planned from 192 groups on; AO_FORCE_RESIDENT=1 (read when the Net is created) plans it for any batch in mode 5.

Networks, boards, reference and bound are those of tests/test_gpu_net_precision.py for the resident-trunk family: conditioned
weights (net_reference.conditioned_state_dict: live heads, an O(1) tower), boards of net_reference.pool, centred log p and
atanh v against the float64 reference within 16 x the float32-vs-float64 error of the plain evaluation on the same boards, and
(p, v) within 1e-4 of the float32 evaluation (the torch fp32 forward)."""
import numpy as np
import pytest

import net_reference as R

pytestmark = pytest.mark.gpu
TOL = 1e-4       # on (p, v) against torch fp32, as tests/test_gpu_net.py and tests/test_gpu_net_precision.py
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


@pytest.mark.parametrize("nb,B", [(nb, B) for B in WIDTHS for nb in (1, 2)])
@pytest.mark.parametrize("grid", [False, True], ids=["w32", "w16grid"])
def test_the_networks_are_conditioned(nb, B, grid):
    """The conditions tests/test_net_reference.py asserts for the networks of the precision cases, for the ones used here."""
    r = R.conditioning_report(R.case_network(nb, B, 128, grid), R.pool(B))
    assert 0.3 <= r["trunk_rms"] <= 4.0 and r["trunk_max"] < 100.0, r
    assert 1.0 <= r["logit_std"] <= 1.6 and r["p_min"] >= 1e-8, r
    assert r["z_absmax"] <= 1.5 and r["z_std"] >= 0.3, r
    assert 0.4 <= r["hp_live"] <= 0.8 and 0.4 <= r["hv_live"] <= 0.8 and 0.3 <= r["h1_live"] <= 0.7, r


@pytest.mark.parametrize("nb,B,batch", SHAPES)
def test_resident_trunk_with_handoff_against_float64_in_logit_space(nb, B, batch, monkeypatch):
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
    p, v = p.cpu().double().numpy(), v.cpu().double().numpy()
    assert p.shape == (batch, B * B) and v.reshape(-1).shape == (batch,)
    v = v.reshape(-1)
    assert np.isfinite(p).all() and np.isfinite(v).all() and p.min() > 0 and np.abs(v).max() < 1
    r64, r32 = R.pool_reference(nb, B, 128, False)
    el, ez = R.units(nb, B, 128, False, m)
    lp = np.log(p)
    err_l = float(np.abs(lp - lp.mean(axis=1, keepdims=True) - r64["logits"][m]).max())
    err_z = float(np.abs(np.arctanh(v) - r64["z"][m]).max())
    dp = float(np.abs(p - r32["p"][m]).max())
    dv = float(np.abs(v - r32["v"][m]).max())
    print("HANDOFF nb=%d B=%d batch=%d: centred logits %.2f x E32 (%.2e), atanh v %.2f x E32 (%.2e), dp %.1e, dv %.1e"
          % (nb, B, batch, err_l / el, err_l, err_z / ez, err_z, dp, dv))
    assert dp < TOL and dv < TOL, (dp, dv)
    assert err_l <= MULT * el and err_z <= MULT * ez, \
        "centred logits off by %.2f x E32 (%.2e), atanh v by %.2f x E32 (%.2e); allowed %d x" % (err_l / el, err_l, err_z / ez, err_z, MULT)


@pytest.mark.parametrize("nb,B,batch", SHAPES)
def test_two_product_resident_trunk_is_the_three_product_bits(nb, B, batch, monkeypatch):
    """k_trunk16h_w16 takes the same hand-off: on conv weights that are fp16 numbers it returns the bits of k_trunk16h (the assertion
    of tests/test_gpu_w16.py), and both are the float32-equivalent result."""
    import torch
    m = R.batch_indices(batch, B)
    x = torch.from_numpy(R.pool(B)[m]).cuda()
    net = _resident_net(monkeypatch, nb, B, True)
    assert net.products() == (2, True)
    p2, v2 = net(x)
    torch.cuda.synchronize()
    name = net.dominant_kernel(batch)[0]
    assert name.startswith("k_trunk16h_w16<%d, 4, 0>" % B) and "2 products" in name, name
    assert net.products(3) == (3, True)
    p3, v3 = net(x)
    torch.cuda.synchronize()
    name = net.dominant_kernel(batch)[0]
    assert name.startswith("k_trunk16h<%d, 4, 0>" % B) and "3 products" in name, name
    assert torch.equal(p2, p3) and torch.equal(v2, v3), "the two-product kernel differs from the three-product kernel on fp16 weights"
    assert net.products(0) == (2, True)
    assert net.status() == 0
    net.close()
    _, r32 = R.pool_reference(nb, B, 128, True)
    dp = float(np.abs(p2.cpu().double().numpy() - r32["p"][m]).max())
    dv = float(np.abs(v2.cpu().double().numpy().reshape(-1) - r32["v"][m]).max())
    assert dp < TOL and dv < TOL, (dp, dv)


@pytest.mark.parametrize("B", WIDTHS)
def test_rows_that_are_not_stored_do_not_leak_from_the_previous_forward(B, monkeypatch):
    """The handed-off rows of a ResBlock's first conv exist in LDS only: their place in HBM keeps whatever an earlier forward --
    of this or of another kernel family -- left there. Two forwards in a row from the same Net return the same bits; so does a
    forward after the per-layer kernels (mode 6, which store every row) ran on OTHER boards in the same workspace, and one
    after the workspace held the activations of a larger batch."""
    import torch
    from alpha_omok_amd.engine import Net
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
    net(big)
    net.set_mode(6)
    net(other)
    net.set_mode(5)
    p2, v2 = (t.clone() for t in net(x))
    torch.cuda.synchronize()
    assert torch.equal(p0, p2) and torch.equal(v0, v2), "a forward depends on what the previous one left in the activation buffers"
    assert net.status() == 0
    net.close()
