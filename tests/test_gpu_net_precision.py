"""-m gpu: every kernel family of the network forward, named, at its seams, against a plain float64 reference in logit space.

The other forward tests compare (p, v) after softmax and tanh with torch fp32 at 1e-4, on golden-vector weights whose value
head is dead and whose policy is nearly one-hot (tests/net_reference.py has the table). Here the networks are conditioned
(net_reference.conditioned_state_dict; tests/test_net_reference.py asserts on the CPU that every case is), the device's
p and v are read back as centred log p and atanh v, and the distance to the float64 reference is bounded in units of what
float32 itself loses on that case:

    E32_l, E32_z = the same two distances between the plain reference run in float32 and in float64 (floor 1e-6 each)
    allowed: 4 x E32 for the kernels that are fp32 throughout, 16 x E32 for the split-fp16 families (net_reference.Case.mult)

The bound comes from the reference, never from the kernel under test. tests/test_net_reference.py shows on the CPU that each
of eleven small defects of the reference, and of conv1 defects per input plane, passes twice this bound on every case. The
measured err / E32 per family and case is kept in profiles/r7a_forward_precision_by_family.txt, that of the cases with
another number of input planes than 5 (net_reference.INPLANES) in profiles/r17a_forward_precision_by_inplanes.txt; with
AO_PRECISION_REPORT=<file> each case appends its figures as a JSON line.

Every batch is made of boards of one pool per board size (net_reference.pool: structured boards -- empty, full, one stone in
each corner and on each edge, float planes that are not 0/1 -- and random 0/1 planes), so one float64 evaluation of the pool
serves every case of a network and EVERY board of a batch is compared, the 4096-board ones included."""
import json
import os

import numpy as np
import pytest

import net_reference as R

pytestmark = pytest.mark.gpu
TOL = 1e-4      # the project's stated contract on (p, v), BASELINE.json north_star: kept beside the logit-space bound


@pytest.mark.parametrize("case", R.CASES, ids=[c.id for c in R.CASES])
def test_kernel_family_against_float64_in_logit_space(case, monkeypatch):
    import torch
    from alpha_omok_amd.engine import Net
    from alpha_omok_amd.pvnet import native_width, pad_state_dict
    sd = R.case_network(*case.net_key())
    m = case.boards()
    x = torch.from_numpy(R.pool(case.B, case.C)[m]).cuda()
    width = native_width(case.planes)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    net = Net(case.nb, case.C, width, case.B, 0)
    for k in case.env:
        monkeypatch.delenv(k)
    net.load_state_dict(sd if width == case.planes else pad_state_dict(sd, width))
    net.set_mode(case.mode)
    if width == 128 and case.nb >= 1:
        assert net.products() == (case.products, case.grid), net.products()
    p, v = net(x)
    torch.cuda.synchronize()
    name = net.dominant_kernel(case.batch)[0]
    assert name.startswith(case.kernel), (name, case.kernel)
    if R.is_split_fp16(case.kernel):
        assert ("2 products" if "_w16<" in case.kernel else "3 products") in name, name
    p2, v2 = net(x)
    torch.cuda.synchronize()
    assert torch.equal(p, p2) and torch.equal(v, v2), "two forwards of the same batch differ"
    assert net.status() == 0
    net.close()
    p, v = p.cpu().double().numpy(), v.cpu().double().numpy()
    assert np.isfinite(p).all() and np.isfinite(v).all() and p.min() > 0 and np.abs(v).max() < 1
    r64, _ = R.pool_reference(*case.net_key())
    el, ez = R.units(case.nb, case.B, case.planes, case.grid, m, case.C)
    lp = np.log(p)
    err_l = float(np.abs(lp - lp.mean(axis=1, keepdims=True) - r64["logits"][m]).max())
    err_z = float(np.abs(np.arctanh(v) - r64["z"][m]).max())
    dp = float(np.abs(p - r64["p"][m]).max())
    dv = float(np.abs(v - r64["v"][m]).max())
    rec = dict(id=case.id, family=case.family, kernel=name.split(" (")[0], nb=case.nb, B=case.B, planes=case.planes, C=case.C, batch=case.batch,
               mode=case.mode, grid=case.grid, mult=case.mult, E32_l=el, E32_z=ez, err_l=err_l, err_z=err_z,
               ratio_l=err_l / el, ratio_z=err_z / ez, dp=dp, dv=dv)
    print("PRECISION " + json.dumps(rec))
    if os.environ.get("AO_PRECISION_REPORT"):
        with open(os.environ["AO_PRECISION_REPORT"], "a") as f:
            f.write(json.dumps(rec) + "\n")
    assert dp < TOL and dv < TOL, (dp, dv)
    assert err_l <= case.mult * el and err_z <= case.mult * ez, \
        "%s: centred logits off by %.2f x E32 (%.2e), atanh v by %.2f x E32 (%.2e); allowed %d x" % (
            name.split(" (")[0], err_l / el, err_l, err_z / ez, err_z, case.mult)
