"""-m gpu: the device buffers the C ABI takes from its caller. Each one is carved out of a larger uint8 tensor -- 64 KiB of a
known byte on each side, the payload 256-byte aligned -- and passed by pointer.

  * outputs: after the call both margins still hold their byte (0xA5): ao_net_forward's policy and value for whole and ragged
    batches, ao_replay_gather's states / pi / z, ao_collect_leaves' planes, ao_positions_from_moves' planes, and the log of
    ao_set_eval_log, where nothing may be written past capacity_floats either;
  * inputs: the same payload gives the same bits whether 0xFF bytes or zeros surround it: ao_net_forward's planes in every
    kernel family, ao_apply_evals' policy and value.

No guard mode is involved: the margins belong to the test."""
import ctypes as C

import numpy as np
import pytest

import net_reference as R
from test_gpu_memory_guard import FAMILY_CASES, _make_net

pytestmark = pytest.mark.gpu

MARGIN = 65536


class Carved:
    """`nbytes` of payload between two margins of `surround` bytes; the payload starts as `surround` too."""

    def __init__(self, nbytes, surround=0xA5):
        import torch
        self.nbytes, self.surround = int(nbytes), surround
        self.raw = torch.full((2 * MARGIN + self.nbytes,), surround, dtype=torch.uint8, device="cuda")
        assert (self.raw.data_ptr() + MARGIN) % 256 == 0

    @property
    def ptr(self):
        return self.raw.data_ptr() + MARGIN

    def payload(self, dtype, shape):
        return self.raw[MARGIN:MARGIN + self.nbytes].view(dtype).view(*shape)

    def put(self, tensor):
        self.raw[MARGIN:MARGIN + self.nbytes].copy_(tensor.contiguous().view(-1).view(self.raw.dtype))
        return self

    def margins_intact(self):
        import torch
        torch.cuda.synchronize()
        return bool((self.raw[:MARGIN] == self.surround).all()) and bool((self.raw[MARGIN + self.nbytes:] == self.surround).all())


IDS = [c.kernel.replace(" ", "") for c in FAMILY_CASES]


@pytest.mark.parametrize("case", FAMILY_CASES, ids=IDS)
def test_net_forward_writes_policy_and_value_inside_their_buffers(case, monkeypatch):
    import torch
    net, _ = _make_net(case, monkeypatch)
    try:
        A = case.B * case.B
        for batch in (case.batch, case.batch + 1):               # whole and ragged
            x = torch.from_numpy(R.pool(case.B, case.C)[R.batch_indices(batch, case.B, case.C)]).cuda()
            p0, v0 = net(x)
            pol, val = Carved(batch * A * 4), Carved(batch * 4)
            net.forward_ptr(x.data_ptr(), batch, pol.ptr, val.ptr, torch.cuda.current_stream().cuda_stream)
            assert pol.margins_intact(), "policy of %d boards" % batch
            assert val.margins_intact(), "value of %d boards" % batch
            assert torch.equal(pol.payload(torch.float32, (batch, A)), p0) and torch.equal(val.payload(torch.float32, (batch,)), v0)
        assert net.status() == 0
    finally:
        net.close()


@pytest.mark.parametrize("case", FAMILY_CASES, ids=IDS)
def test_net_forward_reads_nothing_around_its_planes(case, monkeypatch):
    import torch
    net, _ = _make_net(case, monkeypatch)
    try:
        for batch in (case.batch, case.batch + 1):
            x = torch.from_numpy(R.pool(case.B, case.C)[R.batch_indices(batch, case.B, case.C)]).cuda()
            res = []
            for surround in (0xFF, 0x00):
                planes = Carved(x.numel() * 4, surround).put(x)
                p = torch.empty((batch, case.B * case.B), dtype=torch.float32, device="cuda")
                v = torch.empty((batch,), dtype=torch.float32, device="cuda")
                net.forward_ptr(planes.ptr, batch, p.data_ptr(), v.data_ptr(), torch.cuda.current_stream().cuda_stream)
                assert planes.margins_intact()
                res.append((p, v, net.status()))
            assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and res[0][2] == res[1][2], \
                "%d boards: the result depends on the bytes around the planes" % batch
            p0, v0 = net(x)
            assert torch.equal(res[0][0], p0) and torch.equal(res[0][1], v0)
    finally:
        net.close()


@pytest.mark.parametrize("B,cap", [(15, 37), (3, 8)])
def test_replay_gather_writes_inside_its_buffers(B, cap):
    import torch
    from alpha_omok_amd.replay import DeviceReplay
    from test_gpu_replay import _samples
    rs = np.random.RandomState(B + cap)
    mem = DeviceReplay(B, 5, cap)
    try:
        for n in (3, 7, 2):
            mem.extend_augmented(_samples(rs, n, B))
        idx = np.ascontiguousarray(rs.randint(0, len(mem), size=19), np.int64)
        s0, pi0, z0 = mem.batch(idx)
        A, m = B * B, idx.size
        s, pi, z = Carved(m * 5 * A * 4), Carved(m * A * 4), Carved(m * 4)
        rc = mem._L.ao_replay_gather(mem._h, idx.ctypes.data_as(C.POINTER(C.c_int64)), m, s.ptr, pi.ptr, z.ptr,
                                     torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        assert s.margins_intact() and pi.margins_intact() and z.margins_intact()
        assert torch.equal(s.payload(torch.float32, (m, 5, B, B)), s0) and torch.equal(pi.payload(torch.float32, (m, A)), pi0)
        assert torch.equal(z.payload(torch.float32, (m,)), z0)
    finally:
        mem.close()


def _stepwise(eng, planes_ptr, planes_view, policy, value, oracle, sims=None):
    """One move of the step-wise protocol with the oracle's stub evaluator; policy / value are the device tensors
    ao_apply_evals reads. Returns end_move's outputs and the planes of every collect."""
    import torch
    seen = []
    eng.begin_move()
    while eng.sims_left() > 0 and (sims is None or len(seen) < sims):
        eng.collect_leaves(planes_ptr)
        eng.sync()
        pl = planes_view.cpu().numpy()
        seen.append(pl)
        pv = [oracle.stub_eval(pl[g], 0) for g in range(eng.G)]
        policy.copy_(torch.from_numpy(np.stack([p for p, _ in pv]).astype(np.float32)))
        value.copy_(torch.from_numpy(np.array([v for _, v in pv], np.float32)))
        torch.cuda.synchronize()
        eng.apply_evals(policy.data_ptr(), value.data_ptr())
    return (eng.end_move(np.ones(eng.G, np.int8)) if sims is None else None), seen


@pytest.mark.parametrize("B,G,S", [(9, 5, 24), (15, 3, 24)])
def test_collect_leaves_writes_inside_its_planes(B, G, S, oracle):
    import torch
    from alpha_omok_amd.engine import Engine
    A = B * B
    engs = [Engine(B, S, 5, games=G, noise=True, node_cap=4 * (S + 1)) for _ in range(2)]
    try:
        for e in engs:
            e.seed_all(np.arange(900, 900 + G, dtype=np.uint32))
        pol, val = torch.zeros((G, A), device="cuda"), torch.zeros((G,), device="cuda")
        carved = Carved(G * 5 * A * 4)
        plain = torch.zeros((G, 5, B, B), device="cuda")
        out_c, seen_c = _stepwise(engs[0], carved.ptr, carved.payload(torch.float32, (G, 5, B, B)), pol, val, oracle)
        assert carved.margins_intact()
        out_p, seen_p = _stepwise(engs[1], plain.data_ptr(), plain, pol, val, oracle)
        assert len(seen_c) == len(seen_p) == S + 1             # a fresh root's own expansion, then S simulations
        for a, b in zip(seen_c, seen_p):
            np.testing.assert_array_equal(a, b)
        for a, b in zip(out_c, out_p):
            np.testing.assert_array_equal(a, b)
    finally:
        for e in engs:
            e.close()


@pytest.mark.parametrize("B,G,S", [(9, 5, 24), (15, 3, 24)])
def test_apply_evals_reads_nothing_around_policy_and_value(B, G, S, oracle):
    import torch
    from alpha_omok_amd.engine import Engine
    A = B * B
    res = []
    for surround in (0xFF, 0x00):
        eng = Engine(B, S, 5, games=G, noise=True, node_cap=4 * (S + 1))
        try:
            eng.seed_all(np.arange(900, 900 + G, dtype=np.uint32))
            pol, val = Carved(G * A * 4, surround), Carved(G * 4, surround)
            planes = torch.zeros((G, 5, B, B), device="cuda")
            out, _ = _stepwise(eng, planes.data_ptr(), planes, pol.payload(torch.float32, (G, A)), val.payload(torch.float32, (G,)), oracle)
            assert pol.margins_intact() and val.margins_intact()
            res.append(out + tuple(np.concatenate([eng.root_children(g)[k] for g in range(G)]) for k in ("action", "n", "w", "q", "p")))
        finally:
            eng.close()
    for a, b in zip(*res):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("B", (3, 9, 15))
def test_positions_from_moves_writes_inside_its_planes(B):
    import torch
    from alpha_omok_amd.positions import PositionBatch
    from test_gpu_memory_guard import _position_ids
    ids = _position_ids(B, np.random.RandomState(40 + B))
    with PositionBatch(B, capacity=7) as pb:
        want = pb.planes(ids)
        carved = Carved(len(ids) * 5 * B * B * 4)
        pb._from_moves(ids, True, False, lambda cnt: carved.ptr)
        assert carved.margins_intact()
        assert torch.equal(carved.payload(torch.float32, (len(ids), 5, B, B)), want)


def test_eval_log_stops_at_its_capacity():
    import pvnet_weights
    import torch
    from alpha_omok_amd.engine import Engine, Net
    B, G, S = 9, 5, 24
    A = B * B
    games = [0, 2]
    rec = len(games) * (A + 3)
    capacity = 5 * rec + 50                                  # five launches and a part of a sixth: fewer than the search runs
    net = Net(2, 5, 128, B, 0)
    eng = Engine(B, S, 5, games=G, noise=True, node_cap=4 * (S + 1))
    try:
        net.load_state_dict(pvnet_weights.make_state_dict(2, 5, 128, B, 7))
        eng.seed_all(np.arange(G, dtype=np.uint32))
        log = Carved(capacity * 4)
        eng.set_eval_log(games, log.ptr, capacity)
        eng.search(net, tau=np.ones(G, np.int8))
        eng.sync()
        assert log.margins_intact()
        n = eng.eval_log_count()
        assert 1 <= n <= 5, n
        raw = log.raw[MARGIN:MARGIN + capacity * 4]
        assert bool((raw[n * rec * 4:] == 0xA5).all()), "something was written past the last whole record"
        rows = log.payload(torch.float32, (capacity,))[:n * rec].view(n, len(games), A + 3).cpu().numpy()
        assert np.isfinite(rows).all() and set(np.unique(rows[:, :, A + 2]).tolist()) <= {0.0, 1.0, 2.0, 3.0, 4.0, 5.0}
        eng.set_eval_log([], None, 0)
    finally:
        eng.close()
        net.close()
