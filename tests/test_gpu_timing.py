"""-m gpu: the HIP-event timing rings behind Engine.tree_timing (ao_tree_timing, 256 event pairs) and Net.conv_timing
(ao_net_conv_timing, 512 pairs), which bench.py takes its kernel times from. A 5x5 board, 2 games, a one-block 32-plane network:
the per-board path, where a search launches per simulation one tree kernel and one forward with two timed trunk convs.

Checked: more timed launches than twice the ring holds are all counted (the ring harvests its older half whenever it is full), a
read resets, a disabled timer counts nothing, and with stride 3 every third tick is timed. The tree timer ticks per launch, so a
search of n launches counts ceil(n / 3); the net's ticks per FORWARD and times each of that forward's k trunk convs, so the same
search counts k * ceil(n / 3), not ceil(k * n / 3)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, S, G = 5, 200, 2
TREE_RING, NET_RING = 256, 512


def test_timing_rings_count_every_timed_launch():
    import pvnet_weights
    from alpha_omok_amd.engine import Engine, Net
    net = Net(1, 5, 32, B, 0)
    net.load_state_dict(pvnet_weights.make_state_dict(1, 5, 32, B, 3))
    eng = Engine(B, S, 5, games=G, noise=True)
    eng.seed_all([41, 42])
    tau = np.ones(G, np.int8)

    def move():
        eng.search(net, tau=tau)
        _, win = eng.play()
        assert (win == 0).all()   # six plies at the most on a 5x5 board with five in a row: no game can have ended

    # enabling reads (and resets) what was there: nothing
    assert eng.tree_timing(1) == (0.0, 0)
    assert net.conv_timing(1) == (0.0, 0)
    for _ in range(3):
        move()
    t_ms, t_n = eng.tree_timing(1)
    c_ms, c_n = net.conv_timing(1)
    print("three moves of %d simulations: tree %d launches %.3f ms, convs %d launches %.3f ms" % (S, t_n, t_ms, c_n, c_ms))
    assert t_n > 2 * TREE_RING and c_n > 2 * NET_RING
    assert math.isfinite(t_ms) and t_ms > 0.0 and math.isfinite(c_ms) and c_ms > 0.0
    assert c_n % t_n == 0     # one forward per tree launch, the same number of timed convs in each
    k = c_n // t_n
    # a read resets
    assert eng.tree_timing(0) == (0.0, 0)
    assert net.conv_timing(0) == (0.0, 0)
    # disabled (by the two reads above): a search leaves both at zero
    move()
    assert eng.tree_timing(1) == (0.0, 0)
    assert net.conv_timing(1) == (0.0, 0)
    # stride 1 against stride 3 over one move each, both from an expanded root: the same number of launches
    move()
    _, n1 = eng.tree_timing(3)
    _, c1 = net.conv_timing(3)
    move()
    t3_ms, n3 = eng.tree_timing(0)
    c3_ms, c3 = net.conv_timing(0)
    print("one move: stride 1 tree %d convs %d, stride 3 tree %d convs %d" % (n1, c1, n3, c3))
    assert n1 == S and c1 == k * n1
    assert n3 == -(-n1 // 3)
    assert c3 == k * -(-n1 // 3)
    assert t3_ms > 0.0 and c3_ms > 0.0
    eng.close()
    net.close()
