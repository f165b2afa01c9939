"""CPU: the host side of per-game budgets, settling and playout-cap randomisation -- utils.move_decided (the rule k_settle
applies on the device), main.full_search (which plies are searched fully) and the declarations of the new C calls."""
import itertools
import os
import re

import numpy as np

from conftest import REPO

NEW_SYMBOLS = {"ao_begin_move_opts": 4, "ao_settle": 4, "ao_search_opts": 11, "ao_search_sims": 5}   # name -> arguments


def test_move_decided_means_the_leader_cannot_be_caught_or_tied():
    """Random visit vectors, every way of adding `remaining` visits one at a time (as multisets over the children): where the
    rule holds the argmax is unchanged and unique in every outcome; where it does not and the root has a second child, some
    outcome ties or overtakes the leader -- the rule is exact there, not merely safe (an only child cannot be caught by anybody:
    with n2 = 0 the rule is merely safe for it)."""
    from alpha_omok_amd.utils import move_decided
    rs = np.random.RandomState(5)
    held = failed = 0
    for case in range(400):
        k = int(rs.randint(1, 6))
        v = rs.randint(0, 9, size=k)
        if case % 3 == 0:
            v[int(rs.randint(k))] += int(rs.randint(0, 12))            # a clear leader now and then
        r = int(rs.randint(0, 5))
        lead = int(np.argmax(v))
        outcomes = []
        for add in itertools.combinations_with_replacement(range(k), r):
            w = v.copy()
            for a in add:
                w[a] += 1
            outcomes.append(w)
        stays = all(int(np.argmax(w)) == lead and int((w == w.max()).sum()) == 1 for w in outcomes)
        decided = move_decided(v, r)
        assert stays if decided else (k == 1 or not stays), (v.tolist(), r, decided, stays)
        held += int(decided)
        failed += int(not decided)
    assert held >= 40 and failed >= 40, (held, failed)


def test_move_decided_edges():
    from alpha_omok_amd.utils import move_decided
    assert move_decided([9, 5, 0], 3) and not move_decided([9, 5, 0], 4)     # n1 - n2 == remaining: the runner-up can still tie
    w = np.array([9, 5, 0])
    w[1] += 4
    assert int((w == w.max()).sum()) == 2                                   # ... and argmax_onehot would draw among two
    assert move_decided([7], 6) and not move_decided([7], 7)                 # one child: n2 = 0
    assert not move_decided(np.zeros(81), 0) and not move_decided([], 0)     # no visits (an unexpanded root): never decided
    assert not move_decided([4, 4, 1], 0)                                    # a tie with nothing owed stays a tie
    assert move_decided(np.array([[0., 3.], [40., 1.]]), 36)                 # any shape, float counts (the visit vector of get_pi)


def test_full_search_is_a_fixed_function_of_seed_episode_and_ply():
    """The playout-cap choice: splitmix64 over (seed, episode, ply), restated here with Python integers; the exact number of
    full searches over 100 episodes x 100 plies for two seeds."""
    from alpha_omok_amd import main
    M = (1 << 64) - 1

    def mix(x):
        x = (x + 0x9E3779B97F4A7C15) & M
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
        return x ^ (x >> 31)

    ep = np.repeat(np.arange(100), 100)
    ply = np.tile(np.arange(100), 100)
    np.random.seed(1)
    before = np.random.get_state()[1].copy()
    full = main.full_search(7, ep, ply, 0.25)
    assert np.array_equal(np.random.get_state()[1], before)                  # np.random is not drawn from
    assert full.dtype == bool and full.shape == (10000,)
    assert int(full.sum()) == 2522
    assert int(main.full_search(0, ep, ply, 0.25).sum()) == 2494
    ref = [(mix(mix(mix(7) ^ e) ^ p) >> 11) * 2.0 ** -53 < 0.25 for e in range(100) for p in range(100)]
    assert full.tolist() == ref
    # scalars, any order of asking, other shapes: the same answers
    assert [bool(main.full_search(7, int(e), int(p), 0.25)) for e, p in zip(ep[::97], ply[::97])] == full[::97].tolist()
    assert np.array_equal(main.full_search(7, ep[::-1], ply[::-1], 0.25), full[::-1])
    assert np.array_equal(main.full_search(7, ep.reshape(100, 100), ply.reshape(100, 100), 0.25), full.reshape(100, 100))
    assert main.full_search(7, ep, ply, 1.0).all() and not main.full_search(7, ep, ply, 0.0).any()
    # a higher probability only adds full searches
    assert (main.full_search(7, ep, ply, 0.5) | ~full).all()


def test_configure_refuses_bad_playout_cap_arguments():
    import pytest
    from alpha_omok_amd import main
    with pytest.raises(ValueError):
        main.configure(board_size=9, n_mcts=16, fast_sims=17)
    with pytest.raises(ValueError):
        main.configure(board_size=9, n_mcts=16, fast_sims=0)
    with pytest.raises(ValueError):
        main.configure(board_size=9, n_mcts=16, fast_sims=4, full_prob=1.5)


def test_new_calls_are_declared_bound_and_exported():
    from alpha_omok_amd import _lib
    hdr = open(os.path.join(REPO, "include", "omok_hip.h")).read()
    for name, nargs in NEW_SYMBOLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, hdr)
        assert m, "omok_hip.h does not declare %s" % name
        assert len(m.group(1).split(",")) == nargs, name
        assert name in _lib.SYMBOLS, "_lib.SYMBOLS lacks %s" % name
        assert len(_lib.SYMBOLS[name][1]) == nargs
    assert "utils.move_decided" in hdr                                      # the header cites the host definition of the rule
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
    assert lib.ao_abi_version() == 2                                         # additive change
