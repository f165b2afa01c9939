"""-m gpu: self-play with playout-cap randomisation (configure(fast_sims=)) and with early stop (configure(early_stop=True)):
9x9, 16 simulations, 4 in a fast search, 6 episodes, one kernel family for every batch size (reproducible=True), strict visit
accounting (every search's visits sum to inherited + the simulations it ran)."""
import numpy as np
import pytest

import pvnet_weights

pytestmark = pytest.mark.gpu

B, S, FAST, N, SEED = 9, 16, 4, 6, 11
A = B * B


def _model():
    import torch
    from alpha_omok_amd.pvnet import PVNet
    model = PVNet(1, 5, 128, B)                      # (128 planes: what the one-kernel-family mode of reproducible=True takes)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in pvnet_weights.make_state_dict(1, 5, 128, B, 5).items()})
    return model.cuda().eval()


def _configure(main, slots, **kw):
    main.MAX_CONCURRENT = slots
    main.configure(board_size=B, n_mcts=S, model=_model(), seed=SEED, strict=True, reproducible=True, **kw)
    main.cur_memory.clear()
    main.rep_memory.clear()


def test_fast_searches_play_and_only_full_searches_are_recorded():
    import alpha_omok_amd.main as main
    from alpha_omok_amd import utils
    keep = main.MAX_CONCURRENT
    try:
        runs = []
        for slots in (6, 2):
            _configure(main, slots, fast_sims=FAST, full_prob=0.25)
            runs.append(main._play_episodes(list(range(N)), False, lambda ep: (SEED + ep) & 0xFFFFFFFF, 0))
            assert main._engine.G == slots
        for x, y in zip(runs[0], runs[1]):
            np.testing.assert_array_equal(x, y)                    # the episodes do not depend on the number of concurrent slots
        moves, lengths, wins, ep_of, ply_of, pis = runs[0]
        # the recorded searches are exactly the full plies of the hash
        want = [(e, p) for e in range(N) for p in range(int(lengths[e])) if main.full_search(SEED, e, p, 0.25)]
        assert list(zip(ep_of.tolist(), ply_of.tolist())) == want
        assert 0 < len(want) < int(lengths.sum())
        assert main.playout_totals == {"full": len(want), "fast": int(lengths.sum()) - len(want)}
        for e, p, pi in zip(ep_of, ply_of, pis):
            assert abs(pi.sum() - 1) < 1e-9 and pi[moves[e, p]] > 0
            if p >= main.TAU_THRES:
                assert sorted(pi.tolist())[-2:] == [0.0, 1.0]
        # self_play: as many samples as full plies, each the position of a full ply; the summary counts both kinds
        _configure(main, 6, fast_sims=FAST, full_prob=0.25)
        out = main.self_play(N)
        cm = list(main.cur_memory)
        assert out["episodes"] == N and out["moves"] == int(lengths.sum()) and out["samples"] == len(want) == len(cm)
        for (e, p), (s, pi, z) in zip(want, cm):
            np.testing.assert_array_equal(np.asarray(s), utils.get_state_pt((0,) + tuple(int(a) for a in moves[e, :p]), B, 5))
        np.testing.assert_array_equal(np.stack([m[1] for m in cm]), pis)
        assert len(main.rep_memory) == min(8 * len(cm), main.MEMORY_SIZE)
    finally:
        main.MAX_CONCURRENT = keep
        main.configure(board_size=B, n_mcts=S, model=_model(), seed=SEED, strict=False)
        main.release_engine()


def test_early_stop_self_play_records_the_move_played():
    """early_stop=True alone: every recorded pi of a tau == 0 ply is one-hot on the move played; searches did settle; the
    tau == 1 plies (the first TAU_THRES of an episode) are the plain search's."""
    import alpha_omok_amd.engine as engine
    import alpha_omok_amd.main as main
    keep = main.MAX_CONCURRENT
    every = engine.SETTLE_EVERY
    engine.SETTLE_EVERY = 2                                         # (16 simulations: the default interval would never look)
    try:
        _configure(main, 6)
        plain = main._play_episodes(list(range(N)), False, lambda ep: (SEED + ep) & 0xFFFFFFFF, 0)
        _configure(main, 6, early_stop=True)
        moves, lengths, wins, ep_of, ply_of, pis = main._play_episodes(list(range(N)), False, lambda ep: (SEED + ep) & 0xFFFFFFFF, 0)
        ran = main._engine.sims_run()
        print("early-stop self-play: %d searches settled, %d simulations saved over %d move decisions" %
              (ran["settled_total"], ran["saved_total"], int(lengths.sum())))
        assert ep_of.shape[0] == int(lengths.sum())                 # every ply is recorded
        assert main.playout_totals == {"full": int(lengths.sum()), "fast": 0}
        for e, p, pi in zip(ep_of, ply_of, pis):
            if p >= main.TAU_THRES:
                onehot = np.zeros(A)
                onehot[moves[e, p]] = 1.0
                np.testing.assert_array_equal(pi, onehot)
        assert ran["settled_total"] > 0 and ran["saved_total"] >= ran["settled_total"]
        # up to and including the first tau == 0 ply of every episode nothing differs from the plain search: same moves, same pi
        T = main.TAU_THRES
        np.testing.assert_array_equal(moves[:, :T + 1], plain[0][:, :T + 1])
        early = ply_of <= T
        np.testing.assert_array_equal(pis[early], plain[5][plain[4] <= T])
    finally:
        engine.SETTLE_EVERY = every
        main.MAX_CONCURRENT = keep
        main.configure(board_size=B, n_mcts=S, model=_model(), seed=SEED, strict=False)
        main.release_engine()
