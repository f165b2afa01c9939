"""CPU: the networks and boards of the fp16-range tests (tests/fp16_range_nets.py) are what tests/test_gpu_fp16_range.py and
tests/test_gpu_fp16_range_search.py take them for, in the float64 reference:

  * a dead-channel network with its channel scaled by 2^20 IS the dead network, to 0.0 in centred logits and z, with and without
    the clamp at 65504 on every stored activation -- and not the network it was made from;
  * which boards of the pools are OVER (a stored activation above 2 x 65504) and UNDER (all below 65504 / 2): every batch that
    must raise the flag holds an over board, every shape that gets an under-only batch has under boards;
  * the stem detector stores exactly one activation of k on the chosen board, cell and channel, k + O(1) in the residual stores
    of that channel, and nothing else above 65504 / 2;
  * the sweep's subset at 3073 boards keeps every row, cell and channel; the families name every kernel of the guard."""
import numpy as np
import pytest

import fp16_range_nets as N
import net_reference as R

SHAPES = sorted({(f.nb, f.B, f.grid) for f in N.FAMILIES})


@pytest.mark.parametrize("nb,B,grid", SHAPES, ids=["nb%d-B%d-%s" % (nb, B, "w16grid" if g else "w32") for nb, B, g in SHAPES])
def test_big_network_is_the_dead_network_exactly(nb, B, grid):
    x = R.pool(B)[:24]
    base = R.forward(R.case_network(nb, B, 128, grid), x)
    _, r32 = R.pool_reference(nb, B, 128, grid)
    for kind in N.KINDS:
        big, dead = N.big_network(nb, B, kind, grid), N.dead_network(nb, B, kind, grid)
        d = R.forward(dead, x)
        assert R.distances(R.forward(big, x), d) == (0.0, 0.0)
        assert R.distances(R.forward(big, x, act_round=N.clamp), d) == (0.0, 0.0)
        # cutting the channel off changes the function by far more than any bound the GPU tests allow (16 x E32, E32 about 1e-5):
        # the dead network's reference cannot be met by a kernel that evaluates the original network
        dl, dz = R.distances(d, base)
        assert dl > 0.02, (kind, dl, dz)
        if grid:
            for k, v in big.items():
                if v.ndim == 4 and v.shape[2] == 3:
                    assert np.array_equal(v.astype(np.float16).astype(np.float32), v), k


@pytest.mark.parametrize("fam", N.FAMILIES, ids=[f.id for f in N.FAMILIES])
def test_every_batch_has_the_boards_its_case_needs(fam):
    m = N.batch(fam)
    assert len(m) == fam.batch
    if fam.f16:
        assert N.fp16_planes(R.pool(fam.B)[np.unique(m)]).all()
    for kind in N.KINDS:
        over, under = N.kinds_of_pool(fam.nb, fam.B, kind, fam.grid)
        assert not (over & under).any()
        assert over[m].any(), (fam.id, kind)
        if N.has_under(fam.B, kind):
            mu = N.under_batch(fam, kind)
            assert len(mu) == fam.batch and under[mu].all() and not over[mu].any()
            assert N.fp16_planes(R.pool(fam.B)[np.unique(mu)]).all()
    # both kinds of board on the shapes that test the two in one pool
    if fam.B == 4:
        assert all(N.has_under(4, kind) for kind in N.KINDS)


def test_over_and_under_keep_a_factor_of_two_from_the_limit():
    pk = N.stored_peaks(N.big_network(2, 10, "inner"), R.pool(10))
    over, under = N.kinds_of_pool(2, 10, "inner")
    assert (pk[over] > 2 * N.LIMIT).all() and (pk[under] < N.LIMIT / 2).all() and over.sum() >= 40 and under.sum() >= 2
    # the ordinary networks stay far inside the range on every board
    for nb, B, grid in SHAPES:
        assert N.stored_peaks(R.case_network(nb, B, 128, grid), R.pool(B)).max() < 1000


@pytest.mark.parametrize("B", [9, 4, 7, 10])
def test_stem_detector_stores_one_activation_of_k(B):
    import torch
    base = R.case_network(2, B, 128)
    quiet = N.quiet_pool(B)
    for c, cell in zip(N.CHANNELS, N.sweep_cells(B)):
        x = np.concatenate([quiet[:12], N.detector_board(B, cell)[None]])
        for k in (N.DETECT_OVER, N.DETECT_IN):
            sd = N.stem_detector(base, c, k)
            acts = []
            R.forward(sd, x, act_round=lambda t: (acts.append(t.clone()), t)[1])
            stem = acts[0][:, c]
            want = torch.zeros_like(stem)
            want[12, cell // B, cell % B] = k
            # one activation of k (the library's float fold is k itself, the float64 one is 7e-9 off), exact zeros elsewhere
            assert torch.equal(stem != 0, want != 0) and (stem - want).abs().max() < 1e-3
            for i, a in enumerate(acts):
                others = torch.cat([a[:, :c], a[:, c + 1:]], dim=1)
                assert others.max() < 1000                               # nothing else comes near 65504 / 2
                assert a[:12, c].max() < 1000
                if i % 2 == 0:                                           # the stem and every residual store carry k + O(1)
                    assert abs(a[12, c, cell // B, cell % B].item() - k) < 100
                    a[12, c, cell // B, cell % B] = 0
                assert a[12, c].max() < 1000
            # ... and the outputs do not depend on k
        o = [R.forward(N.stem_detector(base, c, k), x) for k in (N.DETECT_OVER, N.DETECT_IN)]
        assert R.distances(o[0], o[1]) == (0.0, 0.0)
    assert N.DETECT_OVER - 100 > N.LIMIT > N.DETECT_IN + 100


def test_the_sweep_keeps_every_row_cell_and_channel():
    for B, batch in sorted({(f.B, f.batch) for f in N.FAMILIES}):
        pts = N.sweep_points(B, batch)
        rows, cells = N.sweep_boards(batch), N.sweep_cells(B)
        assert {p[0] for p in pts} == set(rows) and {p[1] for p in pts} == set(cells) and {p[2] for p in pts} == set(N.CHANNELS)
        assert batch - 1 in rows and 0 in rows and len(cells) == 5
        if batch >= 3073:
            assert 2 * len(pts) <= 40 and rows == [0, 15, 16, batch - 1]
        else:
            assert len(pts) == len(rows) * len(cells) * len(N.CHANNELS)


def test_the_families_cover_every_kernel_name_of_the_guard():
    """Every family the guard is described with, its two-product form where one exists and the three one-product forms -- and
    ao_net_plan_kernel plans that kernel for the family's shape, batch and mode (the _w16 / _f16 forms are the same plan on
    fp16 weights / under Net.precision)."""
    from alpha_omok_amd.engine import plan_kernel
    have = {f.kernel for f in N.FAMILIES}
    assert set(N.NAMED) <= have, set(N.NAMED) - have
    ids = [f.id for f in N.FAMILIES]
    assert len(ids) == len(set(ids))
    for f in N.FAMILIES:
        head, _, tail = f.kernel.partition("<")
        assert R.is_split_fp16(f.kernel) or head in ("k_trunk16h_f16", "k_boardh_f16", "k_layer16h_f16"), f.kernel
        assert head.endswith("_w16") == (f.grid and not f.f16) and head.endswith("_f16") == f.f16
        plain = head.replace("_w16", "").replace("_f16", "") + "<" + tail
        if f.env.get("AO_TRUNK_FMT") == "1":
            plain = plain.replace(", 4, 1>", ", 4, 0>")                  # (the plan knows nothing of the environment)
        name = plan_kernel(f.nb, 5, 128, f.B, f.batch, in_kind=1, trunk_mode=f.mode)[0]
        assert name.startswith(plain), (f.id, name)
    for B, G, S, kernel in N.SEARCH_FAMILIES:
        assert plan_kernel(2, 5, 128, B, G, in_kind=2)[0].startswith(kernel), (B, G, kernel)
    assert {s[3].split("<")[0] for s in N.SEARCH_FAMILIES} == {"k_trunk16hb", "k_boardh", "k_conv_cells_h"}


def test_check_visits_accepts_a_repeated_ply_of_a_plain_search():
    """main._check_visits (strict mode) after a move that the search repeated on the fp32-MFMA trunk: nothing inherited, the plain
    budget -- two scalars, which it must compare with the visit sums as an array (it raised IndexError on its own error path)."""
    import alpha_omok_amd.main as main
    from alpha_omok_amd.engine import EngineError

    class Eng:
        ev = 0

        def fp16_range_events(self):
            return self.ev, 0

    eng, S, A = Eng(), 8, 9
    keep = main.N_MCTS
    main.N_MCTS = S
    try:
        on, act = np.array([0, 2]), np.array([1, 0, 3])
        vis = np.zeros((3, A))
        vis[:, 1], vis[:, 3] = 5, 3
        inherit = np.array([4, 4, 4], np.int64)
        eng.ev = 1                                                   # an event since the last look: fresh trees, S visits
        assert main._check_visits(eng, vis, act, on, inherit, 0) == 1
        assert inherit.tolist() == [4, 4, 2]
        inherit[:] = 4
        with pytest.raises(EngineError, match="8 visits, 12 expected"):   # no event: the inherited visits are missing
            main._check_visits(eng, vis, act, on, inherit, 1)
        vis[:, 1] += 4
        assert main._check_visits(eng, vis, act, on, inherit, 1) == 1
        eng.ev = 2
        with pytest.raises(EngineError, match="12 visits, 8 expected"):   # an event, and visits that are not the budget
            main._check_visits(eng, vis, act, on, inherit, 1)
    finally:
        main.N_MCTS = keep
