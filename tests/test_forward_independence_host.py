"""CPU: the checks of tests/forward_independence.py can see what they are for.

The stand-in forward is independent by construction: net_reference.forward on a small conditioned network, called once per
board with a batch of one. It passes all five checks; wrapped with each of five small defects of the kind a batched kernel can
have -- a leak from the row before, a lane that rounds differently, a ragged tail, a dependence on the batch size, a read of
the row one group back -- it fails, and which checks fail is asserted. The condition on the permutation (at least 90 % of the
rows change group and lane) is asserted for every batch size the GPU test uses."""
import functools

import numpy as np
import pytest

import forward_independence as FI
import net_reference as R

B, C = 5, 5
SIZES = (1, 3, 17, 33, 70)


@functools.lru_cache(maxsize=None)
def _network():
    """One block of 16 planes on 5x5. The seed is one on which the lively board's value logit is below 0.5 in size (asserted
    below): defect 1 adds 2^-24 of a logit of size O(1), which is a whole ulp of a float32 below 0.5, half an ulp -- rounded
    away -- of one in [0.5, 1), and the value is the one number of a row that defect touches."""
    return R.conditioned_state_dict(1, C, 16, B, 7)


def test_the_stand_in_can_show_a_leak_of_2_to_the_minus_24():
    z = float(R.forward(_network(), R.pool(B, C)[FI.lively_board(B, C)][None])["z"][0])
    assert 0.1 < abs(z) < 0.5, z


_CACHE = {}


def _one(board):
    """(p float32 [A], z float64) of one board: a batch of one through the plain reference."""
    import torch
    key = board.tobytes()
    if key not in _CACHE:
        o = R.forward(_network(), board[None])
        _CACHE[key] = (torch.softmax(o["logits"], dim=1)[0].numpy().astype(np.float32), float(o["z"][0]))
    return _CACHE[key]


def base(x):
    rows = [_one(b) for b in x]
    return np.stack([r[0] for r in rows]), np.array([r[1] for r in rows], np.float64)


def clean(x):
    p, z = base(x)
    return p, np.tanh(z).astype(np.float32)


def _ulp(a, k=1):
    return (a.view(np.uint32) + np.uint32(k)).view(np.float32)


def leak_from_the_row_before(x):
    """1: row i receives 2^-24 times row i-1's value logit"""
    p, z = base(x)
    z = z.copy()
    z[1:] += 2.0 ** -24 * z[:-1]
    return p, np.tanh(z).astype(np.float32)


def lane_15_rounds_differently(x):
    """2: rows with row % 16 == 15 are moved by one ulp"""
    p, v = clean(x)
    v[15::16] = _ulp(v[15::16])
    return p, v


def ragged_tail(x):
    """3: the last row differs when n % 16 != 0"""
    p, v = clean(x)
    if len(x) % 16:
        p[-1, :1] = _ulp(p[-1, :1])
    return p, v


def row_0_depends_on_n(x):
    """4: row 0 depends on n"""
    p, v = clean(x)
    v[:1] = _ulp(v[:1], len(x))
    return p, v


def second_group_reads_one_group_back(x):
    """5: rows of the second group read board row - 16 when the two are equal in plane C - 1"""
    x = np.array(x)
    for r in range(16, min(32, len(x))):
        if np.array_equal(x[r, C - 1], x[r - 16, C - 1]):
            x[r] = x[r - 16]
    return clean(x)


def _failures(fwd, n):
    return FI.Checker(fwd, "stand-in", n, B, C).failures()


@pytest.mark.parametrize("n", SIZES)
def test_the_clean_stand_in_passes_every_check(n):
    ck = FI.Checker(clean, "stand-in", n, B, C)
    assert ck.run() == (list(FI.CHECKS) if n > 1 else list(FI.CHECKS[:4]))
    assert FI.Checker(clean, "stand-in", n, B, C).failures() == {}


def test_the_probe_rows():
    assert FI.probe_rows(70) == [0, 15, 16, 35, 64, 69] and FI.probe_rows(33) == [0, 15, 16, 32]
    assert FI.probe_rows(64) == [0, 15, 16, 32, 48, 63] and FI.probe_rows(17) == [0, 8, 15, 16]
    assert FI.probe_rows(1) == [0] and FI.probe_rows(3) == [0, 1, 2]
    for n in (33, 70):
        for board in (FI.lively_board(B, C), FI.full_board(B, C)):
            m = FI.twins_indices(n, B, C, board)
            assert (m[FI.probe_rows(n)] == board).all() and len(set(m.tolist())) > len(FI.probe_rows(n))
    assert R.structured_boards(B, C)[1][FI.lively_board(B, C)].startswith("float planes")
    assert R.structured_boards(B, C)[1][FI.full_board(B, C)] == "full"


# which checks must see which defect and which cannot, and why; at 70 boards (five groups, the last of six rows) and at 33 (a
# last group of one row)
#   1  a probe row's predecessor is replaced (neighbours) or moved (permutation); row 0 has none, the other rows of the constant
#      batch have one (constant); the probe rows have different predecessors (twins); the rows 0 .. n-2 keep theirs (not tail)
#   2  row 15 holds the board of rows 0 and 16 (twins, constant); a board at lane 15 leaves it or comes to it (permutation); with
#      or without other boards around it, and with or without the last row, lane 15 is off by the same ulp (not neighbours, tail)
#   3  the last row holds the board of row 0 (twins, constant), another board comes to it (permutation); it is a probe row and
#      wrong by the same ulp whatever is around it (not neighbours). Without the last row, row n-2 is the last: tail, unless
#      n - 1 is a multiple of 16 (33)
#   4  tail is the one check that compares two batch sizes; row 0 is also off against the other rows that hold its board
#      (twins, constant) and the board that leaves it (permutation), but by the same n ulps among other boards (not neighbours)
#   5  row 16 reads row 0, which holds the same board in every batch of twins, constant and neighbours, and no other probe
#      row is in rows 17 .. 31; the permuted batch puts other boards there (permutation). twins may see it too, where a board
#      of rows 17 .. 31 also sits elsewhere in batch_indices' draw. The short batch reads the same rows (not tail)
# (defect, the check named for it, {n: (the checks that must fail, the checks that must pass)})
DEFECTS = [
    (leak_from_the_row_before, "neighbours", {n: ({"twins", "constant", "permutation", "neighbours"}, {"tail"}) for n in (70, 33)}),
    (lane_15_rounds_differently, "twins", {n: ({"twins", "constant", "permutation"}, {"neighbours", "tail"}) for n in (70, 33)}),
    (ragged_tail, "constant", {70: ({"twins", "constant", "permutation", "tail"}, {"neighbours"}),
                               33: ({"twins", "constant", "permutation"}, {"neighbours", "tail"})}),
    (row_0_depends_on_n, "tail", {n: ({"twins", "constant", "permutation", "tail"}, {"neighbours"}) for n in (70, 33)}),
    (second_group_reads_one_group_back, "permutation", {n: ({"permutation"}, {"constant", "neighbours", "tail"}) for n in (70, 33)}),
]


@pytest.mark.parametrize("defect,named,expected", DEFECTS, ids=[d[0].__name__ for d in DEFECTS])
def test_each_defect_fails_the_check_named_for_it(defect, named, expected):
    for n, (fail, ok) in expected.items():
        got = _failures(defect, n)
        assert named in fail and fail <= set(got) and not ok & set(got), (n, sorted(got))
        msg = got[named]
        assert msg.startswith(named + ", stand-in: row ") and "group" in msg and "lane" in msg and "pool board" in msg, msg
        assert "policy cell" in msg or "first at value" in msg, msg
    assert {d[1] for d in DEFECTS} == set(FI.CHECKS)


def test_the_message_names_rows_board_and_cell():
    msg = _failures(lane_15_rounds_differently, 70)["twins"]
    lively = FI.lively_board(B, C)
    assert msg.startswith("twins, stand-in: row 0 (group 0, lane 0) and row 15 (group 0, lane 15) hold pool board %d and differ, "
                          "first at value: " % lively), msg
    msg = _failures(ragged_tail, 70)["permutation"]
    assert "policy cell 0" in msg and "(group 4, lane 5)" in msg, msg


def test_the_gpu_test_covers_every_kernel_name():
    """(the GPU module's own count of its cases -- 105 names, a ragged case where one exists, the 14 one-product names -- and
    the conditions on its SIZE_DEPENDENT table need no GPU)"""
    import test_gpu_forward_independence as T
    T.test_the_cases_cover_every_kernel_name()
    assert set(T.SIZE_SEAM) <= set(T.SIZE_DEPENDENT) and all(len(reason) > 40 for reason in T.SIZE_DEPENDENT.values())


def gpu_batch_sizes():
    import test_gpu_forward_independence as T
    return sorted(T.batch_sizes())


def test_the_permutation_moves_nine_rows_in_ten_to_another_group_and_lane():
    sizes = set(gpu_batch_sizes()) | set(SIZES)
    assert min(sizes) == 1 and 33 in sizes and max(sizes) >= 3073
    for n in sizes:
        perm = FI.permutation(n)
        assert sorted(perm.tolist()) == list(range(n)), n
        i = np.arange(n)
        assert ((perm + i) % n == perm[0]).all() or ((perm - i) % n == perm[0]).all(), n        # a shifted reversal, or a rotation
        if not 36 <= n <= 56:
            assert ((perm + i) % n == perm[0]).all(), n
        if n >= 33:
            assert FI.coverage(perm) >= 0.9, (n, FI.coverage(perm))
    assert np.array_equal(FI.permutation(17), (np.arange(17)[::-1] + 7) % 17)
    assert FI.coverage((np.arange(70)[::-1] + 7) % 70) < 0.9          # why the shift is not 7 everywhere
