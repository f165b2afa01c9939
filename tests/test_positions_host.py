"""CPU: the position-batch layer (alpha_omok_amd.positions, csrc/positions.hip) as far as it goes without a device: the C
ABI is declared and exported, and every mistake of shape or type is refused on the host before anything reaches a GPU."""
import os
import re

import numpy as np
import pytest

from conftest import REPO

NEW_SYMBOLS = ("ao_positions", "ao_positions_create", "ao_positions_destroy", "ao_positions_last_error",
               "ao_positions_check_win", "ao_positions_from_moves", "ao_positions_evaluate")


def test_header_declares_and_library_exports_the_position_entry_points():
    from alpha_omok_amd import _lib, build
    hdr = open(os.path.join(REPO, "include", "omok_hip.h")).read()
    assert re.search(r"typedef\s+struct\s+ao_positions\s+ao_positions\s*;", hdr)
    declared = set(re.findall(r"\b(ao_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS[1:]:
        assert name in declared, "omok_hip.h does not declare %s" % name
        assert name in _lib.SYMBOLS, "_lib.SYMBOLS lacks %s" % name
    assert "positions.hip" in build.SOURCES
    build.build()
    lib = _lib.load(build_if_missing=False)
    for name in NEW_SYMBOLS[1:]:
        assert hasattr(lib, name), "libomok_hip.so does not export %s" % name
    assert lib.ao_abi_version() == 2          # additive change


def test_package_exports_the_new_names():
    import alpha_omok_amd
    from alpha_omok_amd import positions
    assert alpha_omok_amd.PositionBatch is positions.PositionBatch
    assert alpha_omok_amd.positions is positions
    from alpha_omok_amd.agents import ZeroAgent
    assert callable(ZeroAgent.get_pv_batch)


@pytest.mark.parametrize("kw", [dict(board_size=4, win_mark=5), dict(board_size=9, win_mark=6), dict(board_size=9, win_mark=2),
                                dict(board_size=2), dict(board_size=16), dict(board_size=9, inplanes=0),
                                dict(board_size=9, inplanes=10), dict(board_size=9, capacity=0), dict(board_size=9.0)])
def test_constructor_refuses_bad_configurations_before_any_device_call(kw, monkeypatch):
    from alpha_omok_amd import _lib, positions

    def no_device(*a, **k):
        raise AssertionError("the library was asked for before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_device)
    with pytest.raises(ValueError):
        positions.PositionBatch(**kw)


def test_win_mark_default_follows_zero_agent():
    from alpha_omok_amd import positions
    assert positions.default_win_mark(3) == 3
    assert [positions.default_win_mark(b) for b in (4, 5, 9, 15)] == [5, 5, 5, 5]
    with pytest.raises(ValueError):          # ... which a 4x4 board cannot hold: say so instead of answering 0 forever
        positions.check_config(4, 5, positions.default_win_mark(4), 16)


def test_pack_boards_validation():
    from alpha_omok_amd.positions import pack_boards
    ok = pack_boards(np.zeros((2, 9, 9)), 9)
    assert ok.dtype == np.int8 and ok.shape == (2, 9, 9) and ok.flags["C_CONTIGUOUS"]
    one = pack_boards(np.eye(3), 3)                      # a single board is a batch of one
    assert one.shape == (1, 3, 3) and one[0, 1, 1] == 1
    flt = pack_boards(np.array([[[1.0, -1.0, 0.0]] * 3]), 3)
    assert flt.tolist() == [[[1, -1, 0]] * 3]
    for bad in (np.zeros((2, 9, 8)), np.zeros((2, 8, 8)), np.zeros((9,)), np.zeros((1, 2, 9, 9)), np.zeros((0,))):
        with pytest.raises(ValueError):
            pack_boards(bad, 9)
    for v in (2, -2, 0.5, np.nan):
        b = np.zeros((1, 9, 9))
        b[0, 4, 4] = v
        with pytest.raises(ValueError):
            pack_boards(b, 9)
    with pytest.raises(ValueError):
        pack_boards([[[0, 1, 0], [0, 0], [1, 1, 1]]], 3)  # ragged
    with pytest.raises(ValueError):
        pack_boards(np.array([["x"] * 3] * 3), 3)


def test_pack_ids_says_what_a_list_is_taken_for():
    from alpha_omok_amd.positions import pack_ids
    mv, n = pack_ids([(0,), (0, 4, 0, 7), (0, 5)])
    assert mv.dtype == np.int32 and n.dtype == np.int32
    assert n.tolist() == [0, 3, 1] and mv.shape == (3, 3)
    assert mv[1].tolist() == [4, 0, 7] and mv[2].tolist() == [5, 0, 0]
    # the same moves as bare lists: nothing is guessed from a leading 0
    mv2, n2 = pack_ids([(), (4, 0, 7), (5,)], leading_zero=False)
    assert np.array_equal(mv, mv2) and np.array_equal(n, n2)
    mv3, n3 = pack_ids([(0, 4)], leading_zero=False)
    assert n3.tolist() == [2] and mv3[0].tolist() == [0, 4]
    # numpy rows and integer-valued floats are fine; bad MOVES are not judged here (they are the position's err)
    mv4, n4 = pack_ids(np.array([[0, 1, 2], [0, 3, 4]]))
    assert n4.tolist() == [2, 2] and mv4.tolist() == [[1, 2], [3, 4]]
    mv5, n5 = pack_ids([(0.0, 3.0), (0, -1, 500, 3, 3)])
    assert n5.tolist() == [1, 4] and mv5[1].tolist() == [-1, 500, 3, 3]
    e, ne = pack_ids([])
    assert ne.shape == (0,) and e.shape[0] == 0


@pytest.mark.parametrize("bad", [
    [(0, 1), (0, (2, 3))],            # ragged: an id with a nested entry
    [(0, 1), [[0, 2], [0, 3]]],       # an id that is itself a list of ids
    [(0, 1), 5],                      # not a sequence
    [(0, 1), "012"],
    [(0, 1.5)],                       # not an integer
    [(0, 1), (3, 4)],                 # lacks the leading 0
    [(0, 1), ()],                     # a reference-style id is never empty
    [(0, 2 ** 31)],                   # does not fit the ABI's int32
    np.zeros((2, 2, 2), np.int64),
    7,
])
def test_pack_ids_refuses_malformed_ids(bad):
    from alpha_omok_amd.positions import pack_ids
    with pytest.raises(ValueError):
        pack_ids(bad)


def test_methods_validate_before_touching_the_device():
    """check_win / describe / planes / evaluate of an instance whose handle must not be used: the ValueError comes first."""
    from alpha_omok_amd.positions import PositionBatch

    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError("device call %s before validation" % name)

    pb = PositionBatch.__new__(PositionBatch)
    pb._h, pb._L, pb._evaluator = None, NoDevice(), None
    pb.board_size, pb.inplanes, pb.win_mark, pb.capacity, pb.device, pb.A = 9, 5, 5, 16, 0, 81
    with pytest.raises(ValueError):
        pb.check_win(np.zeros((1, 9, 8)))
    with pytest.raises(ValueError):
        pb.check_win(np.full((1, 9, 9), 2))
    with pytest.raises(ValueError):
        pb.describe([(0, 1), (0, (2, 3))])
    with pytest.raises(ValueError):
        pb.planes([(1, 2)])
    with pytest.raises(ValueError):
        pb.evaluate(object(), [(0, 1), (2,)])


def test_construction_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from alpha_omok_amd.engine import EngineError
    from alpha_omok_amd.positions import PositionBatch
    with pytest.raises(EngineError, match="ao_positions_create"):
        PositionBatch(9)
