"""-m gpu: "any output may be null" of the id-batch entry points that PositionBatch always calls with every output
(ao_positions_win_cells, _audit, _forced_wins, _forced_defences of include/omok_hip.h), through the C ABI itself.

One workspace: a 5x5 board with win_mark 4 and capacity 2; three ids, so a call spans two chunks and the second one is
partial -- a position that holds a win, an open position of four moves, and an id with a stone on an occupied cell. Each
entry point is called with every output, with each output alone and with none (which must return 0 too); an output asked
for alone must equal the same array of the full call, exactly. Arrays go in filled with 0x55: an output that is not
written would show."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BOARD, MARK, CAP, DEPTH, NODES = 5, 4, 2, 2, 64
A = BOARD * BOARD
IDS = ((0, 5, 1, 6, 2, 7, 3),   # black completes 0..3 with its fourth stone
       (0, 5, 1, 6),            # open
       (0, 5, 0))               # the third move lands on the first
LINE = 2 * DEPTH - 1
I32, U8, I16 = (C.c_int32, np.int32), (C.c_uint8, np.uint8), (C.c_int16, np.int16)
# entry point -> (arguments between n and the outputs, the outputs in ABI order as (name, elements per position, type))
CALLS = {
    "ao_positions_win_cells": ((), (("mine", A, U8), ("theirs", A, U8), ("status", 1, I32), ("turn", 1, I32), ("err", 1, I32))),
    "ao_positions_audit": ((), (("flags", A, U8), ("counts", 8, I32), ("err", 1, I32))),
    "ao_positions_forced_wins": ((DEPTH, NODES), (("result", 1, I32), ("depth", 1, I32), ("move", 1, I32), ("moves", A, U8),
                                                   ("line", LINE, I16), ("line_len", 1, I32), ("nodes", 1, I32),
                                                   ("status", 1, I32), ("turn", 1, I32), ("err", 1, I32))),
    "ao_positions_forced_defences": ((DEPTH, NODES), (("threat", 1, I32), ("threat_depth", 1, I32), ("threat_moves", A, U8),
                                                       ("reply", A, U8), ("depth", A, U8), ("counts", 4, I32), ("nodes", 1, I32),
                                                       ("status", 1, I32), ("turn", 1, I32), ("err", 1, I32))),
}


@pytest.fixture(scope="module")
def workspace():
    from alpha_omok_amd import _lib
    L = _lib.load()
    h = C.c_void_p()
    assert L.ao_positions_create(BOARD, 5, MARK, CAP, 0, C.byref(h)) == 0, L.ao_positions_last_error(None).decode()
    yield L, h
    L.ao_positions_destroy(h)


def _call(L, h, name, wanted):
    """the entry point with the outputs named in `wanted`, NULL for the rest -> dict of the arrays it was given"""
    extra, outs = CALLS[name]
    stride = max(len(i) for i in IDS)
    moves = np.zeros((len(IDS), stride), np.int32)
    for k, i in enumerate(IDS):
        moves[k, :len(i)] = i
    n = np.array([len(i) for i in IDS], np.int32)
    got, ptrs = {}, []
    for key, per, (ct, dt) in outs:
        if key in wanted:
            got[key] = np.full((len(IDS), per), 0x55, dt)
            ptrs.append(got[key].ctypes.data_as(C.POINTER(ct)))
        else:
            ptrs.append(None)
    i32p = C.POINTER(C.c_int32)
    rc = getattr(L, name)(h, moves.ctypes.data_as(i32p), stride, n.ctypes.data_as(i32p), len(IDS), *extra, *ptrs)
    assert rc == 0, "%s with %s: %s" % (name, sorted(wanted), L.ao_positions_last_error(h).decode())
    return got


@pytest.mark.parametrize("name", sorted(CALLS))
def test_each_output_alone_equals_the_full_call(workspace, name):
    L, h = workspace
    keys = [key for key, _, _ in CALLS[name][1]]
    full = _call(L, h, name, keys)
    # (the ids are what the docstring says they are, and every output was written in both chunks)
    np.testing.assert_array_equal(full["err"][:, 0], [0, 0, 2])
    if "status" in full:
        np.testing.assert_array_equal(full["status"][:, 0], [1, 0, 0])
    else:
        np.testing.assert_array_equal(full["counts"][:, 7], [1, 0, 0])
    for key in keys:
        assert not (full[key] == np.asarray(0x55, full[key].dtype)).all(axis=1).any(), key
    for key in keys:
        alone = _call(L, h, name, [key])
        assert list(alone) == [key]
        np.testing.assert_array_equal(alone[key], full[key], err_msg="%s: %s asked for alone" % (name, key))
    assert _call(L, h, name, []) == {}
