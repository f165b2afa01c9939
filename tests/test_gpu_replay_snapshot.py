"""-m gpu: replay snapshots packed and unpacked on the device (csrc/replay_snapshot.hip) against the numpy packer
(ReplaySnapshot.from_arrays, the format's definition) and against deque(maxlen).extend, byte for byte. Every case holds at most
a few hundred entries; chunk_bytes=4096 makes an export or import cross chunk boundaries (a 9x9, 5-plane entry packs to 101 -
2500 bytes)."""
from collections import deque

import numpy as np
import pytest

from test_replay_snapshot_host import ARRAYS, content, same_bits

pytestmark = pytest.mark.gpu


def _tuples(s, pi, z):
    return [(s[i].astype(np.float64), pi[i].copy(), float(z[i])) for i in range(s.shape[0])]


def _content(board, inplanes, seed=0):
    s, pi, z, _ = content(board, inplanes, seed)
    return _tuples(s, pi, z)


def _host_snapshot(mem, first, n):
    from alpha_omok_amd.replay import ReplaySnapshot
    return ReplaySnapshot.from_arrays(*mem.read(first, n), mem.B, mem.C)


def _assert_same_snapshot(got, want, what):
    assert (got.board, got.inplanes, len(got)) == (want.board, want.inplanes, len(want)), what
    for name in ARRAYS:
        assert same_bits(getattr(got, name), getattr(want, name)), "%s: array %r differs" % (what, name)


def _assert_same_memory(mem, ref, what):
    """The ring against a deque of (state, pi, z) tuples: entry for entry, as integers."""
    assert len(mem) == len(ref), what
    if not len(ref):
        return
    s, pi, z = mem.read(0, len(mem))
    rs = np.stack([e[0] for e in ref]).astype(np.float32)
    rp = np.stack([e[1] for e in ref])
    rz = np.array([e[2] for e in ref], np.float32)
    assert np.array_equal(s.astype(np.float32).view(np.uint32), rs.view(np.uint32)), what + ": states"
    assert np.array_equal(pi.view(np.uint64), rp.view(np.uint64)), what + ": pi"
    assert np.array_equal(z.astype(np.float32).view(np.uint32), rz.view(np.uint32)), what + ": z"


def _junk(board, inplanes, n):
    """Dense junk: all planes 1.0, every pi cell non-zero -- a slot byte an import failed to write then shows."""
    A = board * board
    return [(np.ones((inplanes, board, board)), np.full(A, 0.75) + k, -0.5) for k in range(n)]


@pytest.mark.parametrize("inplanes", [1, 5, 17])
@pytest.mark.parametrize("board", [3, 9, 15])
def test_export_equals_the_host_packer(board, inplanes):
    from alpha_omok_amd.replay import DeviceReplay, ReplayError
    cap = 37
    mem = DeviceReplay(board, inplanes, cap)
    try:
        # a range of zero entries of an empty memory
        empty = mem.export_snapshot()
        assert len(empty) == 0 and empty.nbytes == 0
        # not yet full: every content class through extend, three of them through extend_augmented
        ents = _content(board, inplanes)
        mem.extend(ents)
        mem.extend_augmented(ents[:3])
        assert len(mem) == 31
        whole = _host_snapshot(mem, 0, 31)
        assert whole.kind.tolist() == [0, 0, 0, 1, 1, 1, 0] + [0] * 24
        for chunk in (0, 4096, 1):
            _assert_same_snapshot(mem.export_snapshot(chunk_bytes=chunk), whole, "not full, chunk_bytes %d" % chunk)
        _assert_same_snapshot(mem.export_snapshot(5, 0), _host_snapshot(mem, 5, 0), "zero entries")
        _assert_same_snapshot(mem.export_snapshot(4, 9, chunk_bytes=4096), _host_snapshot(mem, 4, 9), "sub-range")
        # wrapped: the kind-1 entries through extend_augmented; 55 entries went in, so the head is slot 18 and the window
        # starts with the last five entries of an orbit of eight
        mem.extend_augmented(ents[3:6])
        assert len(mem) == cap
        before = mem.read(0, cap)
        whole = _host_snapshot(mem, 0, cap)
        assert whole.kind.tolist() == [0] * 13 + [1] * 24 and whole.raw.shape[0] == 24
        for chunk in (0, 4096, 1):
            _assert_same_snapshot(mem.export_snapshot(chunk_bytes=chunk), whole, "wrapped, chunk_bytes %d" % chunk)
        # deque index 19 is slot 0: a sub-range across the wrap, and one that ends on the last slot
        for first, n in ((10, 20), (0, 19), (19, 18), (36, 1)):
            for chunk in (0, 4096):
                _assert_same_snapshot(mem.export_snapshot(first, n, chunk_bytes=chunk), _host_snapshot(mem, first, n),
                                      "range %d+%d, chunk_bytes %d" % (first, n, chunk))
        # read-only on the ring
        after = mem.read(0, cap)
        for a, b in zip(before, after):
            assert same_bits(a, b)
        assert len(mem) == cap
        # a range outside the memory
        for first, n in ((0, cap + 1), (-1, 2), (cap, 1)):
            with pytest.raises(ReplayError, match="range outside"):
                mem.export_snapshot(first, n)
    finally:
        mem.close()


def test_export_fails_with_nothing_written_when_a_capacity_is_too_small():
    import ctypes as C
    from alpha_omok_amd.replay import DeviceReplay, ReplaySnapshot
    mem = DeviceReplay(9, 5, 64)
    try:
        mem.extend(_content(9, 5))
        good = mem.export_snapshot()
        for short in ("pi_val", "raw", "kind"):
            arrays = {name: np.full_like(getattr(good, name), 0x55 if name != "pi_val" else 7.0) for name in ARRAYS}
            arrays[short] = arrays[short][:-1].copy()
            if short == "kind":
                arrays.update(z=arrays["z"][:-1].copy(), bits=arrays["bits"][:-1].copy(), pi_mask=arrays["pi_mask"][:-1].copy())
            snap = ReplaySnapshot(9, 5, **arrays)
            keep = {name: getattr(snap, name).copy() for name in ARRAYS}
            s = snap._struct()
            assert mem._L.ao_replay_export(mem._h, 0, 7, C.byref(s), 0, None) != 0
            msg = mem._L.ao_replay_last_error(mem._h).decode()
            assert {"pi_val": "pi_values", "raw": "raw_entries", "kind": "entries"}[short] in msg
            for name in ARRAYS:
                assert same_bits(getattr(snap, name), keep[name]), name
    finally:
        mem.close()


def _source(board=9, inplanes=5):
    """A wrapped memory of capacity 61 with every content class in it, through extend and extend_augmented."""
    from alpha_omok_amd.replay import DeviceReplay
    src = DeviceReplay(board, inplanes, 61)
    ents = _content(board, inplanes)
    src.extend(ents)
    src.extend_augmented(ents[:2] + ents[3:5])
    src.extend(_content(board, inplanes, seed=1))
    src.extend_augmented(ents[5:])
    assert len(src) == 61
    return src


IMPORTS = [
    ("a fresh ring of the same capacity", 61, 0),
    ("a smaller ring: only the newest survive", 20, 0),
    ("a capacity below 8", 5, 0),
    ("a ring that holds entries and wraps during the import", 80, 30),   # 19 of the 30 survive
]


@pytest.mark.parametrize("board,inplanes", [(9, 5), (3, 1), (15, 17)])
@pytest.mark.parametrize("what,cap,held", IMPORTS, ids=[i[0] for i in IMPORTS])
def test_import_equals_deque_extend(what, cap, held, board, inplanes):
    from alpha_omok_amd.replay import DeviceReplay
    src = _source(board, inplanes)
    dsts = []
    try:
        snap = src.export_snapshot()
        s, pi, z = src.read(0, len(src))
        entries = _tuples(s, pi, z)
        assert snap.kind.any() and not snap.kind.all()
        older = _content(board, inplanes, seed=2) * 5
        results = []
        for chunk in (0, 4096):
            dst = DeviceReplay(board, inplanes, cap)
            dsts.append(dst)
            dst.extend(_junk(board, inplanes, cap))        # every slot holds dense junk
            dst.clear()
            ref = deque(maxlen=cap)
            if held:
                dst.extend(older[:held])
                ref.extend(older[:held])
            dst.import_snapshot(snap, chunk_bytes=chunk)
            ref.extend(entries)
            _assert_same_memory(dst, list(ref), "%s, chunk_bytes %d" % (what, chunk))
            results.append(dst.read(0, len(dst)))
            # the ring goes on behaving like the deque
            more = _content(board, inplanes, seed=4)[:3]
            dst.extend(more)
            ref.extend(more)
            _assert_same_memory(dst, list(ref), "%s, chunk_bytes %d, after a further extend" % (what, chunk))
        for a, b in zip(*results):
            assert same_bits(a, b)
    finally:
        src.close()
        for d in dsts:
            d.close()


def test_import_twice_and_an_empty_snapshot():
    from alpha_omok_amd.replay import DeviceReplay
    src = _source()
    dst = DeviceReplay(9, 5, 100)
    try:
        snap = src.export_snapshot(40, 21)
        entries = _tuples(*src.read(40, 21))
        dst.extend(_junk(9, 5, 100))
        dst.clear()
        ref = deque(maxlen=100)
        for _ in range(6):                                # 126 entries: the ring wraps between two imports
            dst.import_snapshot(snap, chunk_bytes=4096)
            ref.extend(entries)
        _assert_same_memory(dst, list(ref), "six imports")
        dst.import_snapshot(src.export_snapshot(3, 0))
        _assert_same_memory(dst, list(ref), "an empty snapshot")
    finally:
        src.close()
        dst.close()


def test_mini_batches_of_the_restored_ring():
    import torch
    from alpha_omok_amd.replay import DeviceReplay
    src = _source()
    dst = DeviceReplay(9, 5, 61)
    try:
        dst.extend(_junk(9, 5, 40))                       # the restored ring's head is slot 40: another wrap than the source's
        dst.import_snapshot(src.export_snapshot(), chunk_bytes=4096)
        assert len(dst) == 61
        idx = [0, 60, 20, 21, 22, 7, 59, 1, 30, 45, 20]   # across both rings' wraps, one index twice
        for a, b in zip(src.batch(idx), dst.batch(idx)):
            assert a.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))
    finally:
        src.close()
        dst.close()


def test_refusals_leave_the_ring_untouched():
    from alpha_omok_amd.replay import DeviceReplay, ReplayError, ReplaySnapshot
    src = _source()
    dst = DeviceReplay(9, 5, 30)
    try:
        held = _content(9, 5, seed=2) * 3
        dst.extend(held)                                  # 21 of 30: an import of 61 would overwrite all of it
        good = src.export_snapshot()
        b10 = content(10, 5)
        c3 = content(9, 3)
        bad_mask = ReplaySnapshot(9, 5, **{name: getattr(good, name).copy() for name in ARRAYS})
        bad_mask.pi_mask[17, 1] ^= 1 << 5
        cases = [("another board", ReplaySnapshot.from_arrays(b10[0], b10[1], b10[2], 10, 5), "board"),
                 ("other inplanes", ReplaySnapshot.from_arrays(c3[0], c3[1], c3[2], 9, 3), "inplanes"),
                 ("one corrupted mask word", bad_mask, "pi_values")]
        for what, snap, field in cases:
            with pytest.raises(ReplayError, match=field):
                dst.import_snapshot(snap)
            assert len(dst) == 21, what
            _assert_same_memory(dst, held, what)
        dst.import_snapshot(good)                         # and the good one still goes in
        assert len(dst) == 30
    finally:
        src.close()
        dst.close()


def test_main_saves_and_restores_the_device_memory(tmp_path):
    import alpha_omok_amd.main as main
    from alpha_omok_amd.replay import DeviceReplay
    main.PRINT_SELFPLAY = False
    try:
        main.configure(board_size=9, n_mcts=8, n_blocks=1, out_planes=32, seed=0, device_replay=True)
        assert isinstance(main.rep_memory, DeviceReplay)
        main.cur_memory.clear()
        main.rep_memory.clear()
        main.reset_iter(main.result, main.cur_memory)
        main.self_play(2, seeds=[5, 6])
        n = len(main.rep_memory)
        assert n == 8 * len(main.cur_memory) > 0
        before = main.rep_memory.read(0, n)
        path = str(tmp_path / "replay.npz")
        assert main.save_replay(path) == path
        main.rep_memory.clear()
        assert len(main.rep_memory) == 0
        main.load_replay(path)
        assert len(main.rep_memory) == n
        for a, b in zip(before, main.rep_memory.read(0, n)):
            assert same_bits(a, b)
        # the same file restores a host deque
        main.configure(board_size=9, n_mcts=8, n_blocks=1, out_planes=32, seed=0)
        assert isinstance(main.rep_memory, deque)
        main.load_replay(path)
        assert len(main.rep_memory) == n
        for k in (0, n // 2, n - 1):
            s, pi, z = main.rep_memory[k]
            assert same_bits(s, before[0][k]) and same_bits(pi, before[1][k]) and z == before[2][k]
    finally:
        main.cur_memory.clear()
        main.configure(board_size=9, n_mcts=24, n_blocks=1, out_planes=32, seed=0)
        main.rep_memory.clear()
        main.reset_iter(main.result, main.cur_memory)
        main.release_engine()
