"""CPU: the replay snapshot entry points are exported and bound with the declared signatures; ReplaySnapshot.from_arrays /
to_arrays (the format's definition in numpy) round-trip bit for bit over every word count, plane count and content class;
the reference's recorded memory packs without a raw entry; the .npz file round-trips byte for byte and refuses what it must;
ao_replay_snapshot_check (no memory, no device) accepts a hand-built snapshot and refuses one mutation per rule with a message
naming the field; main.save_replay / load_replay reproduce a plain deque. tools/replay_snapshot_check_main.cpp runs the
check's cases as a stand-alone program for a host sanitizer."""
import ctypes as C
from collections import deque

import numpy as np
import pytest

from conftest import load_golden

NEW = ("ao_replay_export_size", "ao_replay_export", "ao_replay_import", "ao_replay_snapshot_check")
ARRAYS = ("kind", "z", "bits", "pi_mask", "pi_val", "raw")


def content(board, inplanes, seed=0):
    """Seven entries of every content class, as (states float32 [7, C, B, B], pi float64 [7, A], z float32 [7]) and the kinds
    they must pack to. 0: 0/1 planes, one-hot pi on the LAST cell; 1: 0/1 planes, dense pi; 2: 0/1 planes, pi holding -0.0, a
    NaN with a payload and a subnormal; 3: a plane value 0.5; 4: a plane value 2.0; 5: a plane value -0.0f on the last cell of
    the last plane; 6: all-one planes, all-zero pi. tests/test_gpu_replay_snapshot.py loads the same entries into a ring."""
    rs = np.random.RandomState(1000 * board + 10 * inplanes + seed)
    A, n = board * board, 7
    s = (rs.rand(n, inplanes, board, board) < 0.4).astype(np.float32)
    pi = rs.dirichlet(np.ones(A), n)
    pi[0] = 0.0
    pi[0, A - 1] = 1.0
    pi[2, 0] = -0.0
    pi[2, 1] = np.array([0x7ff8000000abcdef], np.uint64).view(np.float64)[0]
    pi[2, A - 1] = 5e-324
    pi[2, 3] = 0.0
    s[3, 0, 1, 1] = 0.5
    s[4, inplanes - 1, 0, 0] = 2.0
    s[5, inplanes - 1, board - 1, board - 1] = -0.0
    s[6] = 1.0
    pi[6] = 0.0
    z = np.array([1, -1, 0, 1, -1, 0, 1], np.float32)
    return s, pi, z, [0, 0, 0, 1, 1, 1, 0]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_round_trip(snap, s32, pi, z32):
    """to_arrays() against the float32 states, float64 pi and float32 z that went in: as integers, not with ==."""
    s, p, z = snap.to_arrays()
    assert s.dtype == p.dtype == z.dtype == np.float64
    assert np.array_equal(s.astype(np.float32).view(np.uint32), np.asarray(s32, np.float32).reshape(s.shape).view(np.uint32))
    assert np.array_equal(s.view(np.uint64), np.asarray(s32, np.float32).reshape(s.shape).astype(np.float64).view(np.uint64))
    assert np.array_equal(p.view(np.uint64), np.asarray(pi, np.float64).reshape(p.shape).view(np.uint64))
    assert np.array_equal(z.astype(np.float32).view(np.uint32), np.asarray(z32, np.float32).view(np.uint32))


def _snapshot():
    """3x3, two planes, four entries (the snapshot of tools/replay_snapshot_check_main.cpp). 0: one-hot pi; 1: dense pi with
    -0.0, a NaN and a subnormal; 2: kind 1, pi over three cells; 3: all-zero pi."""
    from alpha_omok_amd.replay import ReplaySnapshot
    raw = np.zeros((1, 2, 9), np.float32)
    raw[0, 0, 0], raw[0, 0, 4], raw[0, 1, 0], raw[0, 1, 8] = 0.5, 2.0, -0.0, 1.0
    val = np.array([1.0, 0.125, -0.0, np.nan, 5e-324, 0.25, 0.125, 0.125, 0.125, 0.25, 0.5, 0.25, 0.25])
    return ReplaySnapshot(3, 2, kind=np.array([0, 0, 1, 0], np.uint8), z=np.array([1, -1, 0, 1], np.float32),
                          bits=np.array([[[0x011], [0x1ff]], [[0x0a2], [0]], [[0], [0]], [[0x100], [0x0ff]]], np.uint64),
                          pi_mask=np.array([[0x010], [0x1ff], [0x007], [0]], np.uint64), pi_val=val, raw=raw)


def test_symbols_exist_with_the_declared_signatures():
    from alpha_omok_amd import _lib, build
    raw = C.CDLL(build.build())
    lib = _lib.load(build_if_missing=False)
    snap_p, i64, i64p = C.POINTER(_lib.AoReplaySnapshot), C.c_int64, C.POINTER(C.c_int64)
    want = {"ao_replay_export_size": [C.c_void_p, i64, i64, i64p, i64p],
            "ao_replay_export": [C.c_void_p, i64, i64, snap_p, i64, C.c_void_p],
            "ao_replay_import": [C.c_void_p, snap_p, i64, C.c_void_p],
            "ao_replay_snapshot_check": [snap_p]}
    for name in NEW:
        assert hasattr(raw, name), "libomok_hip.so does not export %s" % name
        res, args = _lib.SYMBOLS[name]
        fn = getattr(lib, name)
        assert res is C.c_int and fn.restype is C.c_int
        assert list(args) == want[name] and list(fn.argtypes) == want[name]
    # the struct as the header lays it out: four int32, three int64, six pointers
    f = _lib.AoReplaySnapshot
    assert [n for n, _ in f._fields_] == ["board", "inplanes", "format", "words", "entries", "pi_values", "raw_entries"] + list(ARRAYS)
    assert [getattr(f, n).offset for n, _ in f._fields_[:8]] == [0, 4, 8, 12, 16, 24, 32, 40]
    assert C.sizeof(f) == 40 + 6 * C.sizeof(C.c_void_p)
    kinds = {"kind": C.c_uint8, "z": C.c_float, "bits": C.c_uint64, "pi_mask": C.c_uint64, "pi_val": C.c_double, "raw": C.c_float}
    assert {n: t._type_ for n, t in f._fields_[7:]} == kinds
    assert lib.ao_abi_version() == 2


def test_header_declares_the_struct_in_the_bound_order():
    import os
    import re
    from conftest import REPO
    hdr = open(os.path.join(REPO, "include", "omok_hip.h")).read()
    body = re.search(r"typedef struct ao_replay_snapshot \{(.*?)\} ao_replay_snapshot;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        names += [w.strip(" *\n") for w in re.sub(r"^\s*\w+\s", "", decl.strip()).split(",") if w.strip()]
    assert names == ["board", "inplanes", "format", "words", "entries", "pi_values", "raw_entries"] + list(ARRAYS)


def test_python_layers_expose_snapshots():
    from alpha_omok_amd import main, replay
    for name in ("export_snapshot", "import_snapshot"):
        assert callable(getattr(replay.DeviceReplay, name))
    for name in ("from_arrays", "to_arrays", "save", "load", "check"):
        assert callable(getattr(replay.ReplaySnapshot, name))
    for name in ("save_replay", "load_replay"):
        assert callable(getattr(main, name))


@pytest.mark.parametrize("inplanes", [1, 5, 17])
@pytest.mark.parametrize("board,words,last", [(3, 1, 9), (9, 2, 17), (15, 4, 33)])
def test_numpy_round_trip_is_bit_for_bit(board, words, last, inplanes):
    from alpha_omok_amd.replay import ReplaySnapshot
    s, pi, z, kinds = content(board, inplanes)
    A = board * board
    snap = ReplaySnapshot.from_arrays(s, pi, z, board, inplanes).check()
    assert snap.words == words and A - 64 * (words - 1) == last and len(snap) == 7
    assert snap.kind.tolist() == kinds and 0 in kinds and 1 in kinds      # both paths are exercised
    assert snap.raw.shape == (3, inplanes, A) and same_bits(snap.raw, s[[3, 4, 5]].reshape(3, inplanes, A))
    assert not snap.bits[snap.kind == 1].any()
    # the last valid bit of the last word: the one-hot pi of entry 0 sits on cell A - 1, entry 6's planes are all ones
    assert snap.pi_mask[0].tolist() == [0] * (words - 1) + [1 << (last - 1)]
    assert (snap.bits[6, :, -1] == (1 << last) - 1).all() and (snap.bits[6, :, :-1] == 2**64 - 1).all()
    # -0.0, the NaN and the subnormal are values; +0.0 is not
    m2 = int(snap.pi_mask[2, 0])
    assert m2 & 0b1011 == 0b0011 and int(snap.pi_mask[2, -1]) >> (last - 1) == 1
    counts = [sum(bin(int(w)).count("1") for w in row) for row in snap.pi_mask]
    assert counts[0] == 1 and counts[1] == A and counts[2] == A - 1 and counts[6] == 0 and snap.pi_val.shape == (sum(counts),)
    assert snap.nbytes == 7 * (5 + 8 * words * (inplanes + 1)) + 8 * sum(counts) + 3 * 4 * inplanes * A
    assert_round_trip(snap, s, pi, z)
    # a float64 copy of the same entries (what DeviceReplay.read and a deque hold) packs to the same snapshot
    again = ReplaySnapshot.from_arrays(s.astype(np.float64), pi, z.astype(np.float64), board, inplanes)
    for name in ARRAYS:
        assert same_bits(getattr(snap, name), getattr(again, name)), name
    # ... and so does the unpacked form: the snapshot of a content is unique
    back = ReplaySnapshot.from_arrays(*snap.to_arrays(), board, inplanes)
    for name in ARRAYS:
        assert same_bits(getattr(snap, name), getattr(back, name)), name


def test_an_empty_snapshot_round_trips():
    from alpha_omok_amd.replay import ReplaySnapshot
    snap = ReplaySnapshot.from_arrays(np.zeros((0, 5, 9, 9)), np.zeros((0, 81)), np.zeros(0), 9, 5).check()
    assert len(snap) == 0 and snap.nbytes == 0
    assert [a.shape for a in snap.to_arrays()] == [(0, 5, 9, 9), (0, 81), (0,)]


def test_the_references_recorded_memory_packs_without_raw_entries():
    from alpha_omok_amd.replay import ReplaySnapshot
    g = load_golden("gv9_self_play_memory")
    for ci in range(int(g["ncases"])):
        s, pi, z = g["c%d_state" % ci], g["c%d_pi" % ci], g["c%d_z" % ci]
        snap = ReplaySnapshot.from_arrays(s, pi, z, 9, 5).check()
        assert len(snap) == s.shape[0] and snap.raw.shape[0] == 0 and not snap.kind.any()
        assert snap.nbytes == 101 * len(snap) + 8 * snap.pi_val.shape[0] < 2272 * len(snap) // 4
        assert_round_trip(snap, s, pi, z)


def test_arbitrary_float_states_come_out_kind_1():
    from alpha_omok_amd.replay import ReplaySnapshot
    g = load_golden("gv8_augment")
    for i, B in enumerate((3, 9)):
        s, pi = g["as%d" % i].astype(np.float32), g["api%d" % i]          # the memory holds planes as float32
        z = np.ones(8, np.float32)
        snap = ReplaySnapshot.from_arrays(s, pi, z, B, 5).check()
        assert snap.kind.tolist() == [1] * 8 and snap.raw.shape[0] == 8 and not snap.bits.any()
        assert_round_trip(snap, s, pi, z)


def test_save_load_round_trips_byte_for_byte(tmp_path):
    from alpha_omok_amd.replay import ReplaySnapshot
    s, pi, z, _ = content(9, 5)
    snap = ReplaySnapshot.from_arrays(s, pi, z, 9, 5)
    path = str(tmp_path / "memory.snapshot")              # exactly this path: no suffix is added
    snap.save(path)
    back = ReplaySnapshot.load(path)
    assert (back.board, back.inplanes, len(back)) == (9, 5, 7)
    for name in ARRAYS:
        assert same_bits(getattr(snap, name), getattr(back, name)), name
    with np.load(path, allow_pickle=False) as f:          # nothing in the file needs pickle
        assert set(f.files) == set(ARRAYS) | {"meta"} and int(f["meta"][0]) == 1


def _rewrite(path, out, **changes):
    with np.load(path, allow_pickle=False) as f:
        arrays = {k: f[k] for k in f.files}
    for k, v in changes.items():
        if v is None:
            del arrays[k]
        else:
            arrays[k] = v(arrays[k])
    with open(out, "wb") as fh:
        np.savez(fh, **arrays)
    return out


def test_load_refuses_other_files(tmp_path):
    from alpha_omok_amd.replay import ReplayError, ReplaySnapshot
    path = str(tmp_path / "good.npz")
    _snapshot().save(path)
    ReplaySnapshot.load(path)

    def other_format(meta):
        meta = meta.copy()
        meta[0] = 2
        return meta
    with pytest.raises(ReplayError, match="format"):
        ReplaySnapshot.load(_rewrite(path, str(tmp_path / "format.npz"), meta=other_format))
    with pytest.raises(ReplayError, match="'pi_mask'"):
        ReplaySnapshot.load(_rewrite(path, str(tmp_path / "missing.npz"), pi_mask=None))
    with pytest.raises(ReplayError, match="'z'.*float64"):
        ReplaySnapshot.load(_rewrite(path, str(tmp_path / "dtype.npz"), z=lambda a: a.astype(np.float64)))
    with pytest.raises(ReplayError, match="'bits'.*int64"):
        ReplaySnapshot.load(_rewrite(path, str(tmp_path / "dtype2.npz"), bits=lambda a: a.astype(np.int64)))
    with pytest.raises(ReplayError, match="not a replay snapshot"):
        ReplaySnapshot.load(_rewrite(path, str(tmp_path / "nometa.npz"), meta=None))
    with pytest.raises(ReplayError, match="pi_val"):      # the file's content goes through check()
        ReplaySnapshot.load(_rewrite(path, str(tmp_path / "zero.npz"), pi_val=lambda a: np.where(np.arange(a.size) == 4, 0.0, a)))


def test_check_accepts_the_hand_built_snapshot():
    snap = _snapshot().check()
    s, pi, z = snap.to_arrays()
    assert s[0, 0].ravel().tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 0] and s[2, 0].ravel().tolist() == [0.5, 0, 0, 0, 2, 0, 0, 0, 0]
    assert pi[0].tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0] and pi[2].tolist() == [0.5, 0.25, 0.25, 0, 0, 0, 0, 0, 0] and not pi[3].any()
    assert np.signbit(pi[1, 1]) and np.isnan(pi[1, 2]) and pi[1, 3] == 5e-324 and np.signbit(s[2, 1, 0, 0])


def _set(name, index, value):
    def f(s):
        getattr(s, name)[index] = value
    return f


def _attr(name, value):
    def f(s):
        setattr(s, name, value)
    return f


def _resize(name, delta):
    def f(s):
        a = getattr(s, name)
        setattr(s, name, a[:delta].copy() if delta < 0 else np.concatenate([a, np.ones((delta,) + a.shape[1:], a.dtype)]))
    return f


class _Words2:
    """A snapshot whose header says words = 2 on a 3x3 board (the class derives the field from the board)."""
    def __call__(self, s):
        struct = s._struct

        def patched():
            v = struct()
            v.words = 2
            return v
        s._struct = patched


class _Format2:
    def __call__(self, s):
        struct = s._struct

        def patched():
            v = struct()
            v.format = 2
            return v
        s._struct = patched


MUTATIONS = [
    ("board 16", _attr("board", 16), r"\bboard\b"),
    ("inplanes 33", _attr("inplanes", 33), r"\binplanes\b"),
    ("format 2", _Format2(), r"\bformat\b"),
    ("words 2 on a 3x3 board", _Words2(), r"\bwords\b"),
    ("a mask bit at cell A", _set("pi_mask", (3, 0), 1 << 9), r"\bpi_mask\b.*cell 9"),
    ("a mask bit at cell 63", _set("pi_mask", (0, 0), (1 << 63) | 0x10), r"\bpi_mask\b"),
    ("a plane bit at cell A", _set("bits", (0, 1, 0), 0x3ff), r"\bbits\b.*cell 9"),
    ("kind 2", _set("kind", 1, 2), r"\bkind\b"),
    ("bits on a kind-1 row", _set("bits", (2, 1, 0), 1), r"\bbits\b.*kind-1"),
    ("pi_values below the popcounts", _resize("pi_val", -1), r"\bpi_values\b"),
    ("pi_values above the popcounts", _resize("pi_val", 1), r"\bpi_values\b"),
    ("one corrupted mask word", _set("pi_mask", (0, 0), 0x1ff), r"\bpi_values\b"),
    ("raw_entries below the kind-1 entries", _resize("raw", -1), r"\braw_entries\b"),
    ("raw_entries above the kind-1 entries", _resize("raw", 1), r"\braw_entries\b"),
    ("a kind flipped to 0", _set("kind", 2, 0), r"\braw_entries\b"),
    ("an all-zero pattern in pi_val", _set("pi_val", 4, 0.0), r"\bpi_val\b"),
]


@pytest.mark.parametrize("what,mutate,pattern", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_check_rejects(what, mutate, pattern):
    from alpha_omok_amd.replay import ReplayError
    s = _snapshot()
    mutate(s)
    with pytest.raises(ReplayError, match=pattern):
        s.check()


def test_arrays_of_the_wrong_shape_are_refused_before_the_c_check():
    from alpha_omok_amd.replay import ReplayError, ReplaySnapshot
    s = _snapshot()
    arrays = {name: getattr(s, name) for name in ARRAYS}
    with pytest.raises(ReplayError, match="shapes"):
        ReplaySnapshot(3, 2, **dict(arrays, z=arrays["z"][:-1]))
    with pytest.raises(ReplayError, match="shapes"):
        ReplaySnapshot(9, 2, **arrays)
    with pytest.raises(ReplayError, match="shapes"):
        ReplaySnapshot(3, 2, **dict(arrays, raw=arrays["raw"].reshape(2, 9)))
    del arrays["bits"]
    with pytest.raises(ReplayError, match="'bits'"):
        ReplaySnapshot(3, 2, **arrays)


def test_main_saves_and_restores_a_plain_deque(tmp_path):
    from alpha_omok_amd import main
    from alpha_omok_amd.replay import ReplayError
    assert isinstance(main.rep_memory, deque)
    B, Cn = main.BOARD_SIZE, main.IN_PLANES
    s, pi, z, _ = content(B, Cn, seed=3)
    before = [(s[i].astype(np.float64), pi[i].copy(), float(z[i])) for i in range(7)]
    kept = list(main.rep_memory)
    path = str(tmp_path / "replay.npz")
    try:
        main.rep_memory.clear()
        main.rep_memory.extend(before)
        assert main.save_replay(path) == path
        main.rep_memory.clear()
        main.rep_memory.extend(before[:2])                # load_replay clears what is there
        main.load_replay(path)
        after = list(main.rep_memory)
        assert len(after) == 7
        for (s0, p0, z0), (s1, p1, z1) in zip(before, after):
            assert s1.dtype == np.float64 and s1.shape == (Cn, B, B) and p1.dtype == np.float64 and isinstance(z1, float)
            assert same_bits(s0, s1) and same_bits(p0, p1) and z0 == z1
        # an empty memory is a snapshot too
        main.rep_memory.clear()
        main.save_replay(path)
        main.rep_memory.extend(before)
        main.load_replay(path)
        assert len(main.rep_memory) == 0
        # a snapshot of another board is refused and the memory stays
        from alpha_omok_amd.replay import ReplaySnapshot
        o = content(B + 1, Cn)
        ReplaySnapshot.from_arrays(o[0], o[1], o[2], B + 1, Cn).save(path)
        main.rep_memory.extend(before[:3])
        with pytest.raises(ReplayError, match="board"):
            main.load_replay(path)
        assert len(main.rep_memory) == 3
    finally:
        main.rep_memory.clear()
        main.rep_memory.extend(kept)
