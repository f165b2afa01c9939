"""CPU: the tree snapshot entry points are exported and bound with the declared signatures, TreeSnapshot round-trips through
its .npz file byte for byte, and ao_tree_snapshot_check (no engine, no device) accepts a hand-built two-game snapshot and
refuses one mutation per rule with a message naming the field. tools/snapshot_check_main.cpp runs the same mutations as a
stand-alone program for a host sanitizer."""
import ctypes as C

import numpy as np
import pytest

NEW = ("ao_tree_export", "ao_tree_import", "ao_tree_snapshot_check")
FRESH, UNEXPANDED, EXPANDED = 0, 1, 2


def _snapshot():
    """3x3. Game 0: one move played (cell 4), an expanded root with two expanded children and one terminal edge: 3 nodes, 22
    edges. Game 1: fresh, with a cached gaussian."""
    from alpha_omok_amd.snapshot import TreeSnapshot
    hdr = np.array([[3, 22, 1, EXPANDED, 0, 17, 0, 0], [0, 0, 0, FRESH, 0, 624, 1, 0]], np.int32)
    moves = np.zeros((2, 9), np.int32)
    moves[0, 0] = 4
    act = np.array([0, 1, 2, 3, 5, 6, 7, 8] + [1, 2, 3, 5, 6, 7, 8] + [0, 2, 3, 5, 6, 7, 8], np.uint8)
    n, child = np.zeros(22, np.int32), np.full(22, -1, np.int32)
    w, q = np.zeros(22, np.float32), np.zeros(22, np.float32)
    n[[0, 1, 2, 8]] = [3, 2, 1, 1]
    child[[0, 1, 2]] = [1, 2, -2]
    w[[0, 1, 2, 8]] = [1.5, -1.0, 1.0, 0.25]
    q[[0, 1, 2, 8]] = [0.5, -0.5, 1.0, 0.25]
    mt = (np.arange(2 * 624, dtype=np.uint64) * 2654435761 % 2**32).astype(np.uint32).reshape(2, 624)
    return TreeSnapshot(3, 5, 3, sims=10, noise=1, c_puct=5.0, hdr=hdr, gauss=np.array([0.0, -0.25]), mt=mt, moves=moves,
                        nchild=np.array([8, 7, 7], np.int32), parent=np.array([-1, 0, 0], np.int32),
                        parent_edge=np.array([-1, 0, 1], np.int32), act=act, n=n, w=w, q=q, p=np.full(22, 0.125), child=child)


ARRAYS = ("hdr", "gauss", "mt", "moves", "nchild", "parent", "parent_edge", "act", "n", "w", "q", "p", "child")


def test_symbols_exist_with_the_declared_signatures():
    from alpha_omok_amd import _lib, build
    raw = C.CDLL(build.build())
    lib = _lib.load(build_if_missing=False)
    snap_p = C.POINTER(_lib.AoTreeSnapshot)
    want = {"ao_tree_export": [C.c_void_p, C.POINTER(C.c_uint8), snap_p],
            "ao_tree_import": [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, snap_p],
            "ao_tree_snapshot_check": [snap_p]}
    for name in NEW:
        assert hasattr(raw, name), "libomok_hip.so does not export %s" % name
        res, args = _lib.SYMBOLS[name]
        fn = getattr(lib, name)
        assert res is C.c_int and fn.restype is C.c_int
        assert list(args) == want[name] and list(fn.argtypes) == want[name]
    # the struct as the header lays it out: six int32, a double, two int64, thirteen pointers
    f = _lib.AoTreeSnapshot
    assert [n for n, _ in f._fields_] == ["board", "inplanes", "win_mark", "sims", "noise", "games", "c_puct", "nodes", "edges"] + list(ARRAYS)
    assert (f.c_puct.offset, f.nodes.offset, f.edges.offset, f.hdr.offset) == (24, 32, 40, 48)
    assert C.sizeof(f) == 48 + 13 * C.sizeof(C.c_void_p)
    assert lib.ao_abi_version() == 2 and _lib.AO_SNAP_HDR == 8


def test_python_layers_expose_snapshots():
    from alpha_omok_amd import agents, engine, snapshot
    for name in ("export_trees", "import_trees"):
        assert callable(getattr(engine.Engine, name))
    for name in ("save_tree", "load_tree"):
        assert callable(getattr(agents.ZeroAgent, name))
    for name in ("save", "load", "check", "select"):
        assert callable(getattr(snapshot.TreeSnapshot, name))


def test_save_load_round_trips_byte_for_byte(tmp_path):
    from alpha_omok_amd.snapshot import TreeSnapshot
    s = _snapshot()
    path = str(tmp_path / "two_games.npz")
    s.save(path)
    t = TreeSnapshot.load(path)
    assert (t.board, t.inplanes, t.win_mark, t.sims, t.noise, t.c_puct) == (3, 5, 3, 10, 1, 5.0)
    for name in ARRAYS:
        a, b = getattr(s, name), getattr(t, name)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name
    assert (t.games, t.nodes, t.edges) == (2, 3, 22)
    # 25 bytes per edge, 12 per node, a fixed header per game
    assert s.nbytes == 25 * 22 + 12 * 3 + 2 * TreeSnapshot.header_nbytes(3)
    assert s.game_nbytes(0) + s.game_nbytes(1) == s.nbytes
    with np.load(path, allow_pickle=False) as z:          # nothing in the file needs pickle
        assert set(z.files) == set(ARRAYS) | {"meta", "c_puct"}
    # subsets: order and repetition-free selection
    u = s.select([1, 0])
    u.check()
    assert u.hdr[:, 0].tolist() == [0, 3] and u.nodes == 3 and u.edges == 22 and u.gauss.tolist() == [-0.25, 0.0]
    one = s.select([1])
    one.check()
    assert (one.games, one.nodes, one.edges) == (1, 0, 0)
    assert s.select([0]).act.tobytes() == s.act.tobytes()
    with pytest.raises(IndexError):
        s.select([2])


def test_check_accepts_the_hand_built_snapshot():
    assert _snapshot().check() is not None


def _truncate_edges(s):
    for name in ("act", "n", "w", "q", "p", "child"):
        setattr(s, name, getattr(s, name)[:-1].copy())


def _set(name, index, value):
    def f(s):
        getattr(s, name)[index] = value
    return f


def _many(*fs):
    def f(s):
        for g in fs:
            g(s)
    return f


MUTATIONS = [
    ("a child index pointing backwards", _set("child", 8, 0), r"\bchild\b.*backwards"),
    ("a node named by two edges", _many(_set("child", 3, 2), _set("n", 3, 1)), r"\bchild\b.*two edges"),
    ("a wrong parent_edge", _set("parent_edge", 2, 0), r"\bparent_edge\b"),
    ("nchild = 0", _set("nchild", 1, 0), r"\bnchild\b"),
    ("nchild beyond A - ply", _many(_set("nchild", 1, 8), _set("nchild", 2, 6)), r"\bnchild\b.*A - ply"),
    ("a duplicate action", _set("act", 9, 1), r"\bact\b.*repeats"),
    ("a NaN p", _set("p", 5, np.nan), r"\bp: .*not finite"),
    ("a truncated edge array", _truncate_edges, r"\bedges\b"),
    ("pos = 625", _set("hdr", (1, 5), 625), r"\bpos\b"),
    ("a repeated root move", _many(_set("hdr", (1, 2), 2), _set("moves", (1, 0), 3), _set("moves", (1, 1), 3)), r"\bmoves\b.*twice"),
    # beyond the list: what the device code relies on
    ("an action off the board", _set("act", 21, 9), r"\bact\b"),
    ("a child beyond the game", _many(_set("child", 3, 3), _set("n", 3, 1)), r"\bchild\b"),
    ("children out of scan order", _many(_set("child", 0, 2), _set("child", 1, 1)), r"\bchild\b.*scan order"),
    ("an expanded child without a visit", _set("n", 1, 0), r"\bn: "),
    ("a negative n", _set("n", 4, -1), r"\bn: "),
    ("an infinite w", _set("w", 0, np.inf), r"\bw: "),
    ("a NaN q", _set("q", 0, np.nan), r"\bq: "),
    ("a wrong parent", _set("parent", 2, 1), r"\bparent: "),
    ("a huge nchild", _set("nchild", 0, 2**31 - 1), r"\bnchild\b"),
    ("a huge node count", _set("hdr", (0, 0), 2**31 - 1), r"\bnodes\b"),
    ("a root move off the board", _set("moves", (0, 0), 9), r"\bmoves\b"),
    ("a tree below a fresh root", _set("hdr", (0, 3), FRESH), r"\bstatus\b"),
    ("a finished game with a tree", _set("hdr", (0, 4), 1), r"\bover\b"),
]


@pytest.mark.parametrize("what,mutate,pattern", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_check_rejects(what, mutate, pattern):
    from alpha_omok_amd.snapshot import SnapshotError
    s = _snapshot()
    mutate(s)
    with pytest.raises(SnapshotError, match=pattern):
        s.check()


def test_arrays_of_unequal_length_are_refused_before_the_c_check():
    from alpha_omok_amd.snapshot import SnapshotError, TreeSnapshot
    s = _snapshot()
    arrays = {name: getattr(s, name) for name in ARRAYS}
    arrays["q"] = arrays["q"][:-1]
    with pytest.raises(SnapshotError, match="edge arrays"):
        TreeSnapshot(3, 5, 3, **arrays)
    del arrays["q"]
    with pytest.raises(SnapshotError, match="'q'"):
        TreeSnapshot(3, 5, 3, **arrays)
