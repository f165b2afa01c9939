"""`TreeSnapshot`: search trees and MT19937 streams of some games as host data (ao_tree_snapshot, include/omok_hip.h).

What `Engine.export_trees` returns and `Engine.import_trees` takes; `.save` / `.load` keep it in an `.npz` file. Per game: the
root id's moves, the root status, the stream, and what the root reaches, breadth first with the root as node 0 -- per node
`nchild`, `parent`, `parent_edge`, per edge `act`, `n`, `w`, `q`, `p`, `child`. Positions are not stored: the import rebuilds
them from the moves. A snapshot captures trees and streams, not a move in progress.
"""
import ctypes as C

import numpy as np

from . import _lib

_GAME = (("hdr", np.int32), ("gauss", np.float64), ("mt", np.uint32), ("moves", np.int32))
_NODE = (("nchild", np.int32), ("parent", np.int32), ("parent_edge", np.int32))
_EDGE = (("act", np.uint8), ("n", np.int32), ("w", np.float32), ("q", np.float32), ("p", np.float64), ("child", np.int32))
_FORMAT = 1


class SnapshotError(ValueError):
    pass


class TreeSnapshot:
    """Arrays (numpy, C-contiguous): hdr int32 [games, 8] = nodes, edges, number of moves, AO_ROOT_* status, over, stream pos,
    has_gauss, 0; gauss float64 [games]; mt uint32 [games, 624]; moves int32 [games, A]; nchild / parent / parent_edge int32
    [nodes]; act uint8, n int32, w / q float32, p float64, child int32 [edges]. Header fields: board, inplanes, win_mark (the
    importing engine must match), sims, noise, c_puct (information only)."""

    def __init__(self, board, inplanes, win_mark, sims=0, noise=0, c_puct=0.0, **arrays):
        self.board, self.inplanes, self.win_mark = int(board), int(inplanes), int(win_mark)
        self.sims, self.noise, self.c_puct = int(sims), int(noise), float(c_puct)
        A = self.board * self.board
        for name, dt in _GAME + _NODE + _EDGE:
            if name not in arrays:
                raise SnapshotError("snapshot lacks the array %r" % name)
            setattr(self, name, np.ascontiguousarray(arrays[name], dt))
        g = self.hdr.shape[0] if self.hdr.ndim == 2 else -1
        if self.hdr.shape != (g, _lib.AO_SNAP_HDR) or self.gauss.shape != (g,) or self.mt.shape != (g, 624) or self.moves.shape != (g, A):
            raise SnapshotError("hdr / gauss / mt / moves: shapes must be [games, 8], [games], [games, 624], [games, A]")
        for group, what in ((_NODE, "node"), (_EDGE, "edge")):
            shapes = {getattr(self, name).shape for name, _ in group}
            if len(shapes) != 1 or len(next(iter(shapes))) != 1:
                raise SnapshotError("%s arrays (%s): one-dimensional and of one length" % (what, ", ".join(n for n, _ in group)))

    # -- sizes
    @property
    def games(self):
        return self.hdr.shape[0]

    @property
    def nodes(self):
        return self.nchild.shape[0]

    @property
    def edges(self):
        return self.act.shape[0]

    @staticmethod
    def header_nbytes(board):
        """Bytes of one game's fixed-size part: its hdr row, gauss, stream and move row."""
        return 4 * _lib.AO_SNAP_HDR + 8 + 4 * 624 + 4 * board * board

    @property
    def nbytes(self):
        """25 * edges + 12 * nodes + games * header_nbytes(board): the bytes of all arrays."""
        return sum(getattr(self, name).nbytes for name, _ in _GAME + _NODE + _EDGE)

    def game_nbytes(self, i):
        return 25 * int(self.hdr[i, 1]) + 12 * int(self.hdr[i, 0]) + self.header_nbytes(self.board)

    # -- the C view
    def _struct(self):
        s = _lib.AoTreeSnapshot(board=self.board, inplanes=self.inplanes, win_mark=self.win_mark, sims=self.sims, noise=self.noise,
                                games=self.games, c_puct=self.c_puct, nodes=self.nodes, edges=self.edges)
        for name, _ in _GAME + _NODE + _EDGE:
            a = getattr(self, name)
            setattr(s, name, a.ctypes.data_as(dict(_lib.AoTreeSnapshot._fields_)[name]))
        return s

    def check(self):
        """Consistency (ao_tree_snapshot_check; needs no device). Raises SnapshotError naming the first violation."""
        L = _lib.load()
        s = self._struct()
        if L.ao_tree_snapshot_check(C.byref(s)):
            raise SnapshotError(L.ao_last_error(None).decode())
        return self

    # -- subsets
    def select(self, indices):
        """The snapshot of the listed games, in the listed order."""
        idx = [int(i) for i in indices]
        for i in idx:
            if i < 0 or i >= self.games:
                raise IndexError("snapshot game %d of %d" % (i, self.games))
        n1 = np.concatenate([[0], np.cumsum(self.hdr[:, 0], dtype=np.int64)])
        e1 = np.concatenate([[0], np.cumsum(self.hdr[:, 1], dtype=np.int64)])
        if n1[-1] != self.nodes or e1[-1] != self.edges:
            raise SnapshotError("nodes / edges: the games' counts do not sum to the array lengths")
        arrays = {name: getattr(self, name)[idx] for name, _ in _GAME}
        for group, at in ((_NODE, n1), (_EDGE, e1)):
            for name, dt in group:
                a = getattr(self, name)
                arrays[name] = np.concatenate([a[at[i]:at[i + 1]] for i in idx]) if idx else np.zeros(0, dt)
        return TreeSnapshot(self.board, self.inplanes, self.win_mark, self.sims, self.noise, self.c_puct, **arrays)

    # -- files
    def save(self, path):
        """Writes an uncompressed .npz to exactly `path`."""
        meta = np.array([_FORMAT, self.board, self.inplanes, self.win_mark, self.sims, self.noise], np.int64)
        with open(path, "wb") as f:
            np.savez(f, meta=meta, c_puct=np.array([self.c_puct], np.float64),
                     **{name: getattr(self, name) for name, _ in _GAME + _NODE + _EDGE})

    @classmethod
    def load(cls, path):
        """Reads what save() wrote (allow_pickle=False) and checks it."""
        with np.load(path, allow_pickle=False) as z:
            if "meta" not in z.files or "c_puct" not in z.files:
                raise SnapshotError("%s: not a tree snapshot" % path)
            meta = z["meta"]
            if meta.shape != (6,) or int(meta[0]) != _FORMAT:
                raise SnapshotError("%s: unknown snapshot format" % path)
            arrays = {}
            for name, dt in _GAME + _NODE + _EDGE:
                if name not in z.files:
                    raise SnapshotError("%s lacks the array %r" % (path, name))
                if z[name].dtype != np.dtype(dt):
                    raise SnapshotError("%s: array %r is %s, not %s" % (path, name, z[name].dtype, np.dtype(dt)))
                arrays[name] = z[name]
            snap = cls(int(meta[1]), int(meta[2]), int(meta[3]), int(meta[4]), int(meta[5]), float(z["c_puct"][0]), **arrays)
        return snap.check()
