"""Device-resident replay memory: the reference's `rep_memory = deque(maxlen=MEMORY_SIZE)`
(main.py:55) kept in HBM, with `utils.augment_dataset` (utils.py:226-239) run on the device and
mini-batches assembled on the device (main.py:262-292).

Behaves like the deque for everything main.py does with it: len(), maxlen, extend(),
iteration / indexing (entries come back as the reference's (state f64 [C,B,B], pi f64 [A], z)
tuples), clear(). `extend_augmented(samples)` == `extend(utils.augment_dataset(samples, B))`.

`ReplaySnapshot` is the memory, or a range of it, as packed host data (planes as bits, pi as a cell mask and its non-zero
values, lossless): `DeviceReplay.export_snapshot` / `import_snapshot` pack and unpack it on the device
(csrc/replay_snapshot.hip), `from_arrays` / `to_arrays` do the same in numpy, `save` / `load` keep it in an .npz file."""
import ctypes as C

import numpy as np

from . import _lib


class ReplayError(RuntimeError):
    pass


_SNAP = (("kind", np.uint8), ("z", np.float32), ("bits", np.uint64), ("pi_mask", np.uint64), ("pi_val", np.float64),
         ("raw", np.float32))
_FORMAT = 1
_ONE_F32 = 0x3f800000


def _pack_bits(flags, words):
    """bool [..., A] -> uint64 [..., words]: bit (c % 64) of word c / 64 is flags[..., c]."""
    padded = np.zeros(flags.shape[:-1] + (64 * words,), bool)
    padded[..., :flags.shape[-1]] = flags
    return np.ascontiguousarray(np.packbits(padded, axis=-1, bitorder="little")).view("<u8").astype(np.uint64)


def _unpack_bits(words, cells):
    """uint64 [..., W] -> bool [..., cells]: the inverse of _pack_bits."""
    b = np.ascontiguousarray(words.astype("<u8")).view(np.uint8)
    return np.unpackbits(b, axis=-1, bitorder="little")[..., :cells].astype(bool)


class ReplaySnapshot:
    """The replay memory, or a range of it, as host data (ao_replay_snapshot, include/omok_hip.h): entries only, in deque
    order, oldest first. What `DeviceReplay.export_snapshot` returns and `DeviceReplay.import_snapshot` takes; `.save` /
    `.load` keep it in an `.npz` file; `from_arrays` / `to_arrays` are the same packing in numpy -- the format's executable
    definition, and the way a reference pickle or a plain deque becomes a snapshot and back.

    Arrays (numpy, C-contiguous), W = (A + 63) // 64: kind uint8 [n] (0 = planes as bits, 1 = planes raw); z float32 [n];
    bits uint64 [n, C, W] (bit set where the plane holds exactly 1.0f; zero on kind-1 rows); pi_mask uint64 [n, W] (bit set
    where the 64-bit pattern of pi is non-zero); pi_val float64 [sum of the masks' popcounts] (those patterns, ascending
    cell order, entry after entry); raw float32 [number of kind-1 entries, C, A]. An entry is kind 0 only when every plane
    value has the bit pattern of +0.0f or 1.0f. The form is canonical: one memory content has exactly one snapshot."""

    def __init__(self, board, inplanes, **arrays):
        self.board, self.inplanes = int(board), int(inplanes)
        for name, dt in _SNAP:
            if name not in arrays:
                raise ReplayError("snapshot lacks the array %r" % name)
            setattr(self, name, np.ascontiguousarray(arrays[name], dt))
        n, A, W = self.kind.shape[0] if self.kind.ndim == 1 else -1, self.board ** 2, self.words
        if self.kind.shape != (n,) or self.z.shape != (n,) or self.bits.shape != (n, self.inplanes, W) or self.pi_mask.shape != (n, W):
            raise ReplayError("kind / z / bits / pi_mask: shapes must be [n], [n], [n, %d, %d], [n, %d]" % (self.inplanes, W, W))
        if self.pi_val.ndim != 1 or self.raw.ndim != 3 or self.raw.shape[1:] != (self.inplanes, A):
            raise ReplayError("pi_val / raw: shapes must be [pi_values], [raw_entries, %d, %d]" % (self.inplanes, A))

    @property
    def words(self):
        return (self.board ** 2 + 63) // 64

    def __len__(self):
        return self.kind.shape[0]

    @property
    def nbytes(self):
        """(5 + 8 W (C + 1)) per entry + 8 per non-zero pi cell + 4 C A per kind-1 entry: the bytes of all arrays."""
        return sum(getattr(self, name).nbytes for name, _ in _SNAP)

    # -- the C view
    def _struct(self):
        s = _lib.AoReplaySnapshot(board=self.board, inplanes=self.inplanes, format=_FORMAT, words=self.words, entries=len(self),
                                  pi_values=self.pi_val.shape[0], raw_entries=self.raw.shape[0])
        for name, _ in _SNAP:
            setattr(s, name, getattr(self, name).ctypes.data_as(dict(_lib.AoReplaySnapshot._fields_)[name]))
        return s

    def check(self):
        """The canonical form (ao_replay_snapshot_check; needs no device). Raises ReplayError naming the first violation."""
        L = _lib.load()
        s = self._struct()
        if L.ao_replay_snapshot_check(C.byref(s)):
            raise ReplayError(L.ao_replay_last_error(None).decode())
        return self

    # -- the packing in numpy
    @classmethod
    def from_arrays(cls, states, pi, z, board, inplanes):
        """Packs states [n, C, B, B] (any float type; taken as float32), pi [n, A] (float64) and z [n] (float32)."""
        B, Cn = int(board), int(inplanes)
        A, W = B * B, (B * B + 63) // 64
        s = np.ascontiguousarray(np.asarray(states, np.float32).reshape(-1, Cn, A))
        p = np.ascontiguousarray(np.asarray(pi, np.float64).reshape(-1, A))
        zz = np.ascontiguousarray(np.asarray(z, np.float32).reshape(-1))
        if not s.shape[0] == p.shape[0] == zz.shape[0]:
            raise ReplayError("states, pi and z: %d, %d and %d entries" % (s.shape[0], p.shape[0], zz.shape[0]))
        u = s.view(np.uint32)
        one = u == _ONE_F32
        kind = ((u != 0) & ~one).any(axis=(1, 2)).astype(np.uint8)
        bits = _pack_bits(one & (kind == 0)[:, None, None], W)
        pu = p.view(np.uint64)
        nz = pu != 0
        return cls(B, Cn, kind=kind, z=zz, bits=bits, pi_mask=_pack_bits(nz, W), pi_val=pu[nz].view(np.float64), raw=s[kind == 1])

    def to_arrays(self):
        """The inverse of from_arrays, as DeviceReplay.read returns it: float64 states [n, C, B, B], pi [n, A], z [n]."""
        n, A, B = len(self), self.board ** 2, self.board
        s = np.where(_unpack_bits(self.bits, A), np.float32(1), np.float32(0)).astype(np.float32)
        s[self.kind == 1] = self.raw
        pu = np.zeros((n, A), np.uint64)
        pu[_unpack_bits(self.pi_mask, A)] = self.pi_val.view(np.uint64)
        return s.reshape(n, self.inplanes, B, B).astype(np.float64), pu.view(np.float64), self.z.astype(np.float64)

    # -- files
    def save(self, path):
        """Writes an uncompressed .npz to exactly `path`."""
        meta = np.array([_FORMAT, self.board, self.inplanes, self.words, len(self)], np.int64)
        with open(path, "wb") as f:
            np.savez(f, meta=meta, **{name: getattr(self, name) for name, _ in _SNAP})

    @classmethod
    def load(cls, path):
        """Reads what save() wrote (allow_pickle=False), checks the dtypes, then check()."""
        with np.load(path, allow_pickle=False) as f:
            if "meta" not in f.files:
                raise ReplayError("%s: not a replay snapshot" % path)
            meta = f["meta"]
            if meta.shape != (5,) or meta.dtype != np.int64 or int(meta[0]) != _FORMAT:
                raise ReplayError("%s: unknown snapshot format" % path)
            arrays = {}
            for name, dt in _SNAP:
                if name not in f.files:
                    raise ReplayError("%s lacks the array %r" % (path, name))
                if f[name].dtype != np.dtype(dt):
                    raise ReplayError("%s: array %r is %s, not %s" % (path, name, f[name].dtype, np.dtype(dt)))
                arrays[name] = f[name]
            snap = cls(int(meta[1]), int(meta[2]), **arrays)
        if int(meta[3]) != snap.words or int(meta[4]) != len(snap):
            raise ReplayError("%s: meta says %d words and %d entries, the arrays hold %d and %d" % (path, meta[3], meta[4], snap.words, len(snap)))
        return snap.check()


class DeviceReplay:
    def __init__(self, board_size, inplanes, maxlen, device=0):
        self._L = _lib.load()
        self.B, self.C, self.A = int(board_size), int(inplanes), int(board_size) ** 2
        self.device = int(device)
        h = C.c_void_p()
        if self._L.ao_replay_create(self.B, self.C, int(maxlen), self.device, C.byref(h)):
            raise ReplayError(self._L.ao_replay_last_error(None).decode())
        self._h = h

    def _check(self, rc, what):
        if rc:
            raise ReplayError("%s: %s" % (what, self._L.ao_replay_last_error(self._h).decode()))

    @property
    def maxlen(self):
        return int(self._L.ao_replay_capacity(self._h))

    def __len__(self):
        return int(self._L.ao_replay_size(self._h))

    def clear(self):
        self._check(self._L.ao_replay_clear(self._h), "ao_replay_clear")

    def _push(self, samples, augment):
        samples = list(samples)
        if not samples:
            return
        s = np.ascontiguousarray(np.stack([m[0] for m in samples]), dtype=np.float32)
        pi = np.ascontiguousarray(np.stack([m[1] for m in samples]), dtype=np.float64)
        z = np.ascontiguousarray(np.array([m[2] for m in samples]), dtype=np.float32)
        if s.shape[1:] != (self.C, self.B, self.B) or pi.shape[1:] != (self.A,):
            raise ReplayError("sample shapes %r / %r do not match the memory" % (s.shape[1:], pi.shape[1:]))
        self._check(self._L.ao_replay_extend(self._h, s.ctypes.data_as(C.POINTER(C.c_float)),
                                             pi.ctypes.data_as(C.POINTER(C.c_double)),
                                             z.ctypes.data_as(C.POINTER(C.c_float)), len(samples),
                                             1 if augment else 0, None), "ao_replay_extend")

    def extend(self, samples):
        """deque.extend: the samples as they are."""
        self._push(samples, False)

    def extend_augmented(self, samples):
        """rep_memory.extend(utils.augment_dataset(samples, board_size)) with the symmetries made on the device."""
        self._push(samples, True)

    def extend_augmented_arrays(self, states, pi, z):
        """extend_augmented for samples that already are arrays (states [n,C,B,B], pi [n,A], z [n], any float type):
        no per-sample Python objects, and only the samples whose symmetries can survive in the memory are converted
        and uploaded (the rest of the call just moves the ring position, ao_replay_extend_skip)."""
        n = int(states.shape[0])
        if n == 0:
            return
        if tuple(states.shape[1:]) != (self.C, self.B, self.B) or tuple(pi.shape[1:]) != (self.A,):
            raise ReplayError("sample shapes %r / %r do not match the memory" % (states.shape[1:], pi.shape[1:]))
        cap = self.maxlen
        first = 0
        if 8 * n > cap:
            first = max(0, n - (-(-cap // 8) + 1))
            if 8 * (n - first) < cap:
                first = 0
        s = np.ascontiguousarray(states[first:], dtype=np.float32)
        p = np.ascontiguousarray(pi[first:], dtype=np.float64)
        zz = np.ascontiguousarray(z[first:], dtype=np.float32)
        self._check(self._L.ao_replay_extend_skip(self._h, s.ctypes.data_as(C.POINTER(C.c_float)),
                                                  p.ctypes.data_as(C.POINTER(C.c_double)),
                                                  zz.ctypes.data_as(C.POINTER(C.c_float)), n - first, 1, first, None),
                    "ao_replay_extend_skip")

    def extend_augmented_moves(self, moves, ep_of, ply_of, pi, z):
        """extend_augmented_arrays without the states: sample i is the position of episode ep_of[i] after ply_of[i] of its
        moves (moves [E, L] action indices, -1 padded) and the planes of utils.get_state_pt (utils.py:139-168) are built by a
        kernel (ao_replay_extend_moves) -- nothing of size n x C x B x B exists on the host."""
        n = int(np.shape(ep_of)[0])
        if n == 0:
            return
        moves = np.asarray(moves)
        if moves.ndim != 2 or tuple(np.shape(pi)[1:]) != (self.A,) or np.shape(ply_of)[0] != n or np.shape(pi)[0] != n or np.shape(z)[0] != n:
            raise ReplayError("moves [E, L], ep_of / ply_of / z [n] and pi [n, %d] expected" % self.A)
        cap = self.maxlen
        first = 0
        if 8 * n > cap:
            first = max(0, n - (-(-cap // 8) + 1))
            if 8 * (n - first) < cap:
                first = 0
        mv = np.ascontiguousarray(moves[:, :self.A], dtype=np.int16)
        e = np.ascontiguousarray(ep_of[first:], dtype=np.int32)
        t = np.ascontiguousarray(ply_of[first:], dtype=np.int32)
        p = np.ascontiguousarray(pi[first:], dtype=np.float64)
        zz = np.ascontiguousarray(z[first:], dtype=np.float32)
        self._check(self._L.ao_replay_extend_moves(self._h, mv.ctypes.data_as(C.POINTER(C.c_int16)), mv.shape[0], mv.shape[1],
                                                   e.ctypes.data_as(C.POINTER(C.c_int32)), t.ctypes.data_as(C.POINTER(C.c_int32)),
                                                   p.ctypes.data_as(C.POINTER(C.c_double)), zz.ctypes.data_as(C.POINTER(C.c_float)),
                                                   n - first, 1, first, None), "ao_replay_extend_moves")

    def read(self, first, n):
        s = np.empty((n, self.C, self.B, self.B), np.float64)
        pi = np.empty((n, self.A), np.float64)
        z = np.empty(n, np.float64)
        dp = C.POINTER(C.c_double)
        self._check(self._L.ao_replay_read(self._h, int(first), int(n), s.ctypes.data_as(dp), pi.ctypes.data_as(dp),
                                           z.ctypes.data_as(dp)), "ao_replay_read")
        return s, pi, z

    def export_snapshot(self, first=0, n=None, chunk_bytes=0):
        """Deque entries [first, first + n) (n = None: to the end) as a ReplaySnapshot, packed on the device
        (ao_replay_export): only packed bytes are downloaded, in chunks of chunk_bytes (0 = 64 MiB). Read-only on the memory."""
        first = int(first)
        n = len(self) - first if n is None else int(n)
        pv, re = C.c_int64(), C.c_int64()
        self._check(self._L.ao_replay_export_size(self._h, first, n, C.byref(pv), C.byref(re)), "ao_replay_export_size")
        W = (self.A + 63) // 64
        snap = ReplaySnapshot(self.B, self.C, kind=np.empty(n, np.uint8), z=np.empty(n, np.float32), bits=np.empty((n, self.C, W), np.uint64),
                              pi_mask=np.empty((n, W), np.uint64), pi_val=np.empty(pv.value, np.float64),
                              raw=np.empty((re.value, self.C, self.A), np.float32))
        s = snap._struct()
        self._check(self._L.ao_replay_export(self._h, first, n, C.byref(s), int(chunk_bytes), None), "ao_replay_export")
        if (s.entries, s.pi_values, s.raw_entries) != (n, pv.value, re.value):
            raise ReplayError("ao_replay_export: packed %d / %d / %d where the count pass had %d / %d / %d"
                              % (s.entries, s.pi_values, s.raw_entries, n, pv.value, re.value))
        return snap

    def import_snapshot(self, snap, chunk_bytes=0):
        """deque.extend(the snapshot's entries), unpacked on the device (ao_replay_import): only what can survive in the
        memory is uploaded. Refused with the memory untouched when board or inplanes differ or the snapshot fails check()."""
        s = snap._struct()
        self._check(self._L.ao_replay_import(self._h, C.byref(s), int(chunk_bytes), None), "ao_replay_import")

    def __getitem__(self, i):
        n = len(self)
        if isinstance(i, slice):
            idx = range(*i.indices(n))
            return [self[j] for j in idx]
        if i < 0:
            i += n
        if not 0 <= i < n:
            raise IndexError("replay index out of range")
        s, pi, z = self.read(i, 1)
        return s[0], pi[0], float(z[0])

    def __iter__(self):
        n = len(self)
        step = 4096
        for f in range(0, n, step):
            s, pi, z = self.read(f, min(step, n - f))
            for k in range(s.shape[0]):
                yield s[k], pi[k], float(z[k])

    def batch(self, indices):
        """float32 cuda tensors (s [m,C,B,B], pi [m,A], z [m]) for deque indices -- what main.train builds with
        torch.tensor(np.stack(...)).to(device).float() (main.py:283-290)."""
        import torch
        idx = np.ascontiguousarray(np.asarray(indices, dtype=np.int64))
        m = int(idx.shape[0])
        dev = torch.device("cuda", self.device)
        s = torch.empty((m, self.C, self.B, self.B), dtype=torch.float32, device=dev)
        pi = torch.empty((m, self.A), dtype=torch.float32, device=dev)
        z = torch.empty((m,), dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        self._check(self._L.ao_replay_gather(self._h, idx.ctypes.data_as(C.POINTER(C.c_int64)), m, s.data_ptr(),
                                             pi.data_ptr(), z.data_ptr(), stream), "ao_replay_gather")
        return s, pi, z

    def close(self):
        if getattr(self, "_h", None):
            self._L.ao_replay_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
