"""Times the replay snapshot against what main.save_dataset does with a device replay memory.

    python tools/time_replay_snapshot.py [--entries 200000] [--repeats 3] [--out DIR]

Fills a 9x9, 5-plane DeviceReplay from seeded self-play-like samples (positions after 0..39 random moves, eight symmetries
each; half of the samples have a one-hot pi, the other half a pi over the empty cells), then prints the time of
export_snapshot and import_snapshot (every repeat, wall clock around the call: both return with the data complete), the
packed bytes and the .npz size, and for the same ring the parent's way out: deque(list(memory)) followed by pickling.
No threshold, nothing asserted but the round trip itself."""
import argparse
import os
import pickle
import sys
import tempfile
import time
from collections import deque

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def fill(mem, entries, seed):
    B, A, plies = mem.B, mem.A, 40
    n = entries // 8
    E = -(-n // plies)
    rs = np.random.RandomState(seed)
    moves = np.stack([rs.permutation(A)[:plies] for _ in range(E)]).astype(np.int16)
    ep_of = np.repeat(np.arange(E, dtype=np.int32), plies)[:n]
    ply_of = np.tile(np.arange(plies, dtype=np.int32), E)[:n]
    when = np.full((E, A), plies, np.int32)               # ply that fills the cell
    when[np.arange(E)[:, None], moves] = np.arange(plies)[None, :]
    empty = when[ep_of] >= ply_of[:, None]                # [n, A] the cell is empty before ply t
    w = rs.rand(n, A) * empty
    pi = w / w.sum(axis=1, keepdims=True)
    onehot = np.arange(n) % 2 == 0
    hot = np.zeros_like(pi)
    hot[np.arange(n), pi.argmax(axis=1)] = 1.0
    pi[onehot] = hot[onehot]
    z = rs.choice([-1.0, 1.0, 0.0], n, p=[0.45, 0.45, 0.1])
    mem.extend_augmented_moves(moves, ep_of, ply_of, pi, z)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=200_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="directory for the two files (default: a temporary one, removed at the end)")
    a = ap.parse_args()

    import torch
    from alpha_omok_amd.build import source_hash
    from alpha_omok_amd.replay import DeviceReplay, ReplaySnapshot

    tmp = None
    if a.out is None:
        tmp = tempfile.TemporaryDirectory()
        a.out = tmp.name
    os.makedirs(a.out, exist_ok=True)
    mem = DeviceReplay(9, 5, a.entries)
    fill(mem, a.entries, a.seed)
    n = len(mem)
    print("# replay snapshot vs pickled deque: 9x9, 5 planes, %d entries (%d B each in the ring = %.1f MB); %s; source hash %s"
          % (n, 4 * 5 * 81 + 8 * 81 + 4, n * 2272 / 1e6, torch.cuda.get_device_name(0), source_hash()))

    def clock(f):
        t0 = time.perf_counter()
        r = f()
        return r, time.perf_counter() - t0

    snap = None
    for k in range(a.repeats):
        snap, t = clock(mem.export_snapshot)
        print("export_snapshot   run %d: %8.1f ms  (%.2f GB/s of ring read, packed %.2f GB/s)" % (k, 1e3 * t, n * 2272 / t / 1e9, snap.nbytes / t / 1e9))
    print("packed bytes      %d = %.1f B per entry (ring: 2272 B; %d kind-1 entries, %.2f non-zero pi cells per entry)"
          % (snap.nbytes, snap.nbytes / n, int(snap.kind.sum()), snap.pi_val.shape[0] / n))
    path = os.path.join(a.out, "replay_snapshot.npz")
    _, t = clock(lambda: snap.save(path))
    print("save (.npz)       %8.1f ms, %d bytes" % (1e3 * t, os.path.getsize(path)))
    loaded, t = clock(lambda: ReplaySnapshot.load(path))
    print("load + check      %8.1f ms" % (1e3 * t))
    dst = DeviceReplay(9, 5, a.entries)
    for k in range(a.repeats):
        dst.clear()
        _, t = clock(lambda: dst.import_snapshot(loaded))
        print("import_snapshot   run %d: %8.1f ms" % (k, 1e3 * t))
    same = all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for f in range(0, n, 50_000)
               for x, y in zip(mem.read(f, min(50_000, n - f)), dst.read(f, min(50_000, n - f))))
    print("restored ring     %s" % ("bit for bit the original" if same else "DIFFERS"))
    dst.close()

    # the parent's way: main.save_dataset does deque(list(memory)) and pickles it
    dq, t1 = clock(lambda: deque(list(mem), maxlen=mem.maxlen))
    ppath = os.path.join(a.out, "dataset.pickle")

    def dump():
        with open(ppath, "wb") as f:
            pickle.dump(dq, f, pickle.HIGHEST_PROTOCOL)
    _, t2 = clock(dump)
    print("save_dataset way  deque(list(memory)) %8.1f ms + pickle %8.1f ms = %8.1f ms, %d bytes = %.1f B per entry"
          % (1e3 * t1, 1e3 * t2, 1e3 * (t1 + t2), os.path.getsize(ppath), os.path.getsize(ppath) / n))
    mem.close()
    if tmp is not None:
        tmp.cleanup()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
