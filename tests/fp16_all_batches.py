"""Batches of the fp16-all tests (tests/test_fp16_all_host.py on the CPU, tests/test_gpu_fp16_all.py on the GPU).

The shapes of those tests are small on purpose (17 boards = two 16-board groups, one ragged). fp16_forward_nets.batch_of places
the structured boards of the pool at the seams of a batch, some of them twice (the full board at index 0 and on the last index,
a float-plane board's replacement twice), so a 17-board batch holds at most 15 distinct boards. `batch_of` here is that draw
with every LATER occurrence of a board replaced by a board of binary_pool(B) the batch does not hold yet, as long as there is
one: the first occurrences -- the structured boards at index 0 .. 4 -- stay where they are, and a batch of up to len(pool)
boards is all distinct.
"""
import numpy as np

import fp16_forward_nets as fn

# (blocks, board, boards) of every forward the GPU tests run on 0/1 boards
SHAPES = [(2, 9, 17), (2, 9, 1041), (2, 9, 3073), (1, 7, 33), (2, 4, 17), (1, 3, 16), (2, 15, 17), (2, 10, 33), (1, 12, 17)]


def batch_of(B, batch, seed=0):
    """Indices into fp16_forward_nets.binary_pool(B) of a batch of `batch` boards."""
    idx = np.array(fn.batch_of(B, batch, seed=seed))
    n = len(fn.binary_pool(B))
    unused = np.setdiff1d(np.arange(n), idx)
    unused = unused[np.random.RandomState(17 + batch + 7 * B + seed).permutation(len(unused))]
    seen, k = set(), 0
    for i, b in enumerate(idx):
        if b in seen and k < len(unused):
            idx[i] = unused[k]
            k += 1
        seen.add(int(idx[i]))
    return idx
