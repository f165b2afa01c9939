"""Host-side helpers with the reference's `utils` names and results (utils.py:22-239).

Inside a search these are HIP device code (tree_kernels.hip); the functions here serve the callers
on either side of the hot path: building training samples, sampling the played move from the
process-global numpy stream, data augmentation. Implementations are vectorised numpy.
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view


def legal_actions(node_id, board_size):
    """Empty cells in the reference's order (utils.py:22-27): iteration order of a CPython set
    difference, ascending except in deep endgames."""
    return list(set(range(board_size * board_size)) - set(node_id[1:]))


def get_board(node_id, board_size):
    """+1 black / -1 white, black moves first (utils.py:171-179). float64 [B, B]."""
    flat = np.zeros(board_size * board_size)
    mv = np.asarray(node_id[1:], dtype=np.int64)
    flat[mv[0::2]] = 1.0
    flat[mv[1::2]] = -1.0
    return flat.reshape(board_size, board_size)


def get_turn(node_id):
    """0 = black to move, 1 = white to move (utils.py:182-186)."""
    return 0 if len(node_id) % 2 == 1 else 1


def check_win(board, win_mark):
    """0 playing / 1 black / 2 white / 3 draw (utils.py:30-59). Windows are visited row-major and
    black is tested before white inside a window, like the reference's scan."""
    b = np.asarray(board)
    n = b.shape[0]
    k = win_mark
    if n >= k:
        win = sliding_window_view(b, (k, k))                      # [n-k+1, n-k+1, k, k]
        rows = win.sum(axis=3)                                    # horizontal lines
        cols = win.sum(axis=2)                                    # vertical lines
        d1 = np.trace(win, axis1=2, axis2=3)
        d2 = np.trace(win[:, :, ::-1, :], axis1=2, axis2=3)
        black = (rows == k).any(axis=2) | (cols == k).any(axis=2) | (d1 == k) | (d2 == k)
        white = (rows == -k).any(axis=2) | (cols == -k).any(axis=2) | (d1 == -k) | (d2 == -k)
        hit = np.flatnonzero((black | white).ravel())
        if hit.size:
            return 1 if black.ravel()[hit[0]] else 2
    if np.count_nonzero(b) == n * n:
        return 3
    return 0


# flag bits of one audited ply (audit_moves, PositionBatch.audit)
WIN_AVAILABLE, WIN_TAKEN, THREAT, BLOCKED, LOST = 1, 2, 4, 8, 16


def check_win_boards(boards, win_mark):
    """check_win for a stack of boards [n, B, B]: int32 [n]. The same scan -- windows row-major, black before white inside
    a window -- with the line sums taken once per start cell for all boards instead of once per window and board."""
    b = np.asarray(boards).astype(np.int8)
    n, B, k = b.shape[0], b.shape[1], win_mark
    win = np.where((b != 0).all(axis=(1, 2)), 3, 0).astype(np.int32)
    W = B - k + 1
    if n == 0 or W < 1:
        return win
    b = np.ascontiguousarray(b.transpose(1, 2, 0))                           # [B, B, n]: every slice below is long runs
    # sums of the k cells of the line that STARTS at a cell: to the right, downwards, down-right, down-left
    right = sum(b[:, i:i + W] for i in range(k))                             # [B, W, n]
    down = sum(b[i:i + W] for i in range(k))                                 # [W, B, n]
    diag = sum(b[i:i + W, i:i + W] for i in range(k))                        # [W, W, n]
    anti = sum(b[i:i + W, k - 1 - i:k - 1 - i + W] for i in range(k))        # [W, W, n], by the window's top-left cell

    def windows_with_line(total):
        hit = (diag == total) | (anti == total)
        in_row, in_col = right == total, down == total
        for i in range(k):                                                   # the window's k rows and k columns
            hit |= in_row[i:i + W]
            hit |= in_col[:, i:i + W]
        return hit.reshape(W * W, n)

    black, white = windows_with_line(k), windows_with_line(-k)
    either = black | white
    first = either.argmax(axis=0)
    decided = either.any(axis=0)
    win[decided] = np.where(black[first[decided], decided], 1, 2)
    return win


def win_cells(board, turn, win_mark):
    """The cells that win at once, by the definition alone: try every empty cell with check_win (all the tried boards in
    one check_win_boards call). No reference counterpart; pinned to the reference's check_win (utils.py:30-59). `board`
    [B, B] of +1 black / -1 white / 0, `turn` 0 black / 1 white to move. Returns (mine, theirs), bool [A]: cell c is in
    `mine` if check_win(board) == 0, c is empty and check_win of the board with a stone of the mover on c is the mover's
    win index (overlines count; a move that only fills the board, win index 3, does not); `theirs` the same for the
    opponent, as if it were to move. Both are empty on a terminal board. This is the yardstick the device is held to: A
    whole-board scans per colour, obviously right rather than fast."""
    b = np.asarray(board).astype(np.int8)
    A = b.size
    sets = np.zeros((2, A), bool)
    if check_win(b, win_mark) != 0:
        return sets[0], sets[1]
    empty = np.flatnonzero(b.ravel() == 0)
    tried = np.repeat(b.reshape(1, 1, A), empty.size, axis=1).repeat(2, axis=0)      # [who, empty cell, A]
    for who, colour in ((0, turn), (1, 1 - turn)):
        tried[who, np.arange(empty.size), empty] = 1 if colour == 0 else -1
    win = check_win_boards(tried.reshape((2 * empty.size,) + b.shape), win_mark).reshape(2, empty.size)
    sets[0, empty] = win[0] == turn + 1
    sets[1, empty] = win[1] == 2 - turn
    return sets[0], sets[1]


def audit_moves(moves, board_size, win_mark):
    """The tactical audit of ONE record of legal moves (black first): (flags uint8 [A], counts int32 [8]). flags[t]
    describes the move moves[t] played in the position before it, while that position is not terminal: WIN_AVAILABLE
    mine not empty, WIN_TAKEN the move is in mine, THREAT mine empty and theirs not, BLOCKED a THREAT and the move is in
    theirs, LOST a THREAT with two or more cells in theirs (win_cells). Plies from the first terminal position on, and
    beyond the record, are 0. counts: plies audited, WIN_AVAILABLE, wins missed, single threats (THREAT without LOST),
    blocks missed, LOST, end_ply (index of the first move after which check_win is non-zero, -1 if none), final
    check_win. ValueError for a move off the board or onto a stone."""
    A = board_size * board_size
    moves = [int(m) for m in moves]
    if len(moves) > A:
        raise ValueError("%d moves on a board of %d cells" % (len(moves), A))
    flags = np.zeros(A, np.uint8)
    counts = np.zeros(8, np.int32)
    board = np.zeros(A)
    for t, m in enumerate(moves):
        if not 0 <= m < A:
            raise ValueError("move %d is off the board" % m)
        if board[m] != 0:
            raise ValueError("move %d is onto a stone" % m)
        board[m] = 1.0 if t % 2 == 0 else -1.0
    # check_win after every move: the first non-zero one ends the audit
    after = np.zeros((len(moves), board_size, board_size))
    for t in range(len(moves)):
        after[t] = get_board([0] + moves[:t + 1], board_size)
    status = check_win_boards(after, win_mark)
    end_ply = int(np.flatnonzero(status)[0]) if status.any() else -1
    board = np.zeros(A)
    for t, m in enumerate(moves):
        if end_ply < 0 or t <= end_ply:
            mine, theirs = win_cells(board.reshape(board_size, board_size), t % 2, win_mark)
            f = 0
            if mine.any():
                f = WIN_AVAILABLE | (WIN_TAKEN if mine[m] else 0)
            elif theirs.any():
                f = THREAT | (BLOCKED if theirs[m] else 0) | (LOST if theirs.sum() >= 2 else 0)
            flags[t] = f
            counts[0] += 1
            counts[1] += bool(f & WIN_AVAILABLE)
            counts[2] += bool(f & WIN_AVAILABLE) and not f & WIN_TAKEN
            counts[3] += bool(f & THREAT) and not f & LOST
            counts[4] += bool(f & THREAT) and not f & LOST and not f & BLOCKED
            counts[5] += bool(f & LOST)
        board[m] = 1.0 if t % 2 == 0 else -1.0
    counts[6] = end_ply
    counts[7] = status[-1] if moves else 0
    return flags, counts


def get_state_pt(node_id, board_size, channel_size):
    """Network input planes, float64 [C, B, B] (utils.py:139-168): the stones of the mover of each
    of the last C-1 plies as they stood after that ply, oldest first, then the colour plane."""
    A = board_size * board_size
    mv = np.asarray(node_id[1:], dtype=np.int64)
    k = mv.size
    planes = np.zeros((channel_size, A))
    for j in range(channel_size - 1):
        ply = k - j                      # X_{k-j}
        if ply < 1:
            continue
        own = mv[(ply - 1) % 2:ply:2]    # moves of that ply's mover up to and including it
        planes[channel_size - 2 - j, own] = 1.0
    planes[channel_size - 1, :] = 1.0 if k % 2 == 0 else 0.0
    return planes.reshape(channel_size, board_size, board_size)


def states_of_episodes(moves, ep_of, ply_of, board_size, channel_size, dtype=np.float64, chunk=256):
    """get_state_pt for MANY positions at once: sample i is the root (0, m_1, ..., m_t) of episode ep_of[i] after
    t = ply_of[i] of its moves (moves [E, L] int, -1 padded). Returns [N, C, B, B] of `dtype`, equal entry for entry
    to np.stack([get_state_pt(...)]) (utils.py:139-168) -- cumulative stone sets per colour, then one gather per
    history plane instead of a Python call per sample. Episodes are processed `chunk` at a time, so the temporaries
    (one-hot and cumulative stone sets, [chunk, L, A] bytes each) stay at a few MB whatever E is."""
    moves = np.asarray(moves, dtype=np.int64)
    ep_of = np.asarray(ep_of, dtype=np.int64)
    ply_of = np.asarray(ply_of, dtype=np.int64)
    E, L = moves.shape
    A = board_size * board_size
    N = ep_of.shape[0]
    out = np.zeros((N, channel_size, A), dtype)
    out[:, channel_size - 1, :] = (ply_of % 2 == 0).astype(dtype)[:, None]
    if N == 0:
        return out.reshape(N, channel_size, board_size, board_size)
    by_ep = np.argsort(ep_of, kind="stable")              # (already sorted when the samples come from main.self_play)
    bounds = np.searchsorted(ep_of[by_ep], np.arange(0, E + chunk, chunk))
    par = (np.arange(L) % 2)[None, :, None]
    for c, e0 in enumerate(range(0, E, chunk)):
        sel = by_ep[bounds[c]:bounds[c + 1]]
        if sel.size == 0:
            continue
        mv = moves[e0:e0 + chunk]
        # cum[col, e, j] = stones of colour col (0 black: even move index) after the first j+1 moves of episode e0 + e
        onehot = np.zeros((mv.shape[0], L, A), np.uint8)
        ee, jj = np.nonzero(mv >= 0)
        onehot[ee, jj, mv[ee, jj]] = 1
        cum = np.empty((2,) + onehot.shape, np.uint8)
        np.cumsum(onehot * (par == 0), axis=1, dtype=np.uint8, out=cum[0])
        np.cumsum(onehot * (par == 1), axis=1, dtype=np.uint8, out=cum[1])
        e_loc, t = ep_of[sel] - e0, ply_of[sel]
        for j in range(channel_size - 1):
            p = t - j                         # X_p: the mover of (1-based) ply p after that ply; black moves the odd plies
            ok = np.flatnonzero(p >= 1)
            if ok.size:
                pp = p[ok]
                out[sel[ok], channel_size - 2 - j] = cum[(pp - 1) % 2, e_loc[ok], pp - 1]
    return out.reshape(N, channel_size, board_size, board_size)


class LazySamples:
    """The samples of one main.self_play call -- (state [C, B, B] f64, pi [A] f64, z float) as main.py:159-166 appends them --
    without the states: they are rebuilt (states_of_episodes, all of the block at once) the first time anyone looks at one.
    With rep_memory on the device the states are made there (ao_replay_extend_moves) and cur_memory is only ever counted,
    so nothing of size n x C x B x B is built on the host. Iterating yields one tuple-like entry per sample."""

    def __init__(self, moves, ep_of, ply_of, pis, z, board_size, channel_size):
        self.moves, self.ep_of, self.ply_of, self.pis = moves, ep_of, ply_of, pis
        self.z = np.asarray(z, dtype=np.float64).tolist()                     # Python floats, as the reference stores them
        self.board_size, self.channel_size = board_size, channel_size
        self._states = None

    def __len__(self):
        return len(self.z)

    def states(self):
        if self._states is None:
            self._states = states_of_episodes(self.moves, self.ep_of, self.ply_of, self.board_size, self.channel_size)
        return self._states

    def __iter__(self):
        return (LazySample(self, i) for i in range(len(self)))


class SampleQueue:
    """main.cur_memory: the reference's deque of (state, pi, z) tuples (main.py:56) -- len / iteration / indexing / append /
    extend / pop / popleft / clear -- that can also take a whole LazySamples block by reference: extend(block) is O(1), no
    per-sample object exists until somebody iterates or indexes (main.train only ever counts cur_memory)."""
    maxlen = None

    def __init__(self, iterable=()):
        self._seg = []          # [block, lo, hi] (LazySamples, live range) or a plain list of entries
        self.extend(iterable)

    def __len__(self):
        return sum(g[2] - g[1] if _is_block(g) else len(g) for g in self._seg)

    def __bool__(self):
        return len(self) > 0

    def _tail_list(self):
        if not self._seg or _is_block(self._seg[-1]):
            self._seg.append([])
        return self._seg[-1]

    def append(self, x):
        self._tail_list().append(x)

    def extend(self, iterable):
        if isinstance(iterable, LazySamples):
            if len(iterable):
                self._seg.append(_Block((iterable, 0, len(iterable))))
        else:
            self._tail_list().extend(iterable)

    def clear(self):
        self._seg = []

    def _drop_empty(self):
        self._seg = [g for g in self._seg if (g[2] - g[1] if _is_block(g) else len(g)) > 0]

    def pop(self):
        self._drop_empty()
        if not self._seg:
            raise IndexError("pop from an empty SampleQueue")
        g = self._seg[-1]
        if _is_block(g):
            g[2] -= 1
            return LazySample(g[0], g[2])
        return g.pop()

    def popleft(self):
        self._drop_empty()
        if not self._seg:
            raise IndexError("pop from an empty SampleQueue")
        g = self._seg[0]
        if _is_block(g):
            g[1] += 1
            return LazySample(g[0], g[1] - 1)
        return g.pop(0)

    def __iter__(self):
        for g in list(self._seg):
            if _is_block(g):
                for i in range(g[1], g[2]):
                    yield LazySample(g[0], i)
            else:
                yield from list(g)

    def __getitem__(self, i):
        n = len(self)
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(n))]
        if i < 0:
            i += n
        if not 0 <= i < n:
            raise IndexError("SampleQueue index out of range")
        for g in self._seg:
            m = g[2] - g[1] if _is_block(g) else len(g)
            if i < m:
                return LazySample(g[0], g[1] + i) if _is_block(g) else g[i]
            i -= m
        raise IndexError("SampleQueue index out of range")


class _Block(list):
    """[LazySamples, lo, hi]: a block segment of a SampleQueue (a list subclass so that it is told apart from a list of entries)"""


def _is_block(g):
    return type(g) is _Block


class LazySample:
    """One entry of LazySamples: unpacks, indexes and compares like the tuple (state, pi, z)."""
    __slots__ = ("_blk", "_i")

    def __init__(self, blk, i):
        self._blk, self._i = blk, i

    def _tuple(self):
        b, i = self._blk, self._i
        return (b.states()[i], b.pis[i], b.z[i])

    def __iter__(self):
        return iter(self._tuple())

    def __getitem__(self, k):
        return self._tuple()[k]

    def __len__(self):
        return 3


def get_action(pi):
    """Sample the played move from np.random (utils.py:189-195). Returns (one-hot, index)."""
    n = len(pi)
    idx = np.random.choice(n, p=pi)
    onehot = np.zeros(n)
    onehot[idx] = 1
    return onehot, idx


def argmax_onehot(pi):
    """Uniform choice among the maxima of pi (utils.py:198-205). Returns (one-hot, index)."""
    best = np.flatnonzero(pi == pi.max())
    idx = best[np.random.choice(len(best))]
    onehot = np.zeros(len(pi))
    onehot[idx] = 1
    return onehot, idx


def augment_dataset(memory, board_size):
    """8 symmetries per sample in the reference's order r0, r0f, r1, r1f, ... (utils.py:226-239)."""
    out = []
    for s, pi, z in memory:
        grid = pi.reshape(board_size, board_size)
        for r in range(4):
            s_r = np.rot90(s, r, axes=(1, 2))
            p_r = np.rot90(grid, r)
            out.append((s_r.copy(), p_r.reshape(-1).copy(), z))
            out.append((s_r[:, :, ::-1].copy(), p_r[:, ::-1].reshape(-1).copy(), z))
    return out
