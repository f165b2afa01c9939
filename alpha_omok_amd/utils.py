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


FW_NONE, FW_WIN, FW_UNKNOWN = 0, 1, 2      # `result` of forced_win / PositionBatch.forced_wins
FW_MAX_DEPTH, FW_MAX_NODES = 16, 65536


class _OutOfNodes(Exception):
    pass


class ArrayPosition:
    """A position for forced_win with the two inner questions asked literally: check_win and win_cells of the board array.
    Slow; the yardstick WindowPosition is held to."""

    def __init__(self, board_size, win_mark):
        self.B, self.k = board_size, win_mark
        self.board = np.zeros(board_size * board_size, np.int8)

    def place(self, cell, colour):
        self.board[cell] = 1 if colour == 0 else -1

    def remove(self, cell, colour):
        self.board[cell] = 0

    def terminal(self):
        return check_win(self.board.reshape(self.B, self.B), self.k) != 0

    def win_cells(self, turn):
        mine, theirs = win_cells(self.board.reshape(self.B, self.B), turn, self.k)
        return np.flatnonzero(mine).tolist(), np.flatnonzero(theirs).tolist()

    def empty_cells(self):
        return np.flatnonzero(self.board == 0).tolist()


class WindowPosition(ArrayPosition):
    """The same answers from a table of all k-windows (the k cells of every line segment of length k, four directions)
    with the stones of either colour counted per window as stones come and go: the board has a line if a window holds k
    stones of one colour, and a window holding k-1 stones of one colour and one empty cell marks that cell as a winning
    cell of the colour (a stone there completes the window; an overline contains a window). In the style of
    check_win_boards: the same definition, asked of sums that are kept instead of recomputed. A window's two counts are
    kept as one code, black + 8 white, and a table turns the code into what the window says: 0 nothing, 1 / 2 black /
    white is one stone short of it and nothing else is in it, 3 it is a line."""
    _tables = {}

    def __init__(self, board_size, win_mark):
        ArrayPosition.__init__(self, board_size, win_mark)
        key = (board_size, win_mark)
        if key not in self._tables:
            B, k = key
            wins = []
            for r in range(B):
                for c in range(B):
                    for dr, dc in ((0, 1), (1, 0), (1, 1), (1, -1)):
                        if 0 <= r + (k - 1) * dr < B and 0 <= c + (k - 1) * dc < B:
                            wins.append([(r + i * dr) * B + c + i * dc for i in range(k)])
            wins = np.array(wins, np.int64).reshape(-1, k)
            through = [np.flatnonzero((wins == cell).any(axis=1)) for cell in range(B * B)]
            says = np.zeros(9 * k + 1, np.int8)
            says[[k - 1, 8 * (k - 1)]] = 1, 2
            says[[k, 8 * k]] = 3
            self._tables[key] = (wins, through, says)
        self.windows, self.through, self.says = self._tables[key]
        self.code = np.zeros(self.windows.shape[0], np.int64)
        self.stones = 0
        self._said = None                     # says[code] of the position as it stands

    def place(self, cell, colour):
        ArrayPosition.place(self, cell, colour)
        self.code[self.through[cell]] += 1 + 7 * colour
        self.stones += 1
        self._said = None

    def remove(self, cell, colour):
        ArrayPosition.remove(self, cell, colour)
        self.code[self.through[cell]] -= 1 + 7 * colour
        self.stones -= 1
        self._said = None

    def _look(self):
        if self._said is None:
            said = self.says[self.code]
            self._said = (said, int(said.max()) if said.size else 0)
        return self._said

    def terminal(self):
        return self.stones == self.board.size or self._look()[1] == 3

    def win_cells(self, turn):
        said, top = self._look()
        if top == 0 or self.terminal():
            return [], []
        out = []
        for colour in (turn, 1 - turn):
            cells = self.windows[said == colour + 1].ravel()
            out.append(np.unique(cells[self.board[cells] == 0]).tolist())
        return out[0], out[1]


def forced_win(moves, board_size, win_mark, max_depth=8, max_nodes=2000, position=WindowPosition, attacker=None):
    """Is there a forced win by continuous fours (VCF) for the side to move in the position reached by `moves` (legal moves,
    black first)? No reference counterpart; defined through check_win / win_cells alone. The attacker a is the side to
    move, cells are always tried in ascending order, and `nodes` counts the wins_within calls of all iterations:

        wins_within(P, d): a to move, at most d attacker moves. No on a terminal P. With (mine, theirs) = win_cells(P, a):
            yes if mine is not empty; no if d == 1 or theirs holds two or more cells; otherwise yes if four(P, c, d) for
            some c of theirs (a single threat must be answered) or, theirs empty, of all empty cells -- the first such c.
        four(P, c, d): P1 = P with a on c. No on a terminal P1. With (his, replies) = win_cells(P1, 1 - a): no if his is
            not empty (the defender wins first) or replies is empty (c made no four); yes if wins_within(P1 with the
            defender on b, d - 1) for EVERY b of replies.
        for D = 1 .. max_depth (iterative deepening, no iteration skipped): the root is wins_within(P, D), except that it
            tries every candidate and collects those that succeed (mine, if that is not empty) into `moves`; the first
            D with moves ends the search: result 1, depth D.

    Returns a dict: result (FW_NONE no forced win within max_depth, FW_WIN, FW_UNKNOWN: the wins_within call number
    max_nodes + 1 was asked for -- then nodes is max_nodes and everything else of the search is zero / -1 / empty, even if
    a winning move had been found in that iteration), depth (attacker moves, 0 unless result is 1), moves (bool [A]: every
    first move that wins within depth), move (min(moves) or -1), line (list: min(moves), min(replies), then at every
    later attacker node the first c that succeeded or min(mine), the defender always on min(replies); it ends on the stone
    that makes the line and may be shorter than 2 depth - 1), line_len, nodes, status (check_win of the position), turn, and stats
    (host only: `block_fours` nodes at which a candidate taken from theirs succeeded, `multi_reply` fours with two or more
    replies that were tried). ValueError for an illegal move list or limits outside 1..16 / 1..65536.
    `position`: WindowPosition (fast) or ArrayPosition (check_win / win_cells of the array, literally).
    `attacker`: None for the side to move, or 0 / 1 to name the attacker whatever the parity of `moves` -- the side that is
    not to move is then searched as if the mover had passed; `turn` of the result is the attacker. ValueError otherwise."""
    if attacker is not None and (isinstance(attacker, bool) or not isinstance(attacker, (int, np.integer)) or attacker not in (0, 1)):
        raise ValueError("attacker must be None, 0 or 1, got %r" % (attacker,))
    for name, v, hi in (("max_depth", max_depth, FW_MAX_DEPTH), ("max_nodes", max_nodes, FW_MAX_NODES)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= hi:
            raise ValueError("%s must be an integer in 1..%d, got %r" % (name, hi, v))
    A = board_size * board_size
    moves = [int(m) for m in moves]
    if len(moves) > A:
        raise ValueError("%d moves on a board of %d cells" % (len(moves), A))
    pos = position(board_size, win_mark)
    for t, m in enumerate(moves):
        if not 0 <= m < A:
            raise ValueError("move %d is off the board" % m)
        if pos.board[m] != 0:
            raise ValueError("move %d is onto a stone" % m)
        pos.place(m, t % 2)
    a = len(moves) % 2 if attacker is None else int(attacker)
    stats = dict(block_fours=0, multi_reply=0)
    count = [0]
    won = []                                  # the root's collection

    def wins_within(d, root=False):
        """None for no, else the line from here"""
        count[0] += 1
        if count[0] > max_nodes:
            raise _OutOfNodes()
        if pos.terminal():
            return None
        mine, theirs = pos.win_cells(a)
        if mine:
            if root:
                won.extend(mine)
            return [mine[0]]
        if d == 1 or len(theirs) >= 2:
            return None
        first = None
        for c in (theirs if theirs else pos.empty_cells()):
            line = four(c, d)
            if line is not None:
                stats["block_fours"] += bool(theirs)
                if not root:
                    return line
                won.append(c)
                first = first or line
        return first

    def four(c, d):
        pos.place(c, a)
        try:
            if pos.terminal():                # (only the full board: c is not in mine)
                return None
            his, replies = pos.win_cells(1 - a)
            if his or not replies:
                return None
            stats["multi_reply"] += len(replies) >= 2
            line = None
            for b in replies:
                pos.place(b, 1 - a)
                try:
                    rest = wins_within(d - 1)
                finally:
                    pos.remove(b, 1 - a)
                if rest is None:
                    return None
                line = line or [c, b] + rest
            return line
        finally:
            pos.remove(c, a)

    out = dict(result=FW_NONE, depth=0, moves=np.zeros(A, bool), move=-1, line=[], line_len=0, nodes=0,
               status=check_win(get_board([0] + moves, board_size), win_mark), turn=a, stats=stats)
    try:
        for D in range(1, max_depth + 1):
            line = wins_within(D, root=True)
            if won:
                out["moves"][won] = True
                out.update(result=FW_WIN, depth=D, move=min(won), line=line, line_len=len(line))
                break
    except _OutOfNodes:
        out.update(result=FW_UNKNOWN, nodes=max_nodes)
        return out
    out["nodes"] = count[0]
    return out


FD_NONE, FD_SAFE, FD_LOSES, FD_UNKNOWN = 0, 1, 2, 3     # `reply` of forced_defences / PositionBatch.forced_defences


def forced_defences(moves, board_size, win_mark, max_depth=8, max_nodes=2000):
    """Which replies hold against the opponent's forced win by continuous fours? For the position P after `moves` (legal
    moves, black first) with mover m and opponent o, by forced_win alone, A + 1 searches each with its own budget of
    max_nodes, none skipped on the strength of another one's answer:

        threat, threat_depth, threat_moves: result, depth, moves of forced_win(moves, attacker=o) -- what o could do if m
            passed.
        for every empty cell c, r = forced_win(moves + [c]) with o to move: reply[c] = 1 + r.result, depth[c] = r.depth.

    Returns a dict: threat, threat_depth, threat_moves (bool [A]), reply (uint8 [A]: FD_NONE not an empty cell, FD_SAFE the
    reply holds -- also a c that ends the game: the position after it is terminal and forced_win says no --, FD_LOSES,
    FD_UNKNOWN that search ran out of nodes), depth (uint8 [A], non-zero only where LOSES), counts (int32 [4]: empty cells,
    SAFE, LOSES, UNKNOWN), nodes (the sum over all searches run), status (check_win of P), turn (m). On a terminal P every
    output but status and turn is zero / empty: nothing is searched. Argument errors as forced_win."""
    A = board_size * board_size
    moves = [int(m) for m in moves]
    first = forced_win(moves, board_size, win_mark, max_depth, max_nodes, attacker=1 - len(moves) % 2)
    out = dict(threat=FW_NONE, threat_depth=0, threat_moves=np.zeros(A, bool), reply=np.zeros(A, np.uint8),
               depth=np.zeros(A, np.uint8), counts=np.zeros(4, np.int32), nodes=0, status=first["status"], turn=len(moves) % 2)
    if first["status"] != 0:
        return out
    out.update(threat=first["result"], threat_depth=first["depth"], threat_moves=first["moves"], nodes=first["nodes"])
    taken = set(moves)
    for c in range(A):
        if c in taken:
            continue
        r = forced_win(moves + [c], board_size, win_mark, max_depth, max_nodes)
        out["reply"][c] = 1 + r["result"]
        out["depth"][c] = r["depth"]
        out["nodes"] += r["nodes"]
    out["counts"][:] = [A - len(moves)] + [int((out["reply"] == v).sum()) for v in (FD_SAFE, FD_LOSES, FD_UNKNOWN)]
    return out


RT_NONE, RT_WIN, RT_DEFEND, RT_LOST = 0, 1, 2, 3       # `verdict` of root_tactics / Engine.root_tactics


def root_tactics(moves, board_size, win_mark, max_depth=6, max_nodes=512):
    """What the forced-win solver says about searching the position P after `moves` (legal moves, black first), by
    forced_win alone -- the host definition of Engine.root_tactics. With mover m and opponent o:

        a terminal P: verdict RT_NONE, everything zero / empty, nothing searched.
        own = forced_win(moves). own.result == FW_WIN: RT_WIN, allowed = own.moves, depth = own.depth.
        otherwise threat = forced_win(moves, attacker=o). threat.result != FW_WIN: RT_NONE, allowed = every empty cell.
        otherwise every empty cell c is tried as forced_defences does, r = forced_win(moves + [c]): allowed = the cells with
            r.result != FW_WIN (a reply whose search ran out of nodes stays searchable), depth = threat.depth. Nothing
            allowed: RT_LOST, and allowed is every empty cell again (the search is left alone when all is lost); else
            RT_DEFEND.

    Returns a dict: verdict, depth, allowed (bool [A]), nodes (the sum over the searches actually run, each with its own
    budget of max_nodes) and unknown (bit 0 set where own ran out of nodes, bit 1 the threat's search, bit 2 any reply's).
    The replies are searched only under a proven threat with no win of one's own: that is what makes it affordable for
    every move of a batch of games. Argument errors as forced_win."""
    A = board_size * board_size
    moves = [int(m) for m in moves]
    out = dict(verdict=RT_NONE, depth=0, allowed=np.zeros(A, bool), nodes=0, unknown=0)
    own = forced_win(moves, board_size, win_mark, max_depth, max_nodes)
    if own["status"] != 0:
        return out
    out["nodes"] = own["nodes"]
    if own["result"] == FW_WIN:
        out.update(verdict=RT_WIN, depth=own["depth"], allowed=own["moves"].copy())
        return out
    out["unknown"] |= int(own["result"] == FW_UNKNOWN)
    empty = np.ones(A, bool)
    empty[moves] = False
    threat = forced_win(moves, board_size, win_mark, max_depth, max_nodes, attacker=1 - len(moves) % 2)
    out["nodes"] += threat["nodes"]
    out["unknown"] |= 2 * int(threat["result"] == FW_UNKNOWN)
    out["allowed"] = empty
    if threat["result"] != FW_WIN:
        return out
    holds = np.zeros(A, bool)
    for c in np.flatnonzero(empty):
        r = forced_win(moves + [int(c)], board_size, win_mark, max_depth, max_nodes)
        out["nodes"] += r["nodes"]
        out["unknown"] |= 4 * int(r["result"] == FW_UNKNOWN)
        holds[c] = r["result"] != FW_WIN
    out["depth"] = threat["depth"]
    if holds.any():
        out.update(verdict=RT_DEFEND, allowed=holds)
    else:
        out["verdict"] = RT_LOST
    return out


LEAF_MAX_NODES = 1024        # Engine.set_leaf_tactics: max_nodes 1..1024 (the solver runs once per simulation)


def leaf_tactics_value(moves, board_size, win_mark, value, max_depth, max_nodes):
    """The value of the leaf reached by `moves` under leaf tactics (Engine.set_leaf_tactics), by forced_win alone: exactly
    np.float32(1.0) where the side to move has a proven forced win by continuous fours -- the value is the leaf mover's own
    (the search backs up -value into the leaf's record) -- and `value` as it is otherwise: no forced win within max_depth, a
    search that ran out of max_nodes (FW_UNKNOWN), a terminal position. No reference counterpart."""
    if forced_win(moves, board_size, win_mark, max_depth, max_nodes)["result"] == FW_WIN:
        return np.float32(1.0)
    return value


def leaf_tactics_evaluator(evaluator, board_size, win_mark, max_depth, max_nodes):
    """The evaluator of a search with leaf tactics, around evaluator(moves, planes, sim) -> (policy, value): the policy as it
    is, the value through leaf_tactics_value. A search with the switch on is the reference search under this evaluator."""
    def f(moves, planes, sim):
        p, v = evaluator(moves, planes, sim)
        return p, leaf_tactics_value(moves, board_size, win_mark, v, max_depth, max_nodes)
    return f


def leaf_tactics_limits(leaf_tactics):
    """The leaf_tactics= argument of ZeroAgent / evaluate_batched / main.configure as (max_depth, max_nodes), or None for off
    (None / False): True is the default 2 / 16 -- see Engine.set_leaf_tactics --, a dict names max_depth and / or
    max_nodes. ValueError for anything else or limits outside 1..16 / 1..LEAF_MAX_NODES."""
    if leaf_tactics is None or leaf_tactics is False:
        return None
    if leaf_tactics is True:
        d, n = 2, 16
    elif isinstance(leaf_tactics, dict):
        extra = set(leaf_tactics) - {"max_depth", "max_nodes"}
        if extra:
            raise ValueError("leaf_tactics: unknown keys %r" % sorted(extra))
        d, n = leaf_tactics.get("max_depth", 2), leaf_tactics.get("max_nodes", 16)
    else:
        raise ValueError("leaf_tactics must be None, False, True or a dict(max_depth, max_nodes), got %r" % (leaf_tactics,))
    for name, v, hi in (("max_depth", d, FW_MAX_DEPTH), ("max_nodes", n, LEAF_MAX_NODES)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= hi:
            raise ValueError("leaf_tactics: %s must be an integer in 1..%d, got %r" % (name, hi, v))
    return int(d), int(n)


def parse_leaf_tactics(text):
    """The command line's --leaf-tactics value "DEPTH,NODES" as the dict configure(leaf_tactics=) takes; None stays None."""
    if text is None:
        return None
    parts = str(text).split(",")
    if len(parts) != 2:
        raise ValueError("--leaf-tactics takes DEPTH,NODES, got %r" % (text,))
    return dict(max_depth=int(parts[0]), max_nodes=int(parts[1]))


# proven outcomes (Engine.tree_proofs / utils.tree_proofs): a node's status for its side to move; Engine.set_proof_moves' verdicts
PROOF_UNKNOWN, PROOF_WIN, PROOF_LOSS, PROOF_DRAW = 0, 1, 2, 3
PM_NONE, PM_WIN, PM_PRUNED, PM_MOVED = 0, 1, 2, 3
_PROOF_FLIP = (PROOF_UNKNOWN, PROOF_LOSS, PROOF_WIN, PROOF_DRAW)


def tree_proofs(snapshot, game, max_len=None):
    """What game `game` of a TreeSnapshot (Engine.export_trees) PROVES, by exact minimax over the tree as it stands -- the
    definition of Engine.tree_proofs. No reference counterpart: the reference stores a visited terminal child like any other and
    only its backed-up value tells. Every expanded node gets a status for its side to move and the plies to the end of the game.
    An edge, seen from the node's mover: a CH_TERMINAL child -- the stone is placed and check_win asked -- is (WIN, 1) if the
    mover has won, (DRAW, 1) on a full board; an expanded child c is its status with WIN and LOSS swapped and plies[c] + 1; an
    unvisited child (a barred root child is one) is UNKNOWN. A node: any WIN edge -> (WIN, fewest plies); else any UNKNOWN edge ->
    UNKNOWN; else any DRAW edge -> (DRAW, fewest plies among the draws); else (LOSS, most plies). The proof line: from the root,
    while the node is proven, the first edge in stored order that carries the node's own (status, plies).
    Returns a dict: root int32 [4] = status, plies, proven nodes, nodes walked; child_status int8 [A] (-1: the root has no edge
    for the action) and child_plies int16 [A] by action; line int32 [max_len] (-1 beyond it; max_len None: A) and len; status
    int8 / plies int32 [nodes] for every node in the snapshot's breadth-first numbering."""
    s = snapshot
    B = s.board
    A = B * B
    L = A if max_len is None else int(max_len)
    n0 = int(s.hdr[:game, 0].sum())
    e0 = int(s.hdr[:game, 1].sum())
    N = int(s.hdr[game, 0])
    nch = s.nchild[n0:n0 + N].astype(np.int64)
    first = e0 + np.concatenate([[0], np.cumsum(nch)])[:N]
    moves = [int(a) for a in s.moves[game, :int(s.hdr[game, 2])]]
    # the moves that lead to every node: breadth first, a parent comes before its children
    path = [None] * N
    for j in range(N):
        if j == 0:
            path[j] = moves
        else:
            par, pe = int(s.parent[n0 + j]), int(s.parent_edge[n0 + j])
            path[j] = path[par] + [int(s.act[first[par] + pe])]
    status, plies = np.zeros(N, np.int8), np.zeros(N, np.int32)

    def edges(j):
        """[(status, plies)] of node j's edges in stored order"""
        out = []
        for k in range(int(nch[j])):
            at = first[j] + k
            c = int(s.child[at])
            if c >= 0:
                cs = int(status[c])
                out.append((_PROOF_FLIP[cs], int(plies[c]) + 1 if cs != PROOF_UNKNOWN else 0))
            elif c == -2:                                   # CH_TERMINAL
                mv = path[j] + [int(s.act[at])]
                w = check_win(get_board([0] + mv, B), s.win_mark)
                mover = 1 + (len(path[j]) & 1)              # check_win's index of the side that placed the stone
                out.append((PROOF_WIN, 1) if w == mover else ((PROOF_DRAW, 1) if w == 3 else (PROOF_UNKNOWN, 0)))
            else:
                out.append((PROOF_UNKNOWN, 0))
        return out

    for j in range(N - 1, -1, -1):
        ev = edges(j)
        wins = [p for st, p in ev if st == PROOF_WIN]
        draws = [p for st, p in ev if st == PROOF_DRAW]
        if wins:
            status[j], plies[j] = PROOF_WIN, min(wins)
        elif not ev or any(st == PROOF_UNKNOWN for st, _ in ev):
            status[j], plies[j] = PROOF_UNKNOWN, 0
        elif draws:
            status[j], plies[j] = PROOF_DRAW, min(draws)
        else:
            status[j], plies[j] = PROOF_LOSS, max(p for _, p in ev)
    child_status, child_plies = np.full(A, -1, np.int8), np.zeros(A, np.int16)
    line, n = np.full(L, -1, np.int32), 0
    root = np.zeros(4, np.int32)
    if N:
        for k, (st, p) in enumerate(edges(0)):
            a = int(s.act[first[0] + k])
            child_status[a], child_plies[a] = st, p
        root[:] = (status[0], plies[0], int(np.count_nonzero(status)), N)
        j = 0
        while status[j] != PROOF_UNKNOWN and n < L:
            k = edges(j).index((int(status[j]), int(plies[j])))
            line[n] = s.act[first[j] + k]
            n += 1
            j = int(s.child[first[j] + k])
            if j < 0:
                break
    return dict(root=root, child_status=child_status, child_plies=child_plies, line=line, len=n, status=status, plies=plies)


def proof_pi(pi, visit, child_status, child_plies):
    """What Engine.set_proof_moves makes of one game's pi [A] (Engine.end_move) given the root's edge values by action
    (tree_proofs): (pi', verdict).
    PM_WIN: some edge is WIN -- pi' is one-hot on the WIN edge with the fewest plies, ties to the larger visit, then to the lowest
    action. PM_PRUNED: no WIN edge, some edge is LOSS, some is not, and some LOSS edge has pi > 0 -- with s the sum of pi over the
    edges that are not LOSS (sequential in ascending action order, fp64), pi' = pi / s on them and 0 elsewhere; if s == 0 (a
    tau == 0 one-hot on a lost move) the verdict is PM_MOVED and pi' is one-hot on the non-lost edge with the most visits, lowest
    action on ties. PM_NONE: everything else, a root proven LOSS included -- pi' is `pi` itself."""
    pi = np.asarray(pi, np.float64)
    st = np.asarray(child_status)
    win = np.flatnonzero(st == PROOF_WIN)
    if win.size:
        a = min(win, key=lambda a: (int(child_plies[a]), -float(visit[a]), int(a)))
        out = np.zeros_like(pi)
        out[a] = 1.0
        return out, PM_WIN
    lost = st == PROOF_LOSS
    keep = (st == PROOF_UNKNOWN) | (st == PROOF_DRAW)
    if not (lost.any() and keep.any() and (pi[lost] > 0).any()):
        return pi, PM_NONE
    s = 0.0
    for a in np.flatnonzero(keep):
        s = s + float(pi[a])
    out = np.zeros_like(pi)
    if s > 0:
        out[keep] = pi[keep] / s
        return out, PM_PRUNED
    out[min(np.flatnonzero(keep), key=lambda a: (-float(visit[a]), int(a)))] = 1.0
    return out, PM_MOVED


def check_allowed(allowed, games, cells):
    """The `allowed` argument of Engine.begin_move / search as uint8 [games, cells] (None stays None). ValueError for
    another shape or for values that are not 0 / 1 / bool."""
    if allowed is None:
        return None
    a = np.asarray(allowed)
    if a.shape != (games, cells):
        raise ValueError("allowed must have shape (%d, %d), got %r" % (games, cells, a.shape))
    if a.dtype != bool and not (np.issubdtype(a.dtype, np.integer) and ((a == 0) | (a == 1)).all()):
        raise ValueError("allowed must be bool or 0 / 1 integers")
    return np.ascontiguousarray(a, np.uint8)


def root_bar(allowed, ids, board_size):
    """The host definition of the root move restriction: bool [G, A], True where game g's root child on that cell is
    barred from the move -- the empty cells of the position of ids[g] (a reference id (0, a1, a2, ...)) that allowed[g]
    does not name. Ones on occupied cells are ignored; a row that allows every empty cell bars nothing. ValueError for a
    bad shape (check_allowed) or a row that allows none of its game's empty cells (a full board has none to allow)."""
    A = board_size * board_size
    a = check_allowed(allowed, len(ids), A).astype(bool)
    bar = np.zeros_like(a)
    for g, rid in enumerate(ids):
        empty = np.ones(A, bool)
        empty[list(rid)[1:]] = False
        bar[g] = empty & ~a[g]
        if empty.any() and not (empty & a[g]).any():
            raise ValueError("game %d: the root bar allows no empty cell of the position" % g)
    return bar


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


def move_decided(visits, remaining):
    """Is the most-visited move of a search already certain? visits: the root children's visit counts (any shape, e.g. the [A]
    visit vector of get_pi), remaining: simulations the search still owes. Every simulation adds exactly one visit to exactly
    one root child, so with n1 >= n2 the two largest counts (n2 = 0 with fewer than two entries) the leader cannot be caught,
    or even tied, iff n1 - n2 > remaining: argmax_onehot of the finished search then picks it without a draw among equals.
    No reference counterpart (the reference always runs num_mcts simulations); the device rule of k_settle is this one."""
    v = np.sort(np.asarray(visits).reshape(-1))
    n1 = int(v[-1]) if v.size >= 1 else 0
    n2 = int(v[-2]) if v.size >= 2 else 0
    return n1 - n2 > int(remaining)


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


# ---- the eight symmetries of the board as index maps (csrc/symmetry.hpp holds the same functions; the two agree bit for bit) ----
def sym_cell(s, c, board_size):
    """Source cell of output cell c under symmetry s = 2*r + f (rot90 by r, then a flip of the last axis if f; the order of
    augment_dataset): sym_planes(X, s)[..., c] = X[..., sym_cell(s, c)]. c may be an array."""
    B = board_size
    c = np.asarray(c)
    i, j = c // B, c % B
    jj = B - 1 - j if s & 1 else j
    r = s >> 1
    if r == 0:
        si, sj = i, jj
    elif r == 1:
        si, sj = jj, B - 1 - i
    elif r == 2:
        si, sj = B - 1 - i, B - 1 - jj
    else:
        si, sj = B - 1 - jj, i
    out = si * B + sj
    return int(out) if out.ndim == 0 else out


def sym_inverse(s):
    """The symmetry that undoes s: the opposite rotation; a rotation followed by a flip is a reflection and undoes itself."""
    return s if s & 1 else (8 - s) & 7


def sym_cell_inv(s, d, board_size):
    """Where source cell d goes under s: the c with sym_cell(s, c) == d."""
    return sym_cell(sym_inverse(s), d, board_size)


def sym_planes(x, s, board_size=None):
    """x under symmetry s, same shape: the s-th state augment_dataset makes of x. x is [..., B, B], or flat [..., A] when
    board_size is given and the last two axes are not (B, B)."""
    x = np.asarray(x)
    B = x.shape[-1] if board_size is None else board_size
    A = B * B
    grid = x.ndim >= 2 and x.shape[-2:] == (B, B)
    flat = x.reshape(x.shape[:-2] + (A,)) if grid else x
    return flat[..., sym_cell(s, np.arange(A), B)].reshape(x.shape)


def sym_policy_back(p, s, board_size=None):
    """The policy in the board's own frame, given the network's answer p [..., A] on sym_planes(X, s):
    out[sym_cell(s, c)] = p[c]."""
    p = np.asarray(p)
    A = p.shape[-1]
    if board_size is None:
        board_size = int(round(np.sqrt(A)))
    out = np.empty_like(p)
    out[..., sym_cell(s, np.arange(A), board_size)] = p
    return out


def leaf_symmetry(key, ply, sim):
    """The symmetry (0..7) under which the leaf with `ply` stones is evaluated in simulation `sim` (0-based inside the move) of
    the game with key `key`; arithmetic mod 2^32. Stateless: host, oracle and device compute it independently."""
    M = 0xFFFFFFFF
    x = (int(key) ^ (int(ply) * 0x9E3779B1) ^ (int(sim) * 0x85EBCA77)) & M
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M
    x ^= x >> 15
    x = (x * 0x846CA68B) & M
    x ^= x >> 16
    return x >> 29


def leaf_key(base, seed):
    """The key of a game from the caller's base key and the game's seed (Engine.set_leaf_symmetry)."""
    return (int(base) ^ (int(seed) * 0xC2B2AE35)) & 0xFFFFFFFF
