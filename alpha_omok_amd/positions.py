"""`PositionBatch`: stateless questions about positions you name, answered on the device in batches.

Who has won this board (utils.check_win, utils.py:30-59)? Which moves are legal, whose turn is it, what does the board
look like (utils.py:22-27, 171-186)? What are the input planes (utils.get_state_pt, utils.py:139-168)? What does the
network say about these n positions (ZeroAgent.get_pv, agents.py:252-260)? No Engine, no tree, no game is involved: one
wavefront per position (csrc/positions.hip), any number of positions per call.

Positions are given as ids. With `leading_zero=True` (the default) every id is a reference-style root id
`(0, a1, a2, ...)` and MUST start with the 0; with `leading_zero=False` every id is the bare move list `(a1, a2, ...)`.
Nothing is guessed from the content: a bare list may well begin with move 0.

Mistakes of shape or type raise ValueError on the host, before any device call (pack_boards, pack_ids). Mistakes INSIDE a
position -- a move off the board, a stone on an occupied cell, more moves than cells -- are that position's own: its
`err` is 1, 2 or 3, its outputs are zero, and the rest of the batch is unaffected.
"""
import ctypes as C

import numpy as np

from . import _lib
from .engine import EngineError, _ptr

ERR_OK, ERR_RANGE, ERR_OCCUPIED, ERR_LENGTH = 0, 1, 2, 3
# flag bits of one audited ply (PositionBatch.audit; the same values as utils.audit_moves)
WIN_AVAILABLE, WIN_TAKEN, THREAT, BLOCKED, LOST = 1, 2, 4, 8, 16
# `result` of PositionBatch.forced_wins and the limits of its search (the same values as utils.forced_win)
FW_NONE, FW_WIN, FW_UNKNOWN = 0, 1, 2
FW_MAX_DEPTH, FW_MAX_NODES = 16, 65536
# `reply` of PositionBatch.forced_defences (the same values as utils.forced_defences)
FD_NONE, FD_SAFE, FD_LOSES, FD_UNKNOWN = 0, 1, 2, 3
_CTYPE = {np.int32: C.c_int32, np.uint8: C.c_uint8, np.int16: C.c_int16}   # of an output array's dtype (PositionBatch._ask)


def default_win_mark(board_size):
    """The reference's rule (agents.py:46): 3 on a 3x3 board, 5 otherwise."""
    return 3 if board_size == 3 else 5


def check_config(board_size, inplanes, win_mark, capacity):
    """ValueError for a PositionBatch configuration the device workspace would refuse (ao_positions_create)."""
    for name, v in (("board_size", board_size), ("inplanes", inplanes), ("win_mark", win_mark), ("capacity", capacity)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s must be an integer, got %r" % (name, v))
    if not 3 <= board_size <= 15:
        raise ValueError("board_size must be in 3..15, got %d" % board_size)
    if not 1 <= inplanes <= 9:
        raise ValueError("inplanes must be in 1..9, got %d" % inplanes)
    if not 3 <= win_mark <= 5:
        raise ValueError("win_mark must be in 3..5, got %d" % win_mark)
    if win_mark > board_size:
        raise ValueError("win_mark %d does not fit a %dx%d board" % (win_mark, board_size, board_size))
    if capacity < 1:
        raise ValueError("capacity must be >= 1, got %d" % capacity)


def pack_boards(boards, board_size):
    """boards: [n, B, B] (or one [B, B] board) of +1 black / -1 white / 0 empty, any integer or float dtype ->
    contiguous int8 [n, B, B]. ValueError for another shape, a non-numeric dtype or any other value."""
    try:
        b = np.asarray(boards)
    except Exception as e:
        raise ValueError("boards are not an array: %s" % e)
    if b.dtype == object or b.dtype.kind not in "iuf":
        raise ValueError("boards must be a numeric array of +1 / -1 / 0 (ragged input or dtype %s)" % b.dtype)
    if b.ndim == 2:
        b = b[None]
    if b.ndim != 3 or b.shape[1:] != (board_size, board_size):
        raise ValueError("boards must have shape [n, %d, %d], got %s" % (board_size, board_size, tuple(b.shape)))
    if not np.isin(b, (-1, 0, 1)).all():
        raise ValueError("boards may hold +1 (black), -1 (white) and 0 (empty) only")
    return np.ascontiguousarray(b, np.int8)


def pack_ids(root_ids, leading_zero=True):
    """root_ids: a sequence of ids, each a flat sequence of integers -> (moves int32 [n, stride], n int32 [n]), the
    bare move lists padded with 0. leading_zero=True: reference-style ids (0, a1, ...), the 0 is checked and dropped;
    False: bare move lists. ValueError for an id that is not a flat sequence of integers (nested or ragged inside, floats
    with a fraction, strings), that lacks its leading 0, or whose entries do not fit int32. The VALUES of the moves are not
    judged here: a bad move is its position's `err`."""
    if isinstance(root_ids, np.ndarray) and root_ids.ndim != 2:
        raise ValueError("root_ids as an array must be [n, length], got shape %s" % (tuple(root_ids.shape),))
    try:
        ids = list(root_ids)
    except TypeError:
        raise ValueError("root_ids must be a sequence of ids")
    rows = []
    for k, rid in enumerate(ids):
        if isinstance(rid, (str, bytes)) or not hasattr(rid, "__len__"):
            raise ValueError("id %d is not a sequence of moves: %r" % (k, rid))
        try:
            a = np.asarray(rid)
        except Exception:
            raise ValueError("id %d is ragged: %r" % (k, rid))
        if a.size == 0:
            a = np.zeros(0, np.int64)
        if a.dtype == object or a.ndim != 1:
            raise ValueError("id %d is not a flat sequence of integers: %r" % (k, rid))
        if a.dtype.kind == "f":
            if not np.all(a == np.floor(a)):
                raise ValueError("id %d holds a move that is not an integer: %r" % (k, rid))
        elif a.dtype.kind not in "iu":
            raise ValueError("id %d is not a sequence of integers (dtype %s)" % (k, a.dtype))
        if a.size and (a.min() < -2 ** 31 or a.max() > 2 ** 31 - 1):
            raise ValueError("id %d holds a move beyond int32" % k)
        a = a.astype(np.int64)
        if leading_zero:
            if a.size == 0 or a[0] != 0:
                raise ValueError("id %d is not a reference-style id (0, a1, a2, ...): %r -- pass leading_zero=False for "
                                 "bare move lists" % (k, rid))
            a = a[1:]
        rows.append(a)
    n = np.array([r.size for r in rows], np.int32).reshape(len(rows))
    stride = int(n.max()) if len(rows) else 0
    moves = np.zeros((len(rows), max(stride, 1)), np.int32)
    for k, r in enumerate(rows):
        moves[k, :r.size] = r
    return moves, n


def _check_limits(max_depth, max_nodes):
    """ValueError for search limits ao_positions_forced_wins / ao_positions_forced_defences would refuse"""
    for name, v, hi in (("max_depth", max_depth, FW_MAX_DEPTH), ("max_nodes", max_nodes, FW_MAX_NODES)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= hi:
            raise ValueError("%s must be an integer in 1..%d, got %r" % (name, hi, v))


class PositionBatch:
    """Device workspace for batched position queries (ao_positions_*, include/omok_hip.h).

    win_mark=None follows ZeroAgent: 3 on a 3x3 board, 5 otherwise. `capacity` positions go through the device per
    launch; a call may name more, it is then worked through in chunks. Use as a context manager or call close()."""

    def __init__(self, board_size, inplanes=5, win_mark=None, capacity=4096, device=0):
        if win_mark is None:
            win_mark = default_win_mark(board_size)
        check_config(board_size, inplanes, win_mark, capacity)
        self._h = None
        self._L = _lib.load()
        h = C.c_void_p()
        if self._L.ao_positions_create(int(board_size), int(inplanes), int(win_mark), int(capacity), int(device), C.byref(h)):
            raise EngineError("ao_positions_create: " + self._L.ao_positions_last_error(None).decode())
        self._h = h
        self.board_size, self.inplanes, self.win_mark = int(board_size), int(inplanes), int(win_mark)
        self.capacity, self.device = int(capacity), int(device)
        self.A = self.board_size * self.board_size
        self._evaluator = None

    def _check(self, rc, what):
        if rc:
            raise EngineError("%s: %s" % (what, self._L.ao_positions_last_error(self._h).decode()))

    def _handle(self):
        if not self._h:
            raise EngineError("PositionBatch is closed")
        return self._h

    # -- raw boards
    def check_win(self, boards):
        """utils.check_win for every board of [n, B, B] (+1 / -1 / 0): int32 [n] of 0 playing, 1 black, 2 white, 3 draw."""
        b = pack_boards(boards, self.board_size)
        win = np.zeros(b.shape[0], np.int32)
        self._check(self._L.ao_positions_check_win(self._handle(), _ptr(b, C.c_int8), b.shape[0], _ptr(win, C.c_int32)),
                    "ao_positions_check_win")
        return win

    # -- positions by id
    def _from_moves(self, root_ids, leading_zero, host, planes_ptr):
        moves, n = pack_ids(root_ids, leading_zero)
        cnt = n.shape[0]
        out = {}
        if host:
            B = self.board_size
            out = dict(status=np.zeros(cnt, np.int32), end_ply=np.zeros(cnt, np.int32), turn=np.zeros(cnt, np.int32),
                       board=np.zeros((cnt, B, B), np.int8), legal=np.zeros((cnt, self.A), np.uint8),
                       err=np.zeros(cnt, np.int32))
        g = out.get
        self._check(self._L.ao_positions_from_moves(
            self._handle(), _ptr(moves, C.c_int32), moves.shape[1], _ptr(n, C.c_int32), cnt,
            _ptr(g("status"), C.c_int32), _ptr(g("end_ply"), C.c_int32), _ptr(g("turn"), C.c_int32), _ptr(g("board"), C.c_int8),
            _ptr(g("legal"), C.c_uint8), planes_ptr(cnt) if planes_ptr else None, _ptr(g("err"), C.c_int32)),
            "ao_positions_from_moves")
        return out

    def describe(self, root_ids, leading_zero=True):
        """dict of arrays, one row per id: status (check_win of the final board), end_ply (index into the id's moves of
        the first one after which check_win is non-zero, -1 if none), turn (utils.get_turn), board (utils.get_board as
        int8 [n, B, B]), legal (uint8 [n, A], 1 on empty cells), err (0 ok, 1 move off the board, 2 occupied cell,
        3 more moves than cells). Rows with err != 0 are all zero."""
        return self._from_moves(root_ids, leading_zero, True, None)

    def planes(self, root_ids, leading_zero=True):
        """utils.get_state_pt for every id: torch float32 [n, C, B, B] on the device (zeros where the id has an error)."""
        import torch
        box = []

        def alloc(cnt):
            box.append(torch.empty((cnt, self.inplanes, self.board_size, self.board_size), dtype=torch.float32,
                                   device=torch.device("cuda", self.device)))
            return box[0].data_ptr() if cnt else None

        self._from_moves(root_ids, leading_zero, False, alloc)
        return box[0]

    def _native(self, model):
        if hasattr(model, "forward_ptr"):        # an engine.Net
            return model
        if self._evaluator is None:
            from .evaluator import Evaluator
            self._evaluator = Evaluator(self.device)
            self._evaluator.strict_native = True
        net = self._evaluator.native_net(model, self.board_size, self.inplanes)
        if net is None:
            raise ValueError("evaluate needs a module in the PVNet wire format for a %dx%d board and %d input planes "
                             "(or an engine.Net)" % (self.board_size, self.board_size, self.inplanes))
        return net

    def evaluate(self, model, root_ids, leading_zero=True, symmetries=1):
        """ZeroAgent.get_pv for every id in one call: (policy float32 [n, A] -- the softmax over all cells, nothing masked --,
        value float32 [n], status int32 [n], err int32 [n]). Terminal positions are evaluated too (status says which they
        are); ids with err != 0 get zeros. `model`: a module in the PVNet wire format (exported to the native forward as
        ZeroAgent does, re-exported when its parameters change) or an engine.Net. symmetries=8: the mean over the eight
        symmetries of the board, each policy brought back into the board's own frame (ao_positions_evaluate_sym: one forward
        over eight rows per position, fp32 sum in the order s = 0..7, times 1/8; capacity >= 8); 1: the position as it stands."""
        if symmetries not in (1, 8):
            raise ValueError("symmetries must be 1 or 8")
        moves, n = pack_ids(root_ids, leading_zero)
        net = self._native(model)
        cnt = n.shape[0]
        pol = np.zeros((cnt, self.A), np.float32)
        val = np.zeros(cnt, np.float32)
        status = np.zeros(cnt, np.int32)
        err = np.zeros(cnt, np.int32)
        if symmetries == 1:
            self._check(self._L.ao_positions_evaluate(
                self._handle(), net._h, _ptr(moves, C.c_int32), moves.shape[1], _ptr(n, C.c_int32), cnt,
                _ptr(pol, C.c_float), _ptr(val, C.c_float), _ptr(status, C.c_int32), _ptr(err, C.c_int32)),
                "ao_positions_evaluate")
        else:
            self._check(self._L.ao_positions_evaluate_sym(
                self._handle(), net._h, _ptr(moves, C.c_int32), moves.shape[1], _ptr(n, C.c_int32), cnt, int(symmetries),
                _ptr(pol, C.c_float), _ptr(val, C.c_float), _ptr(status, C.c_int32), _ptr(err, C.c_int32)),
                "ao_positions_evaluate_sym")
        return pol, val, status, err

    # -- tactics: defined through utils.check_win alone (utils.win_cells / utils.audit_moves are the host definition)
    def _ask(self, fn, root_ids, leading_zero, outputs, *limits):
        """The id-batch entry point `fn` with every output: `outputs` lists them as (name, shape of one row, dtype) in the
        order of the C ABI, `limits` go between the ids and the outputs -> dict of the arrays, one row per id."""
        moves, n = pack_ids(root_ids, leading_zero)
        cnt = n.shape[0]
        out = {name: np.zeros((cnt,) + shape, dtype) for name, shape, dtype in outputs}
        self._check(getattr(self._L, fn)(
            self._handle(), _ptr(moves, C.c_int32), moves.shape[1], _ptr(n, C.c_int32), cnt, *limits,
            *(_ptr(a, _CTYPE[a.dtype.type]) for a in out.values())), fn)
        return out

    def win_cells(self, root_ids, leading_zero=True):
        """The cells that win at once, one row per id: dict of mine (uint8 [n, A], 1 where a stone of the side to move
        completes a line: check_win of the board with that stone is the mover's index), theirs (the same for the
        opponent, as if it were to move: the cells the mover must occupy), status (check_win of the position; a terminal
        position has no winning cells), turn, err (as describe; rows with err != 0 are all zero)."""
        A = self.A
        return self._ask("ao_positions_win_cells", root_ids, leading_zero, (
            ("mine", (A,), np.uint8), ("theirs", (A,), np.uint8), ("status", (), np.int32), ("turn", (), np.int32),
            ("err", (), np.int32)))

    def audit(self, root_ids, leading_zero=True):
        """The tactical audit of game records, one row per id: dict of flags (uint8 [n, A]: the flag byte of ply t at
        [i, t] -- WIN_AVAILABLE, WIN_TAKEN, THREAT, BLOCKED, LOST, set while the position before the move is not terminal;
        zeros from the first terminal position on and beyond the record), counts (int32 [n, 8]: plies audited,
        WIN_AVAILABLE, wins missed, single threats, blocks missed, LOST, end_ply and status as describe), err (as
        describe; rows with err != 0 are all zero)."""
        return self._ask("ao_positions_audit", root_ids, leading_zero, (
            ("flags", (self.A,), np.uint8), ("counts", (8,), np.int32), ("err", (), np.int32)))

    def forced_wins(self, root_ids, max_depth=8, max_nodes=2000, leading_zero=True):
        """Forced wins by continuous fours (VCF) for the side to move, one row per id; utils.forced_win is the definition.
        dict of result (FW_NONE no forced win within max_depth attacker moves, FW_WIN, FW_UNKNOWN the budget of max_nodes
        search nodes ran out: everything else of the search is then as for FW_NONE), depth (the fewest attacker moves,
        0 unless FW_WIN), move (the lowest winning first move, -1 if none), moves (uint8 [n, A]: every first move that
        wins within depth), line (int16 [n, 2 max_depth - 1]: the principal line, padded with -1), line_len, nodes, and
        status, turn, err as win_cells (a terminal position has result 0; rows with err != 0 are all zero, move and line
        -1). 1 <= max_depth <= 16, 1 <= max_nodes <= 65536, ValueError otherwise: the node budget bounds the launch."""
        _check_limits(max_depth, max_nodes)
        i32 = ((), np.int32)
        return self._ask("ao_positions_forced_wins", root_ids, leading_zero, (
            ("result",) + i32, ("depth",) + i32, ("move",) + i32, ("moves", (self.A,), np.uint8),
            ("line", (2 * int(max_depth) - 1,), np.int16), ("line_len",) + i32, ("nodes",) + i32, ("status",) + i32,
            ("turn",) + i32, ("err",) + i32), int(max_depth), int(max_nodes))

    def forced_defences(self, root_ids, max_depth=8, max_nodes=2000, leading_zero=True):
        """Which replies of the side to move hold against the opponent's forced win by continuous fours, one row per id;
        utils.forced_defences is the definition: forced_wins of the position after every empty cell, and of the position
        itself with the opponent attacking as if the mover had passed -- A + 1 searches per id, each with its own budget
        of max_nodes, one wavefront each. dict of threat, threat_depth, threat_moves (uint8 [n, A]): result, depth and
        moves of the opponent's search after a pass; reply (uint8 [n, A]: FD_NONE not an empty cell, FD_SAFE the opponent
        has no forced win after a stone there -- also a stone that ends the game --, FD_LOSES it has one, FD_UNKNOWN that
        search ran out of nodes); depth (uint8 [n, A]: the opponent's attacker moves after the reply, 0 unless LOSES);
        counts (int32 [n, 4]: empty cells, SAFE, LOSES, UNKNOWN); nodes (the sum over the searches run); status, turn, err
        as win_cells. A terminal position has every output but status and turn zero, and so has a row with err != 0.
        Limits as forced_wins, ValueError otherwise."""
        _check_limits(max_depth, max_nodes)
        i32, u8 = ((), np.int32), ((self.A,), np.uint8)
        return self._ask("ao_positions_forced_defences", root_ids, leading_zero, (
            ("threat",) + i32, ("threat_depth",) + i32, ("threat_moves",) + u8, ("reply",) + u8, ("depth",) + u8,
            ("counts", (4,), np.int32), ("nodes",) + i32, ("status",) + i32, ("turn",) + i32, ("err",) + i32),
            int(max_depth), int(max_nodes))

    # -- lifetime
    def close(self):
        if getattr(self, "_h", None):
            self._L.ao_positions_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
