"""Python handles over the C ABI: `Engine` (G concurrent games) and `Net` (PVNet weights).

Thin by design: argument marshalling and error propagation only. Tensors are exchanged as raw
device pointers (torch.Tensor.data_ptr()); no torch types cross the boundary.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import AO_ROOT_EXPANDED, AO_ROOT_FRESH, AO_ROOT_UNEXPANDED  # noqa: F401
from ._lib import AO_NODE_ABSENT, AO_NODE_EXPANDED, AO_NODE_LEAF, AO_NODE_TERMINAL  # noqa: F401


class EngineError(RuntimeError):
    pass


# Engine.search(early_stop=...): simulations between two looks at whether the moves are decided
SETTLE_EVERY = 16

# q of a root child that is barred from the current move (begin_move / search with allowed= or tactics=): AO_BAR_Q of
# include/omok_hip.h, the float32 nearest to -1e30. Such a child has n == 0 and w == 0; Engine.root_children shows it.
BAR_Q = float(np.float32(-1.0e30))
RT_NONE, RT_WIN, RT_DEFEND, RT_LOST = 0, 1, 2, 3      # `verdict` of Engine.root_tactics / utils.root_tactics
# Engine.tree_proofs' status of a node for its side to move, and the verdicts of Engine.set_proof_moves (utils.proof_pi)
from .utils import PROOF_UNKNOWN, PROOF_WIN, PROOF_LOSS, PROOF_DRAW, PM_NONE, PM_WIN, PM_PRUNED, PM_MOVED  # noqa: E402,F401


def _ptr(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype)) if a is not None else None


def plan_kernel(n_block, inplanes, planes, board_size, boards, in_kind=2, trunk_mode=0):
    """(kernel name as rocprofv3 prints it + description, algorithmic FLOPs per launch) of the kernel that would
    carry the conv stack for `boards` positions -- planning logic only, needs no GPU (ao_net_plan_kernel).
    in_kind 2: the engine's bit planes (what ao_search feeds), 1: the fp32 plane batch (ao_net_forward)."""
    L = _lib.load()
    buf = C.create_string_buffer(256)
    f = C.c_double(0)
    if L.ao_net_plan_kernel(int(n_block), int(inplanes), int(planes), int(board_size), int(trunk_mode), int(boards),
                            int(in_kind), buf, 256, C.byref(f)):
        raise EngineError("ao_net_plan_kernel: bad network shape")
    return buf.value.decode(), f.value


def guard_check():
    """(guarded device blocks alive, damaged blocks, message) -- ao_guard_check. Blocks are guarded when their handle was created
    under AO_POOL_GUARD=<bytes> (with AO_POOL_FILL=<0..255> written to the guards and the body); a damaged block has a guard byte
    that is no longer the fill: something wrote outside the block. Waits for the devices that have guarded blocks. Blocks whose
    damage was found when they were freed are counted too; every damaged block is reported once. The message has one line
    per block (the first few), as include/omok_hip.h words it."""
    L = _lib.load()
    blocks, damaged = C.c_int32(0), C.c_int32(0)
    buf = C.create_string_buffer(4096)
    if L.ao_guard_check(C.byref(blocks), C.byref(damaged), buf, 4096):
        raise EngineError("ao_guard_check: " + buf.value.decode())
    return blocks.value, damaged.value, buf.value.decode()


def guard_block(index):
    """(device pointer of the body, bytes, guard bytes) of the index-th live guarded block in allocation order, or None past
    the end (ao_guard_block)."""
    L = _lib.load()
    p, n, g = C.c_void_p(), C.c_int64(0), C.c_int64(0)
    if L.ao_guard_block(int(index), C.byref(p), C.byref(n), C.byref(g)):
        return None
    return p.value or 0, n.value, g.value


def guard_mode():
    """(guard bytes an allocation made now would get: AO_POOL_GUARD rounded up to 4096, 0 = off; the fill byte) -- ao_guard_mode."""
    L = _lib.load()
    g, f = C.c_int64(0), C.c_int32(0)
    L.ao_guard_mode(C.byref(g), C.byref(f))
    return g.value, f.value


class Net:
    """model.PVNet(n_block, inplanes, planes, board_size) in eval() mode, on the MI355X."""

    def __init__(self, n_block, inplanes, planes, board_size, device=0):
        self._L = _lib.load()
        h = C.c_void_p()
        if self._L.ao_net_create(n_block, inplanes, planes, board_size, device, C.byref(h)):
            raise EngineError("ao_net_create: " + self._L.ao_net_last_error(None).decode())
        self._h = h
        self.n_block, self.inplanes, self.planes, self.board_size = n_block, inplanes, planes, board_size
        self.device = device
        self.A = board_size * board_size

    def _check(self, rc, what):
        if rc:
            raise EngineError("%s: %s" % (what, self._L.ao_net_last_error(self._h).decode()))

    def load_state_dict(self, state_dict):
        """state_dict: name -> array-like (numpy or torch tensor), reference key names. Device tensors come over in
        ONE flattened copy (a per-tensor .cpu() costs ~60 synchronous transfers per export)."""
        items = list(state_dict.items())
        dev = [(k, v) for k, v in items if hasattr(v, "is_cuda") and v.is_cuda]
        host = {}
        if dev:
            import torch
            flat = torch.cat([v.detach().reshape(-1).to(torch.float32) for _, v in dev]).cpu().numpy()
            off = 0
            for k, v in dev:
                n = v.numel()
                host[k] = flat[off:off + n]
                off += n
        for name, val in items:
            if name in host:
                arr = host[name]
            else:
                if hasattr(val, "detach"):
                    val = val.detach().cpu().numpy()
                arr = np.ascontiguousarray(np.asarray(val), dtype=np.float32).reshape(-1)
            arr = np.ascontiguousarray(arr, dtype=np.float32)
            self._check(self._L.ao_net_set_param(self._h, name.encode(), _ptr(arr, C.c_float), arr.size),
                        "ao_net_set_param(%s)" % name)
        self._check(self._L.ao_net_finalize(self._h), "ao_net_finalize")
        return self

    def forward_ptr(self, planes_ptr, batch, policy_ptr, value_ptr, stream=None):
        self._check(self._L.ao_net_forward(self._h, planes_ptr, batch, policy_ptr, value_ptr, stream),
                    "ao_net_forward")

    def __call__(self, x):
        """x: torch.cuda float32 [batch, C, B, B] -> (policy [batch, A], value [batch]) tensors."""
        import torch
        x = x.contiguous().float()
        batch = x.shape[0]
        pol = torch.empty((batch, self.A), dtype=torch.float32, device=x.device)
        val = torch.empty((batch,), dtype=torch.float32, device=x.device)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        self.forward_ptr(x.data_ptr(), batch, pol.data_ptr(), val.data_ptr(), stream)
        return pol, val

    def set_mode(self, mode):
        """0 auto, 1 layer kernels (32-board groups), 2 group-resident trunk, 3 per-board, 4 row-chunked layers,
        5 group-resident trunk on split-fp16 MFMAs (fp32-accurate; 128 planes, board <= 9x9), 6 the per-layer split-fp16
        kernels for every batch size (a position's evaluation then does not depend on what else is in the batch)."""
        self._check(self._L.ao_net_set_mode(self._h, int(mode)), "ao_net_set_mode")

    def get_mode(self):
        """The mode in force: what set_mode asked for, or 2 while the fp16-range fallback holds the network on the
        fp32-MFMA trunk (three repeated moves with the same weights; ends with the next load_state_dict / set_mode)."""
        return int(self._L.ao_net_get_mode(self._h))

    def status(self, clear=True, stream=None):
        """Status word (ao_net_status): bit 0 = an activation left the fp16 range in the split-fp16 trunk since
        the last clear (those forwards were clamped, not fp32-equivalent). Synchronises `stream`."""
        f = C.c_int32(0)
        self._check(self._L.ao_net_status(self._h, stream, C.byref(f), 1 if clear else 0), "ao_net_status")
        return f.value

    def products(self, request=-1):
        """(MFMA products per multiply-add in force: 2 or 3, True when the loaded conv weights are fp16 numbers) -- ao_net_products.
        request 0: two products whenever the weights allow (default), 3: always three, -1: query only."""
        a, b = C.c_int32(0), C.c_int32(0)
        self._check(self._L.ao_net_products(self._h, int(request), C.byref(a), C.byref(b)), "ao_net_products")
        return a.value, bool(b.value)

    PRECISIONS = ("fp32", "fp16", "fp16-all")       # AO_NET_PRECISION_FP32 / AO_NET_PRECISION_FP16 / AO_NET_PRECISION_FP16_ALL

    def precision(self, request=None):
        """"fp32" (the default: every forward fp32-equivalent), "fp16" (the opt-in plain-fp16 forward: one MFMA product per
        multiply-add, activations rounded once to fp16, on the batches planned onto the resident / board-resident trunk; every
        other batch keeps its fp32-equivalent kernel) or "fp16-all" (that arithmetic for EVERY forward of this net: the other
        batches of modes 0 / 5 / 6 run the one-product per-layer kernel k_layer16h_f16; in mode 6 one arithmetic for every batch
        size) -- ao_net_precision. request: None = query, or one of PRECISIONS. Belongs to this Net and survives load_state_dict;
        "fp16" / "fp16-all" on a network the split-fp16 kernels do not cover raises EngineError and changes nothing."""
        if request is not None and request not in self.PRECISIONS:
            raise ValueError("precision must be 'fp32', 'fp16' or 'fp16-all', not %r" % (request,))
        a, b = C.c_int32(0), C.c_int32(0)
        req = -1 if request is None else self.PRECISIONS.index(request)
        self._check(self._L.ao_net_precision(self._h, req, C.byref(a), C.byref(b)), "ao_net_precision")
        return self.PRECISIONS[a.value]

    def dominant_kernel(self, boards):
        """(name, algorithmic FLOPs per launch) of the kernel conv_timing() measures."""
        buf = C.create_string_buffer(256)
        f = C.c_double(0)
        self._check(self._L.ao_net_dominant_kernel(self._h, int(boards), buf, 256, C.byref(f)),
                    "ao_net_dominant_kernel")
        return buf.value.decode(), f.value

    def conv_timing(self, enable=True):
        """Returns (total ms, launches) of the TIMED trunk conv launches since the last call; enable = n > 1 times every
        n-th forward only (an event pair per launch costs ~1 % of a 1.5 ms step)."""
        ms, cnt = C.c_double(0), C.c_int64(0)
        self._check(self._L.ao_net_conv_timing(self._h, int(enable), C.byref(ms), C.byref(cnt)),
                    "ao_net_conv_timing")
        return ms.value, cnt.value

    def close(self):
        if getattr(self, "_h", None):
            self._L.ao_net_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine:
    """G concurrent games: SoA search trees in HBM + the tree kernels (see include/omok_hip.h)."""

    def __init__(self, board_size, num_mcts, inplanes=5, games=1, noise=True, device=0, node_cap=0,
                 c_puct=0.0, alpha=0.0, win_mark=0, arena_fraction=0.0):
        self._L = _lib.load()
        cfg = _lib.AoConfig(board=board_size, win_mark=win_mark, sims=num_mcts, inplanes=inplanes,
                            games=games, noise=1 if noise else 0, node_cap=node_cap, device=device,
                            c_puct=c_puct, alpha=alpha, arena_fraction=arena_fraction)
        h = C.c_void_p()
        if self._L.ao_create(C.byref(cfg), C.byref(h)):
            raise EngineError("ao_create: " + self._L.ao_last_error(None).decode())
        self._h = h
        self.board_size, self.num_mcts, self.inplanes, self.G = board_size, num_mcts, inplanes, games
        self.A = board_size * board_size
        self.device = device
        self._fp16_seen = self._fp16_games_seen = 0

    def _check(self, rc, what):
        if rc:
            msg = self._L.ao_last_error(self._h).decode()
            if "the root bar allows no empty cell" in msg:      # an argument error of allowed=, found on the host before any device call
                raise ValueError("%s: %s" % (what, msg))
            raise EngineError("%s: %s" % (what, msg))

    # -- rng
    def seed(self, game, seed):
        self._check(self._L.ao_seed(self._h, game, seed & 0xFFFFFFFF), "ao_seed")

    def seed_all(self, seeds):
        s = np.ascontiguousarray(seeds, np.uint32)
        assert s.size == self.G
        self._check(self._L.ao_seed_all(self._h, _ptr(s, C.c_uint32)), "ao_seed_all")

    def seed_games(self, games, seeds):
        """seed() for the listed games with one synchronisation (ao_seed_games)."""
        g = np.ascontiguousarray(games, np.int32)
        s = np.ascontiguousarray(np.asarray(seeds, np.uint64) & 0xFFFFFFFF, np.uint32)
        assert g.size == s.size
        if g.size:
            self._check(self._L.ao_seed_games(self._h, _ptr(g, C.c_int32), _ptr(s, C.c_uint32), int(g.size)), "ao_seed_games")

    def set_leaf_symmetry(self, base_key=None, keys=None, games=None):
        """Leaf symmetries (ao_set_leaf_symmetry): with a base key (an int) every leaf is evaluated under the symmetry
        utils.leaf_symmetry(key_g, stones on the leaf, simulation index) -- planes in, policy back --, where key_g =
        utils.leaf_key(base_key, seed of game g) follows the seed calls (a game never seeded: g). None switches it off: every
        result is then what it is on an engine that never had it. keys (with games, default all) sets the keys of single games
        directly afterwards (ao_set_leaf_symmetry_keys; needs a base key in this or an earlier call). Refused inside a move.
        Tree snapshots do not carry the keys, and set_eval_log records rows in the network's frame."""
        if base_key is not None or keys is None:
            on = base_key is not None
            self._check(self._L.ao_set_leaf_symmetry(self._h, 1 if on else 0, (int(base_key) & 0xFFFFFFFF) if on else 0),
                        "ao_set_leaf_symmetry")
        if keys is not None:
            k = np.ascontiguousarray(np.asarray(keys, np.uint64) & 0xFFFFFFFF, np.uint32).reshape(-1)
            g = np.arange(self.G, dtype=np.int32) if games is None else np.ascontiguousarray(games, np.int32).reshape(-1)
            if g.size != k.size:
                raise ValueError("set_leaf_symmetry: %d keys for %d games" % (k.size, g.size))
            if g.size:
                self._check(self._L.ao_set_leaf_symmetry_keys(self._h, _ptr(g, C.c_int32), _ptr(k, C.c_uint32), int(g.size)),
                            "ao_set_leaf_symmetry_keys")

    def set_leaf_tactics(self, max_depth=2, max_nodes=16):
        """Leaf tactics (ao_set_leaf_tactics): the forced-win solver runs on every leaf the search expands, and where it proves
        a win for the side to move there the leaf's value is exactly +1 instead of the network's -- utils.leaf_tactics_value;
        the search is the reference search under utils.leaf_tactics_evaluator, bit for bit. max_depth None / False / 0: off,
        and every result is what it is on an engine that never had it. max_depth 1..16, max_nodes 1..1024 per leaf. The default
        was a guess, 4 / 64, and is 2 / 16 after one table: a launch lasts as long as its longest search, so
        the cost follows max_nodes, and 2 / 16 proved 95 - 99 % of the leaves that 4 / 64 proved for a fifth to a half of the time
        added per simulation; whether the deeper proofs are worth more in play has not been measured. Refused inside a move and
        for an open roll with games in a move. Tree snapshots do not carry the switch; set_eval_log records the network's value."""
        if max_depth is None or max_depth is False:
            max_depth = 0
        if isinstance(max_depth, bool) or isinstance(max_nodes, bool):
            raise ValueError("set_leaf_tactics: max_depth / max_nodes must be integers")
        self._check(self._L.ao_set_leaf_tactics(self._h, int(max_depth), int(max_nodes)), "ao_set_leaf_tactics")

    def leaf_tactics_stats(self, per_game=False, reset=False):
        """dict(searched, proven, unknown, nodes): the leaves the solver searched, those it proved won, the searches that ran out
        of max_nodes and the solver's nodes, since the last reset (ao_leaf_tactics_stats); per_game=True adds `per_game`,
        int32 [G, 4] in that order. A move that search() repeated on the fp32-MFMA trunk (fp16_range_events) counts with BOTH
        attempts: the leaves of the discarded first one were searched, and nothing but reset=True clears the counters."""
        out = np.zeros(4, np.int64)
        pg = np.zeros((self.G, 4), np.int32) if per_game else None
        self._check(self._L.ao_leaf_tactics_stats(self._h, _ptr(out, C.c_int64), _ptr(pg, C.c_int32), 1 if reset else 0),
                    "ao_leaf_tactics_stats")
        d = dict(searched=int(out[0]), proven=int(out[1]), unknown=int(out[2]), nodes=int(out[3]))
        if per_game:
            d["per_game"] = pg
        return d

    def get_rng_state(self, game):
        mt = np.zeros(624, np.uint32)
        pos, hg, gs = C.c_int32(0), C.c_int32(0), C.c_double(0)
        self._check(self._L.ao_get_rng_state(self._h, game, _ptr(mt, C.c_uint32), C.byref(pos), C.byref(hg),
                                             C.byref(gs)), "ao_get_rng_state")
        return mt, pos.value, hg.value, gs.value

    def set_rng_state(self, game, mt, pos, has_gauss=0, gauss=0.0):
        mt = np.ascontiguousarray(mt, np.uint32)
        self._check(self._L.ao_set_rng_state(self._h, game, _ptr(mt, C.c_uint32), int(pos), int(has_gauss),
                                             float(gauss)), "ao_set_rng_state")

    # -- state
    def reset(self, mask=None):
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self._check(self._L.ao_reset(self._h, _ptr(m, C.c_uint8)), "ao_reset")

    def set_root(self, game, moves):
        mv = np.ascontiguousarray(list(moves), np.int32)
        st = C.c_int32(0)
        self._check(self._L.ao_set_root(self._h, game, _ptr(mv, C.c_int32), mv.size, C.byref(st)), "ao_set_root")
        return st.value

    def set_roots(self, ids, mask=None):
        """ids: one reference-style root id (0, a1, a2, ...) per game; mask selects the games that move. One
        launch for all of them. Returns the AO_ROOT_* status per game (int32 [G], -2 where unmasked)."""
        mv = np.zeros((self.G, self.A), np.int32)
        n = np.zeros(self.G, np.int32)
        for g, rid in enumerate(ids):
            if mask is not None and not mask[g]:
                continue
            m = list(rid)[1:]
            n[g] = len(m)
            mv[g, :len(m)] = m
        st = np.full(self.G, -2, np.int32)
        mk = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self._check(self._L.ao_set_roots(self._h, _ptr(mk, C.c_uint8), _ptr(mv, C.c_int32), self.A, _ptr(n, C.c_int32),
                                         _ptr(st, C.c_int32)), "ao_set_roots")
        return st

    def get_moves(self, game):
        mv = np.zeros(self.A + 1, np.int32)
        n = C.c_int32(0)
        self._check(self._L.ao_get_moves(self._h, game, _ptr(mv, C.c_int32), C.byref(n)), "ao_get_moves")
        return mv[:n.value].tolist()

    # -- stepwise move
    def set_stream(self, stream_ptr):
        self._check(self._L.ao_set_stream(self._h, stream_ptr), "ao_set_stream")

    def sync(self):
        self._check(self._L.ao_sync(self._h), "ao_sync")

    def _per_game(self, v, dtype):
        return None if v is None else np.ascontiguousarray(np.broadcast_to(v, (self.G,)), dtype)

    def set_root_bar(self, allowed):
        """The root move restriction of the NEXT begin_move / search (ao_set_root_bar): allowed uint8 / bool [G, A], 1 = the
        cell may be searched at that game's root; None clears it. What begin_move(allowed=) and search(allowed=) call."""
        from .utils import check_allowed
        m = check_allowed(allowed, self.G, self.A)
        self._check(self._L.ao_set_root_bar(self._h, _ptr(m, C.c_uint8)), "ao_set_root_bar")

    def root_tactics(self, active=None, max_depth=6, max_nodes=512, apply=False):
        """utils.root_tactics of every active game's root position, solved on the device from the engine's own positions
        (ao_root_tactics). Returns dict(verdict int32 [G]: RT_NONE / RT_WIN / RT_DEFEND / RT_LOST, depth int32 [G], allowed
        bool [G, A], nodes int32 [G], unknown int32 [G]); inactive, ended and terminal games get zeros. apply=True: the bar
        of the next begin_move / search is set on the device from `allowed` (intersected with a pending set_root_bar; a
        game whose intersection is empty keeps the caller's), with no host round trip of the mask. ValueError for limits
        outside 1..16 / 1..65536."""
        from .positions import _check_limits
        _check_limits(max_depth, max_nodes)
        a = None if active is None else np.ascontiguousarray(active, np.uint8)
        G = self.G
        v, d, n, u = (np.zeros(G, np.int32) for _ in range(4))
        al = np.zeros((G, self.A), np.uint8)
        self._check(self._L.ao_root_tactics(self._h, _ptr(a, C.c_uint8), int(max_depth), int(max_nodes), 1 if apply else 0,
                                            _ptr(v, C.c_int32), _ptr(d, C.c_int32), _ptr(al, C.c_uint8), _ptr(n, C.c_int32),
                                            _ptr(u, C.c_int32)), "ao_root_tactics")
        return dict(verdict=v, depth=d, allowed=al.astype(bool), nodes=n, unknown=u)

    def last_tactics(self):
        """What root_tactics said in the last search(tactics=...) of this engine, or None."""
        return getattr(self, "_last_tactics", None)

    def _tactics(self, tactics, active, sims):
        """search(tactics=): root_tactics(apply=True) for the active games; returns the per-game budgets with solved_sims
        applied to the games with a proven win."""
        opt = {} if tactics is True else dict(tactics)
        unknown = set(opt) - {"max_depth", "max_nodes", "solved_sims"}
        if unknown:
            raise ValueError("tactics: unknown key(s) %s" % sorted(unknown))
        k = opt.pop("solved_sims", None)
        if k is not None and (isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= self.num_mcts):
            raise ValueError("tactics: solved_sims must be an integer in 1..%d, got %r" % (self.num_mcts, k))
        rt = self.root_tactics(active, apply=True, **opt)
        self._last_tactics = rt
        if k is not None and (rt["verdict"] == RT_WIN).any():
            s = np.array(np.broadcast_to(self.num_mcts if sims is None else sims, (self.G,)), np.int32)
            won = rt["verdict"] == RT_WIN
            s[won] = np.minimum(s[won], int(k))
            return s
        return sims

    def begin_move(self, active=None, sims=None, noise=None, allowed=None):
        """sims: simulations per game for this move (int or [G], 1..num_mcts), noise: per-game noise switch (bool or [G]; False
        = this game searches this move as on a noise=False engine, stream untouched). None: the engine's configuration.
        allowed: uint8 / bool [G, A], the cells that may be searched at each game's root in this move (set_root_bar); a
        barred root child gets no visit and reads q == BAR_Q in root_children. ValueError for a row of an active game that
        allows none of its empty cells; None: no restriction."""
        a = None if active is None else np.ascontiguousarray(active, np.uint8)
        if allowed is not None:
            self.set_root_bar(allowed)
        if sims is None and noise is None:
            self._check(self._L.ao_begin_move(self._h, _ptr(a, C.c_uint8)), "ao_begin_move")
            return
        s, n = self._per_game(sims, np.int32), self._per_game(noise, np.uint8)
        self._check(self._L.ao_begin_move_opts(self._h, _ptr(a, C.c_uint8), _ptr(s, C.c_int32), _ptr(n, C.c_uint8)),
                    "ao_begin_move_opts")

    def sims_left(self):
        return self._L.ao_sims_left(self._h)

    def settle(self, mask=None, stop=False):
        """Inside a move: lower the target of every masked game (None: all) whose move is decided (utils.move_decided) -- or of
        every masked game, with stop=True -- to what it has run, a pending leaf included (ao_settle). Returns the number of
        games that still owe simulations; sims_left() then tells how many launches that takes."""
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        left = C.c_int32(0)
        self._check(self._L.ao_settle(self._h, _ptr(m, C.c_uint8), 1 if stop else 0, C.byref(left)), "ao_settle")
        return left.value

    def sims_run(self):
        """The last move: dict(sims int32 [G] simulations run per game in budget units, settled bool [G], settled_total and
        saved_total: games settled / simulations saved since the engine was created) -- ao_search_sims."""
        s, f = np.zeros(self.G, np.int32), np.zeros(self.G, np.uint8)
        a, b = C.c_int64(0), C.c_int64(0)
        self._check(self._L.ao_search_sims(self._h, _ptr(s, C.c_int32), _ptr(f, C.c_uint8), C.byref(a), C.byref(b)),
                    "ao_search_sims")
        return dict(sims=s, settled=f.astype(bool), settled_total=a.value, saved_total=b.value)

    def collect_leaves(self, planes_ptr=None):
        self._check(self._L.ao_collect_leaves(self._h, planes_ptr), "ao_collect_leaves")

    def apply_evals(self, policy_ptr, value_ptr):
        self._check(self._L.ao_apply_evals(self._h, policy_ptr, value_ptr), "ao_apply_evals")

    def _outs(self):
        return tuple(np.zeros((self.G, self.A), np.float64) for _ in range(3))

    def end_move(self, tau=None):
        """Returns (pi, visit, policy), float64 [G, A] each."""
        t = None if tau is None else np.ascontiguousarray(np.broadcast_to(tau, (self.G,)), np.int8)
        pi, vis, pol = self._outs()
        self._check(self._L.ao_end_move(self._h, _ptr(t, C.c_int8), _ptr(pi, C.c_double), _ptr(vis, C.c_double),
                                        _ptr(pol, C.c_double)), "ao_end_move")
        return pi, vis, pol

    def play(self):
        """utils.get_action + env.step + re-root. Returns (action[G], win_index[G])."""
        act = np.zeros(self.G, np.int32)
        win = np.zeros(self.G, np.int32)
        self._check(self._L.ao_play(self._h, _ptr(act, C.c_int32), _ptr(win, C.c_int32)), "ao_play")
        return act, win

    # -- fused move with the native network
    def search(self, net, tau=None, active=None, sims=None, noise=None, early_stop=None, settle_every=None, allowed=None,
               tactics=None):
        """sims / noise / allowed: as begin_move. early_stop: the games that may stop once their move is decided (utils.move_decided) --
        a bool [G] mask, or True for the games with tau == 0 (the only ones whose result is the leader alone); the loop looks
        every settle_every simulations (None: SETTLE_EVERY, 0: never). tactics: True or dict(max_depth, max_nodes,
        solved_sims) -- root_tactics(apply=True) runs first for the active games: a game with a proven forced win searches
        only its winning first moves (with solved_sims=k: at most k simulations), a game facing one only the replies not
        proven to lose; intersected with `allowed`, and read afterwards with last_tactics(). With none of them given this
        is ao_search."""
        t = None if tau is None else np.ascontiguousarray(np.broadcast_to(tau, (self.G,)), np.int8)
        a = None if active is None else np.ascontiguousarray(active, np.uint8)
        if allowed is not None:
            self.set_root_bar(allowed)
        self._last_tactics = None
        if tactics is not None and tactics is not False:
            sims = self._tactics(tactics, a, sims)
        pi, vis, pol = self._outs()
        if early_stop is True:
            early_stop = np.zeros(self.G, bool) if t is None else (t == 0)
        elif early_stop is False:
            early_stop = None
        if sims is None and noise is None and early_stop is None:
            self._check(self._L.ao_search(self._h, net._h, _ptr(a, C.c_uint8), _ptr(t, C.c_int8),
                                          _ptr(pi, C.c_double), _ptr(vis, C.c_double), _ptr(pol, C.c_double)),
                        "ao_search")
        else:
            s, n, m = self._per_game(sims, np.int32), self._per_game(noise, np.uint8), self._per_game(early_stop, np.uint8)
            k = SETTLE_EVERY if settle_every is None else int(settle_every)
            self._check(self._L.ao_search_opts(self._h, net._h, _ptr(a, C.c_uint8), _ptr(t, C.c_int8), _ptr(s, C.c_int32),
                                               _ptr(n, C.c_uint8), _ptr(m, C.c_uint8), k, _ptr(pi, C.c_double),
                                               _ptr(vis, C.c_double), _ptr(pol, C.c_double)), "ao_search_opts")
        ev, games = self.fp16_range_events()
        if ev != self._fp16_seen:
            import warnings
            warnings.warn("the split-fp16 trunk met an activation beyond the fp16 range (|x| > 65504): this move was searched "
                          "again on the fp32-MFMA trunk with fresh trees for its %d games (%d such move(s) of this engine so far). "
                          "From the third such move of the SAME weights on, the network stays on the fp32-MFMA trunk -- also "
                          "when mode 6 (reproducible=True) had been asked for -- until new weights are loaded or set_mode is "
                          "called; Net.get_mode() tells which kernels run" % (games - self._fp16_games_seen, ev),
                          RuntimeWarning, stacklevel=2)
            self._fp16_seen, self._fp16_games_seen = ev, games
        return pi, vis, pol

    # -- rolling search: every game moves on its own clock inside one launch loop (ao_roll_*)
    def _by_ply(self, v, dtype):
        """None, a scalar, [G] or [G, P] -> a contiguous [G, P] table by ply (the last column holds for every later ply)."""
        if v is None:
            return None
        a = np.asarray(v)
        if a.ndim == 2 and a.shape[0] == self.G and a.shape[1] >= 1:
            return np.ascontiguousarray(a, dtype)
        if a.ndim > 1:
            raise ValueError("expected a scalar, [G] or [G, P], got shape %r" % (a.shape,))
        return np.ascontiguousarray(np.broadcast_to(a, (self.G,)).reshape(self.G, 1), dtype)

    def _roll_opts(self, active, tau_plies, sims, noise, early_stop=False, turn_every=None, visit=False, policy=False):
        keep = (None if active is None else np.ascontiguousarray(active, np.uint8), self._per_game(tau_plies, np.int32),
                self._by_ply(sims, np.int32), self._by_ply(noise, np.uint8))
        a, t, s, n = keep
        o = _lib.AoRollOpts(active=_ptr(a, C.c_uint8), tau_plies=_ptr(t, C.c_int32), sims=_ptr(s, C.c_int32),
                            sims_stride=0 if s is None else s.shape[1], noise=_ptr(n, C.c_uint8),
                            noise_stride=0 if n is None else n.shape[1], early_stop=1 if early_stop else 0,
                            turn_every=SETTLE_EVERY if turn_every is None else int(turn_every),
                            want_visit=1 if visit else 0, want_policy=1 if policy else 0)
        return o, keep                                   # (the struct holds pointers into `keep`: the caller keeps it until the call returns)

    def _roll_tactics(self, tactics):
        """roll_begin(tactics=): validated like search(tactics=) (+ allowed=True: the records carry the allowed rows); arms or
        disarms the solver for the roll that is about to open (ao_roll_set_tactics). Returns (armed, allowed rows asked for)."""
        from .positions import _check_limits
        if tactics is None or tactics is False:
            if getattr(self, "_roll_armed", False):
                self._check(self._L.ao_roll_set_tactics(self._h, 0, 0, 0, 0), "ao_roll_set_tactics")
                self._roll_armed = False
            return False, False
        opt = {} if tactics is True else dict(tactics)
        unknown = set(opt) - {"max_depth", "max_nodes", "solved_sims", "allowed"}
        if unknown:
            raise ValueError("tactics: unknown key(s) %s" % sorted(unknown))
        k = opt.get("solved_sims")
        if k is not None and (isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= self.num_mcts):
            raise ValueError("tactics: solved_sims must be an integer in 1..%d, got %r" % (self.num_mcts, k))
        depth, nodes = opt.get("max_depth", 6), opt.get("max_nodes", 512)
        _check_limits(depth, nodes)
        want = bool(opt.get("allowed", False))
        self._check(self._L.ao_roll_set_tactics(self._h, int(depth), int(nodes), 0 if k is None else int(k), 1 if want else 0),
                    "ao_roll_set_tactics")
        self._roll_armed = True
        return True, want

    def roll_begin(self, net, active=None, tau_plies=None, sims=None, noise=None, early_stop=False, turn_every=None,
                   visit=False, policy=False, tactics=None):
        """Opens a rolling search on `net` (ao_roll_begin): the listed games (None: all that are not over) begin a move and
        from then on every game ends its move, plays and begins the next one on its own clock, turn_every launches apart
        (None: SETTLE_EVERY), while the others go on searching. tau_plies: int or [G], tau is 1 while fewer moves than that
        are on the board (None: always); sims / noise: budgets and noise switches by ply, a scalar, [G] or [G, P] (a ply
        beyond P reads the last column); early_stop: tau == 0 moves stop once decided; visit / policy: roll_run returns
        them. tactics: True or dict(max_depth, max_nodes, solved_sims, allowed) -- every move of the roll is begun as
        search(tactics=dict(max_depth, max_nodes, solved_sims)) begins it, the solver running beside the loop
        (ao_roll_set_tactics); roll_run's records then carry verdict, depth, nodes, unknown (and, with allowed=True, allowed).
        Until roll_end, begin_move / search / end_move / play / set_root(s) / export_trees ... raise EngineError."""
        tac = self._roll_tactics(tactics)
        o, keep = self._roll_opts(active, tau_plies, sims, noise, early_stop, turn_every, visit, policy)
        self._check(self._L.ao_roll_begin(self._h, net._h, C.byref(o)), "ao_roll_begin")
        self._roll_tac = tac
        self._roll_buf = self._roll_buffers(visit, policy)

    def _roll_buffers(self, visit=False, policy=False):
        G, A = self.G, self.A
        return dict({k: np.zeros(G, np.int32) for k in ("game", "ply", "action", "win", "tau", "sims", "settled")},
                    pi=np.zeros((G, A)), visit=np.zeros((G, A)) if visit else None, policy=np.zeros((G, A)) if policy else None)

    def roll_run(self, max_launches=0):
        """Runs the loop until a turn has produced a record, nothing is in a move, or max_launches launches are spent (0: no
        bound) -- ao_roll_run. Returns a dict of arrays cut to the record count, one entry per game that ended a move: game,
        ply (moves on the board before it), action, win, tau, sims (simulations run, budget units), settled (bool), pi
        [n, A], and visit / policy [n, A] where roll_begin asked for them. With roll_begin(tactics=...) also what the solver said
        at the root of the move each record played: verdict, depth, nodes, unknown int32 [n] (and allowed bool [n, A] with
        tactics=dict(..., allowed=True)) -- ao_roll_tactics_records; without tactics the keys are the ones above. A game with
        win != 0 is over; every other one is already searching its next move, or waits for its verdict (unless draining)."""
        b = getattr(self, "_roll_buf", None) or self._roll_buffers()
        rec = _lib.AoRollRecords(count=0, pi=_ptr(b["pi"], C.c_double), visit=_ptr(b["visit"], C.c_double),
                                 policy=_ptr(b["policy"], C.c_double),
                                 **{k: _ptr(b[k], C.c_int32) for k in ("game", "ply", "action", "win", "tau", "sims", "settled")})
        self._check(self._L.ao_roll_run(self._h, int(max_launches), C.byref(rec)), "ao_roll_run")
        n = rec.count
        out = {k: b[k][:n].copy() for k in ("game", "ply", "action", "win", "tau", "sims", "pi")}
        out["settled"] = b["settled"][:n].astype(bool)
        for k in ("visit", "policy"):
            if b[k] is not None:
                out[k] = b[k][:n].copy()
        armed, want = getattr(self, "_roll_tac", (False, False))
        if armed:
            w = [np.zeros(max(n, 1), np.int32) for _ in range(4)]
            al = np.zeros((max(n, 1), self.A), np.uint8) if want else None
            self._check(self._L.ao_roll_tactics_records(self._h, *[_ptr(x, C.c_int32) for x in w], _ptr(al, C.c_uint8)),
                        "ao_roll_tactics_records")
            for k, x in zip(("verdict", "depth", "nodes", "unknown"), w):
                out[k] = x[:n]
            if want:
                out["allowed"] = al[:n].astype(bool)
        return out

    def roll_join(self, active=None, tau_plies=None, sims=None, noise=None):
        """Games that are not in a move (a slot refilled by reset + seed_games) begin one and join the running loop
        (ao_roll_join); tau_plies / sims / noise replace the listed games' rows, shapes as at roll_begin."""
        o, keep = self._roll_opts(active, tau_plies, sims, noise)
        self._check(self._L.ao_roll_join(self._h, C.byref(o)), "ao_roll_join")

    def roll_drain(self):
        """From now on no turned game begins another move; roll_run returns records until nothing is in a move."""
        self._check(self._L.ao_roll_drain(self._h), "ao_roll_drain")

    def roll_end(self):
        """Closes the roll (ao_roll_end); EngineError while any game is in a move. The engine is between moves afterwards."""
        self._check(self._L.ao_roll_end(self._h), "ao_roll_end")

    def roll_stats(self):
        """dict(turns, games_turned, bytes, last_games, last_bytes): host traffic of the turns (ao_roll_stats)."""
        v = [C.c_int64(0) for _ in range(5)]
        self._check(self._L.ao_roll_stats(self._h, *[C.byref(x) for x in v]), "ao_roll_stats")
        return dict(zip(("turns", "games_turned", "bytes", "last_games", "last_bytes"), (x.value for x in v)))

    def roll_tactics_stats(self):
        """dict(batches, games_solved, waited_turns, host_blocks, nodes, bytes) of the solver beside the open (or the last) roll
        (ao_roll_tactics_stats): waited_turns sums, over the games, the turns they spent waiting for a verdict; host_blocks
        counts the times the host had to wait for a batch; bytes are also part of roll_stats()["bytes"]."""
        v = (C.c_int64 * 6)()
        self._check(self._L.ao_roll_tactics_stats(self._h, v), "ao_roll_tactics_stats")
        return dict(zip(("batches", "games_solved", "waited_turns", "host_blocks", "nodes", "bytes"), (int(x) for x in v)))

    def fp16_range_events(self):
        """(moves ao_search repeated on the fp32-MFMA trunk, games searched again) since the engine was created."""
        a, b = C.c_int64(0), C.c_int64(0)
        self._check(self._L.ao_fp16_range_events(self._h, C.byref(a), C.byref(b)), "ao_fp16_range_events")
        return a.value, b.value

    def node_cap(self):
        """(expanded-node capacity of one game's arena, True if it was derived from the free HBM: node_cap=-1)."""
        a, b = C.c_int32(0), C.c_int32(0)
        self._check(self._L.ao_node_cap(self._h, C.byref(a), C.byref(b)), "ao_node_cap")
        return a.value, bool(b.value)

    # -- introspection
    def root_children(self, game):
        """The root's children in stored order: dict(action int32, n, w, q, p float64), empty while the root is not expanded.
        A child that is barred from the current move (begin_move / search with allowed= or tactics=) reads q == BAR_Q with
        n == 0 and w == 0 -- the sentinel is what keeps the selection off it; it stays until a later move of the same root
        allows the child again (then q == 0) or the root moves on."""
        A = self.A
        act = np.zeros(A, np.int32)
        n, w, q, p = (np.zeros(A) for _ in range(4))
        cnt = C.c_int32(0)
        self._check(self._L.ao_get_root_children(self._h, game, _ptr(act, C.c_int32), _ptr(n, C.c_double),
                                                 _ptr(w, C.c_double), _ptr(q, C.c_double), _ptr(p, C.c_double),
                                                 C.byref(cnt)), "ao_get_root_children")
        k = cnt.value
        return dict(action=act[:k].copy(), n=n[:k].copy(), w=w[:k].copy(), q=q[:k].copy(), p=p[:k].copy())

    def tree_nodes(self, game):
        a, b = C.c_int64(0), C.c_int64(0)
        self._check(self._L.ao_tree_nodes(self._h, game, C.byref(a), C.byref(b)), "ao_tree_nodes")
        return a.value, b.value

    # -- tree read-out on the device
    def tree_lookup(self, ids, games=None):
        """The reference's `self.tree[node_id]` for many ids in one call (ao_tree_lookup). ids: full reference ids
        (0, a1, a2, ...); games: the game each id is asked of (None: id i belongs to game i). Returns a dict of numpy arrays:
        status int32 [n] (AO_NODE_ABSENT / LEAF / TERMINAL / EXPANDED), the node's own n float64, w / q float32, p float64 [n]
        (NaN where the engine has no parent edge: see include/omok_hip.h), nchild int32 [n], and the children in stored order:
        child_action int32 [n, A] (-1 in unused slots), child_n int32, child_w / child_q float32, child_p float64 [n, A] (0 there)."""
        ids = [list(i)[1:] for i in ids]
        n, A = len(ids), self.A
        g = np.arange(n, dtype=np.int32) if games is None else np.ascontiguousarray(games, np.int32).reshape(-1)
        if g.size != n:
            raise ValueError("tree_lookup: one game per id")
        m = np.array([len(i) for i in ids], np.int32)
        stride = max(1, int(m.max()) if n else 1)
        mv = np.zeros((n, stride), np.int32)
        for k, i in enumerate(ids):
            mv[k, :len(i)] = i
        status, nchild = np.zeros(n, np.int32), np.zeros(n, np.int32)
        nwqp = np.full((n, 4), np.nan)
        ca, cn = np.full((n, A), -1, np.int32), np.zeros((n, A), np.int32)
        cw, cq, cp = np.zeros((n, A), np.float32), np.zeros((n, A), np.float32), np.zeros((n, A), np.float64)
        self._check(self._L.ao_tree_lookup(self._h, _ptr(g, C.c_int32), _ptr(mv, C.c_int32), stride, _ptr(m, C.c_int32), n,
                                           _ptr(status, C.c_int32), _ptr(nwqp, C.c_double), _ptr(nchild, C.c_int32),
                                           _ptr(ca, C.c_int32), _ptr(cn, C.c_int32), _ptr(cw, C.c_float), _ptr(cq, C.c_float),
                                           _ptr(cp, C.c_double)), "ao_tree_lookup")
        return dict(status=status, n=nwqp[:, 0].copy(), w=nwqp[:, 1].astype(np.float32), q=nwqp[:, 2].astype(np.float32),
                    p=nwqp[:, 3].copy(), nchild=nchild, child_action=ca, child_n=cn, child_w=cw, child_q=cq, child_p=cp)

    def principal_variations(self, max_len=None, mask=None):
        """The most-visited line from every masked game's root, first maximum in stored order (ao_tree_pv). Returns a dict:
        action int32 [G, max_len] (-1 beyond the line), n int32 and q float32 [G, max_len] (0 there), len int32 [G]."""
        L = self.A if max_len is None else int(max_len)
        mk = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        act = np.full((self.G, L), -1, np.int32)
        n, q, ln = np.zeros((self.G, L), np.int32), np.zeros((self.G, L), np.float32), np.zeros(self.G, np.int32)
        self._check(self._L.ao_tree_pv(self._h, _ptr(mk, C.c_uint8), L, _ptr(act, C.c_int32), _ptr(n, C.c_int32),
                                       _ptr(q, C.c_float), _ptr(ln, C.c_int32)), "ao_tree_pv")
        return dict(action=act, n=n, q=q, len=ln)

    def tree_stats(self, mask=None):
        """Per masked game (ao_tree_stats): expanded nodes the root reaches, dict entries, tree depth (del_parents' print,
        agents.py:241-250) and nodes_used (arena records in use, dead ones included). int32 [G] each, -1 for unmasked games."""
        mk = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        out = np.full((self.G, 4), -1, np.int32)
        self._check(self._L.ao_tree_stats(self._h, _ptr(mk, C.c_uint8), _ptr(out, C.c_int32)), "ao_tree_stats")
        return dict(expanded=out[:, 0].copy(), entries=out[:, 1].copy(), depth=out[:, 2].copy(), nodes_used=out[:, 3].copy())

    # -- proven outcomes
    def tree_proofs(self, mask=None, max_len=None):
        """What every masked game's tree PROVES, by exact minimax over it on the device (ao_tree_proofs; the definition is
        utils.tree_proofs). Read-only, as the other read-outs; fails inside a move and while a roll is open. Returns a dict:
        status, plies, proven, walked int32 [G] (the root's PROOF_* for its side to move, plies to the end, proven nodes, nodes
        walked; -1 for unmasked games), child_status int8 [G, A] (the root's edge by action, -1: no edge), child_plies int16
        [G, A], line int32 [G, max_len] (the proof line's actions, -1 beyond it; max_len None: A) and len int32 [G]."""
        L = self.A if max_len is None else int(max_len)
        mk = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        root = np.full((self.G, 4), -1, np.int32)
        cs, cp = np.full((self.G, self.A), -1, np.int8), np.zeros((self.G, self.A), np.int16)
        line, ln = np.full((self.G, L), -1, np.int32), np.zeros(self.G, np.int32)
        self._check(self._L.ao_tree_proofs(self._h, _ptr(mk, C.c_uint8), L, _ptr(root, C.c_int32), _ptr(cs, C.c_int8),
                                           _ptr(cp, C.c_int16), _ptr(line, C.c_int32), _ptr(ln, C.c_int32)), "ao_tree_proofs")
        return dict(status=root[:, 0].copy(), plies=root[:, 1].copy(), proven=root[:, 2].copy(), walked=root[:, 3].copy(),
                    child_status=cs, child_plies=cp, line=line, len=ln)

    def set_proof_moves(self, on=True):
        """Proof moves (ao_set_proof_moves): with the switch on, end_move / search rewrite pi by what the root's tree proves
        before it is returned and played -- utils.proof_pi: one-hot on the fastest proven win, or renormalised over the moves
        that are not proven lost. visit, policy and the games' streams are what they are without it; the recorded pi is then no
        longer pure visit counts. Off (the default) nothing runs. Refused inside a move and for an open roll; roll_begin raises
        while it is on."""
        self._check(self._L.ao_set_proof_moves(self._h, 1 if on else 0), "ao_set_proof_moves")

    def proof_move_stats(self, per_game=False, reset=False):
        """dict(none, win, pruned, moved): the moves that got each verdict (PM_*) under set_proof_moves since the last reset,
        over the active games of every end_move (ao_proof_move_records); per_game=True adds `verdict`, int32 [G]: each game's
        most recent one. A move that search() repeated on the fp32-MFMA trunk is ended once and counts once."""
        out = np.zeros(4, np.int64)
        v = np.zeros(self.G, np.int32) if per_game else None
        self._check(self._L.ao_proof_move_records(self._h, _ptr(v, C.c_int32), _ptr(out, C.c_int64), 1 if reset else 0),
                    "ao_proof_move_records")
        d = dict(none=int(out[0]), win=int(out[1]), pruned=int(out[2]), moved=int(out[3]))
        if per_game:
            d["verdict"] = v
        return d

    # -- tree snapshots
    def export_trees(self, mask=None):
        """The trees and streams of the masked games (None: all) as a TreeSnapshot, games in ascending order (ao_tree_export).
        Read-only on the engine; fails inside a move."""
        from .snapshot import TreeSnapshot
        mk = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        st = self.tree_stats(mk)                       # sizes every array before the pack launch
        sel = np.arange(self.G) if mk is None else np.flatnonzero(mk)
        ng = int(sel.size)
        N = int(st["expanded"][sel].sum())
        E = int((st["entries"][sel] - 1)[st["expanded"][sel] > 0].sum())
        snap = TreeSnapshot(self.board_size, self.inplanes, 0, hdr=np.zeros((ng, _lib.AO_SNAP_HDR), np.int32),
                            gauss=np.zeros(ng), mt=np.zeros((ng, 624), np.uint32), moves=np.zeros((ng, self.A), np.int32),
                            nchild=np.zeros(N, np.int32), parent=np.zeros(N, np.int32), parent_edge=np.zeros(N, np.int32),
                            act=np.zeros(E, np.uint8), n=np.zeros(E, np.int32), w=np.zeros(E, np.float32),
                            q=np.zeros(E, np.float32), p=np.zeros(E, np.float64), child=np.zeros(E, np.int32))
        s = snap._struct()
        self._check(self._L.ao_tree_export(self._h, _ptr(mk, C.c_uint8), C.byref(s)), "ao_tree_export")
        assert (s.games, s.nodes, s.edges) == (ng, N, E)
        snap.win_mark, snap.sims, snap.noise, snap.c_puct = s.win_mark, s.sims, s.noise, s.c_puct
        return snap

    def import_trees(self, snapshot, games=None):
        """Snapshot game i goes into slot games[i] (None: slot i), tree, stream, moves and root status; other games are
        untouched (ao_tree_import). The snapshot may come from another slot, engine, `games`, node_cap or num_mcts; board,
        inplanes and win_mark must match. Raises EngineError, with every game left as it was, on a damaged snapshot, a game
        with more nodes than node_cap - num_mcts - 1, a bad game index, or inside a move. `play` must follow a search."""
        g = np.arange(snapshot.games, dtype=np.int32) if games is None else np.ascontiguousarray(games, np.int32).reshape(-1)
        s = snapshot._struct()
        self._check(self._L.ao_tree_import(self._h, _ptr(g, C.c_int32), int(g.size), C.byref(s)), "ao_tree_import")

    def tree_timing(self, enable=True):
        """(total ms, launches) of the TIMED per-simulation tree kernel launches (k_expand_select) since the last call;
        enable = n > 1 times every n-th launch only."""
        ms, cnt = C.c_double(0), C.c_int64(0)
        self._check(self._L.ao_tree_timing(self._h, int(enable), C.byref(ms), C.byref(cnt)), "ao_tree_timing")
        return ms.value, cnt.value

    def trim_stats(self):
        """(child subtrees dropped, re-rootings that dropped any) since the engine was created: non-zero only when
        a game's kept tree outgrew node_cap - sims - 1 nodes (ao_trim_stats)."""
        a, b = C.c_int64(0), C.c_int64(0)
        self._check(self._L.ao_trim_stats(self._h, C.byref(a), C.byref(b)), "ao_trim_stats")
        return a.value, b.value

    def search_stats(self):
        v = [C.c_int64(0) for _ in range(4)]
        self._check(self._L.ao_search_stats(self._h, *[C.byref(x) for x in v]), "ao_search_stats")
        return dict(levels=v[0].value, ties=v[1].value, terminal=v[2].value, evaluated=v[3].value)

    def set_row_cap(self, rows):
        """rows > 0: `search` hands out the evaluation-batch rows per simulation (terminal leaves take none) and evaluates at
        most `rows` leaves per simulation -- fewer rows than games = over-subscription; 0: the per-move packing (ao_set_row_cap)."""
        self._check(self._L.ao_set_row_cap(self._h, int(rows)), "ao_set_row_cap")
        self.row_cap = int(rows)

    def row_stats(self):
        """dict(launches, rows_live, rows_launched, waits) over the searches that handed out rows per simulation (ao_row_stats)."""
        v = [C.c_int64(0) for _ in range(4)]
        self._check(self._L.ao_row_stats(self._h, *[C.byref(x) for x in v]), "ao_row_stats")
        return dict(launches=v[0].value, rows_live=v[1].value, rows_launched=v[2].value, waits=v[3].value)

    def set_eval_log(self, games, dev_ptr=None, capacity_floats=0):
        """Test hook (ao_set_eval_log): record the (policy, value) the listed games' leaves are evaluated with in `search`."""
        g = np.ascontiguousarray(list(games), np.int32)
        self._check(self._L.ao_set_eval_log(self._h, _ptr(g, C.c_int32) if g.size else None, int(g.size), dev_ptr,
                                            int(capacity_floats)), "ao_set_eval_log")

    def eval_log_count(self):
        """Simulations recorded since set_eval_log (ao_eval_log_count). A move that search() repeated on the fp32-MFMA trunk
        (fp16_range_events) is in the log with BOTH attempts: the rows of the discarded first one -- clamped evaluations --
        come first, the repeat's follow them, as long as the buffer has room."""
        return int(self._L.ao_eval_log_count(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._L.ao_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
