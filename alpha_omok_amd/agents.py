"""Drop-in `agents.ZeroAgent` (reference: agents.py:16-260) and the net-free rollout agents
`PUCTAgent` / `UCTAgent` (agents.py:263-614), all backed by the HIP engine.

Same constructor, attributes and methods as the reference class; the per-simulation Python loop
is replaced by the batched tree kernels with G = 1. The evaluator is `self.model`, assigned after
construction exactly as main.py:81 / eval_main.py:87-101 do:
  * a module whose state_dict has the PVNet wire format runs on the hand-written MFMA forward
    (weights are re-exported whenever the module's parameters change);
  * any other callable `model(x[B,C,Bd,Bd]) -> (policy[B,A], value[B])` is called once per
    simulation on the leaf batch (planes are produced on the device).
Randomness is the process-global numpy stream (main.py:60): its MT19937 state is moved into the
engine for the search and written back afterwards, so `np.random.seed(s)` reproduces the
reference's visit counts and the stream position it leaves behind.
"""
import sys
import time

import numpy as np

from .evaluator import Evaluator
from .engine import AO_NODE_ABSENT, AO_ROOT_FRESH, Engine, EngineError  # noqa: F401

PRINT_MCTS = True


class Agent(object):
    def __init__(self, board_size):
        self.policy = np.zeros(board_size ** 2, 'float')
        self.visit = np.zeros(board_size ** 2, 'float')
        self.message = 'Hello'

    def get_policy(self):
        return self.policy

    def get_visit(self):
        return self.visit

    def get_name(self):
        return type(self).__name__

    def get_message(self):
        return self.message

    def get_pv(self, root_id):
        return None, None


class _TreeView(object):
    """Stands in for the reference's `self.tree` dict: len() / clear(), and the read idiom `tree[node_id]` /
    `node_id in tree` (agents.py:52,206-210), answered from the device tree by Engine.tree_lookup. A node's entry is
    {'child': actions in stored order, 'n': float, 'w' / 'q': np.float32, 'p': np.float64}; the root has no parent edge in
    the engine, so its 'w' / 'q' / 'p' are NaN."""

    def __init__(self, agent):
        self._agent = agent

    def __len__(self):
        eng = self._agent._engine
        return 0 if eng is None else eng.tree_nodes(0)[1]

    def __bool__(self):
        return len(self) > 0

    def _lookup(self, node_id):
        eng = self._agent._engine
        if eng is None or not isinstance(node_id, (tuple, list)) or len(node_id) < 1 or node_id[0] != 0:
            return None
        try:
            ids = [tuple(int(a) for a in node_id)]
        except (TypeError, ValueError):
            return None
        r = eng.tree_lookup(ids, games=[0])
        return None if r["status"][0] == AO_NODE_ABSENT else r

    def __contains__(self, node_id):
        return self._lookup(node_id) is not None

    def __getitem__(self, node_id):
        r = self._lookup(node_id)
        if r is None:
            raise KeyError(node_id)
        k = int(r["nchild"][0])
        return {'child': r["child_action"][0, :k].tolist(), 'n': float(r["n"][0]), 'w': np.float32(r["w"][0]),
                'q': np.float32(r["q"][0]), 'p': np.float64(r["p"][0])}

    def clear(self):
        if self._agent._engine is not None:
            self._agent._engine.reset()


class ZeroAgent(Agent):
    def __init__(self, board_size, num_mcts, inplanes, noise=True, device=0, node_cap=0, leaf_symmetry=None, leaf_tactics=None,
                 proof_moves=False):
        """leaf_symmetry: None, or an int key -- every leaf of the search is then evaluated under a symmetry of the board
        drawn from (key, stones on the leaf, simulation index) (Engine.set_leaf_symmetry).
        leaf_tactics: None / False, True (max_depth 2, max_nodes 16) or dict(max_depth, max_nodes) -- a leaf whose mover has a
        proven forced win by continuous fours is valued +1 (Engine.set_leaf_tactics). A one-game engine then runs without the
        fused per-game step.
        proof_moves: True -- get_pi's pi follows what the root's tree proves (Engine.set_proof_moves, utils.proof_pi): one-hot on
        the fastest proven win, or without the moves that are proven lost; last_proof_verdict tells which (PM_*)."""
        super(ZeroAgent, self).__init__(board_size)
        self.proof_moves = bool(proof_moves)
        self.last_proof_verdict = 0
        self.leaf_symmetry = leaf_symmetry
        from . import utils
        self.leaf_tactics = utils.leaf_tactics_limits(leaf_tactics)
        self.board_size = board_size
        self.num_mcts = num_mcts
        self.inplanes = inplanes
        self.win_mark = 3 if board_size == 3 else 5
        self.alpha = 10 / self.board_size ** 2
        self.c_puct = 5
        self.noise = noise
        self.root_id = None
        self.model = None
        self.is_real_root = True
        self.tree = _TreeView(self)
        self._device = device
        self._node_cap = node_cap
        self._engine = None
        self._evaluator = Evaluator(device)
        self._positions = None

    # -- engine plumbing --------------------------------------------------------------------
    def _eng(self):
        if self._engine is None:
            self._engine = Engine(self.board_size, self.num_mcts, self.inplanes, games=1, noise=self.noise,
                                  device=self._device, node_cap=self._node_cap, c_puct=float(self.c_puct),
                                  alpha=float(self.alpha), win_mark=self.win_mark)
            if self.leaf_symmetry is not None:
                self._engine.set_leaf_symmetry(self.leaf_symmetry)
            if self.leaf_tactics is not None:
                self._engine.set_leaf_tactics(*self.leaf_tactics)
            if self.proof_moves:
                self._engine.set_proof_moves(True)
        return self._engine

    # -- reference API ----------------------------------------------------------------------
    def reset(self):
        self.root_id = None
        self.is_real_root = True
        if self._engine is not None:
            self._engine.reset()

    def get_pi(self, root_id, tau, sims=None, early_stop=False, allowed=None, tactics=None):
        """sims: simulations of THIS move (1..num_mcts; None: num_mcts); early_stop=True: a tau == 0 search ends once its move is
        decided (utils.move_decided) -- same pi and move, fewer visits in the tree the next move inherits. allowed: the cells
        that may be searched at the root, a bool [A] or a list of cells (Engine.search); tactics: True or dict(max_depth,
        max_nodes, solved_sims) -- the forced-win solver restricts the root first (a proven win: the winning first moves; a
        proven threat: the replies not proven to lose); last_tactics tells what it said."""
        start = time.time()
        eng = self._eng()
        if allowed is not None:
            a = np.asarray(allowed)
            if a.dtype != bool or a.shape != (self.board_size ** 2,):
                cells = np.asarray(list(allowed), np.int64).reshape(-1)
                if cells.size and (cells.min() < 0 or cells.max() >= self.board_size ** 2):
                    raise ValueError("allowed: a cell is off the board")
                a = np.zeros(self.board_size ** 2, bool)
                a[cells] = True
            allowed = a.reshape(1, -1)
        st = np.random.get_state()                      # the reference's global stream
        eng.set_rng_state(0, st[1], st[2], st[3], st[4])
        status = eng.set_root(0, list(root_id)[1:])
        self.root_id = tuple(root_id)
        self.is_real_root = (status == AO_ROOT_FRESH)
        num = (self.num_mcts if sims is None else int(sims)) + (1 if self.is_real_root else 0)
        def progress(i):
            self.message = 'simulation: {}\r'.format(i)

        pi, visit, policy = self._evaluator.search(eng, self.model, tau, on_sim=progress, sims=sims,
                                                   early_stop=True if early_stop else None, allowed=allowed, tactics=tactics)
        self.last_tactics = eng.last_tactics()
        if self.proof_moves:
            self.last_proof_verdict = int(eng.proof_move_stats(per_game=True)["verdict"][0])
        mt, pos, has_gauss, gauss = eng.get_rng_state(0)
        np.random.set_state(('MT19937', mt, pos, has_gauss, gauss))
        self.message = 'simulation: {}\r'.format(num)
        self.visit = visit[0]
        self.policy = policy[0]
        if PRINT_MCTS:
            sys.stdout.write('simulation: {}\r'.format(num))
            print("{} simulations end ({:0.0f}s)".format(num, time.time() - start))
        return pi[0]

    def del_parents(self, root_id):
        """The engine keeps only the subtree of the last root (what del_parents leaves reachable)."""
        expanded, entries = (0, 0) if self._engine is None else self._engine.tree_nodes(0)
        print('tree size:', entries)
        print('tree depth:', 0 if expanded == 0 else '>= 1')

    def principal_variation(self, max_len=None):
        """(actions, n, q) along the most-visited line from the current root (Engine.principal_variations): int32 actions,
        int32 visit counts and the float32 q of each edge; empty before the first search."""
        if self._engine is None:
            return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)
        r = self._engine.principal_variations(max_len)
        k = int(r["len"][0])
        return r["action"][0, :k].copy(), r["n"][0, :k].copy(), r["q"][0, :k].copy()

    def get_proof(self, root_id=None, max_len=None):
        """What the tree below the current root proves (Engine.tree_proofs; no reference counterpart): dict(status -- PROOF_*
        for the side to move at the root --, plies to the end of the game, cells int8 [B, B]: the PROOF_* of the move on each
        cell for the mover, -1 on a cell without a move, cell_plies int16 [B, B], line: the actions of the proof line). root_id:
        None or the id of the last get_pi / load_tree -- the engine keeps that root's subtree only. Before any search: unknown."""
        B = self.board_size
        if root_id is not None and self.root_id is not None and tuple(root_id) != tuple(self.root_id):
            raise ValueError("get_proof: %r is not the current root %r" % (tuple(root_id), tuple(self.root_id)))
        if self._engine is None:
            return dict(status=0, plies=0, cells=np.full((B, B), -1, np.int8), cell_plies=np.zeros((B, B), np.int16),
                        line=np.zeros(0, np.int32))
        r = self._engine.tree_proofs(max_len=max_len)
        return dict(status=int(r["status"][0]), plies=int(r["plies"][0]), cells=r["child_status"][0].reshape(B, B).copy(),
                    cell_plies=r["child_plies"][0].reshape(B, B).copy(), line=r["line"][0, :int(r["len"][0])].copy())

    def save_tree(self, path):
        """Puts the searched position aside: the tree below the current root, its id and the numpy stream position the last
        get_pi left, as a TreeSnapshot file (Engine.export_trees)."""
        self._eng().export_trees().save(path)

    def load_tree(self, path):
        """Takes up what save_tree wrote: tree[...], principal_variation() and the next get_pi answer as the saved agent's
        would. The process-global numpy stream is left alone (get_pi hands it to the engine, as always)."""
        from .snapshot import TreeSnapshot
        snap = TreeSnapshot.load(path)
        if snap.games != 1:
            raise ValueError("load_tree: the file holds %d games, a ZeroAgent has one" % snap.games)
        self._eng().import_trees(snap)
        self.root_id = (0,) + tuple(self._engine.get_moves(0))
        self.is_real_root = int(snap.hdr[0, 3]) == AO_ROOT_FRESH

    def tree_depth(self):
        """The number del_parents prints as `tree depth` in the reference (agents.py:241-250), from the device tree."""
        return 0 if self._engine is None else int(self._engine.tree_stats()["depth"][0])

    def get_pv(self, root_id, symmetries=1):
        """symmetries=8: the mean over the eight symmetries of the board (PositionBatch.evaluate); needs a model the native
        forward takes."""
        if symmetries != 1:
            net = self.model if hasattr(self.model, "forward_ptr") else self._evaluator.native_net(self.model, self.board_size, self.inplanes)
            if net is None:
                raise ValueError("get_pv(symmetries=%r) needs a model in the PVNet wire format or an engine.Net" % (symmetries,))
            p, v, _, _ = self._position_batch().evaluate(net, [tuple(root_id)], symmetries=symmetries)
            return p[0], v[0]
        import torch
        from . import utils
        state = utils.get_state_pt(root_id, self.board_size, self.inplanes)
        x = torch.from_numpy(state[None]).float()
        net = self._evaluator.native_net(self.model, self.board_size, self.inplanes)
        with torch.no_grad():
            if net is not None:
                p, v = net(x.cuda(self._device))
            else:
                if hasattr(self.model, "eval"):
                    self.model.eval()
                p, v = self.model(x.to(Evaluator._model_device(self.model)))
        return p.detach().cpu().numpy()[0], v.detach().cpu().numpy()[0]

    def _position_batch(self):
        from .positions import PositionBatch
        if self._positions is None:
            self._positions = PositionBatch(self.board_size, self.inplanes, self.win_mark, device=self._device)
        return self._positions

    def get_win_cells(self, root_id):
        """The cells that win at once in the position of `root_id` (PositionBatch.win_cells): (mine, theirs), bool [B, B]
        -- where the side to move completes a line, and where its opponent would: the cells to show as "must block
        here" beside get_pv. Both are empty on a finished game. ValueError for an id that is not a legal move list."""
        d = self._position_batch().win_cells([root_id])
        if d["err"][0]:
            raise ValueError("root_id %r is not a legal move list (err %d)" % (root_id, int(d["err"][0])))
        B = self.board_size
        return d["mine"][0].reshape(B, B).astype(bool), d["theirs"][0].reshape(B, B).astype(bool)

    def get_forced_win(self, root_id, max_depth=8, max_nodes=2000):
        """Is there a forced win by continuous fours for the side to move in the position of `root_id`
        (PositionBatch.forced_wins)? (result, depth, moves, line): result 0 no / 1 yes / 2 the node budget ran out, depth
        the fewest attacker moves, moves bool [B, B] every first move that wins that fast, line the principal line as a
        list of cells. ValueError for an id that is not a legal move list or limits outside 1..16 / 1..65536."""
        d = self._position_batch().forced_wins([root_id], max_depth, max_nodes)
        if d["err"][0]:
            raise ValueError("root_id %r is not a legal move list (err %d)" % (root_id, int(d["err"][0])))
        B = self.board_size
        return (int(d["result"][0]), int(d["depth"][0]), d["moves"][0].reshape(B, B).astype(bool),
                d["line"][0, :int(d["line_len"][0])].tolist())

    def get_forced_defences(self, root_id, max_depth=8, max_nodes=2000):
        """Which moves of the side to move stop the opponent's forced win by continuous fours in the position of
        `root_id` (PositionBatch.forced_defences)? (threat, threat_depth, safe, losing): threat 0 the opponent has no
        forced win if the mover passes / 1 it has one / 2 the node budget ran out, threat_depth its fewest attacker moves,
        safe bool [B, B] the empty cells after which the opponent has none -- the "must answer here" set when there is a
        threat --, losing bool [B, B] those after which it has one (cells whose search ran out of nodes are in neither).
        All empty on a finished game. ValueError for an id that is not a legal move list or limits outside 1..16 /
        1..65536."""
        from .positions import FD_LOSES, FD_SAFE
        d = self._position_batch().forced_defences([root_id], max_depth, max_nodes)
        if d["err"][0]:
            raise ValueError("root_id %r is not a legal move list (err %d)" % (root_id, int(d["err"][0])))
        B = self.board_size
        reply = d["reply"][0].reshape(B, B)
        return int(d["threat"][0]), int(d["threat_depth"][0]), reply == FD_SAFE, reply == FD_LOSES

    def get_root_tactics(self, root_id, max_depth=6, max_nodes=512):
        """What the forced-win solver says about searching the position of `root_id` (Engine.root_tactics, utils.root_tactics
        is the definition): (verdict, depth, allowed bool [B, B], nodes, unknown) -- verdict RT_WIN a forced win for the side
        to move (allowed: its winning first moves), RT_DEFEND / RT_LOST the opponent threatens one (allowed: the replies not
        proven to lose / every empty cell when all lose), RT_NONE nothing proven. The agent's root moves to `root_id`, as in
        get_pi. ValueError for limits outside 1..16 / 1..65536."""
        eng = self._eng()
        eng.set_root(0, list(root_id)[1:])
        self.root_id = tuple(root_id)
        r = eng.root_tactics(max_depth=max_depth, max_nodes=max_nodes)
        B = self.board_size
        return int(r["verdict"][0]), int(r["depth"][0]), r["allowed"][0].reshape(B, B), int(r["nodes"][0]), int(r["unknown"][0])

    def get_pv_batch(self, root_ids):
        """get_pv for many ids in one call (PositionBatch.evaluate): (policy float32 [n, A], value float32 [n],
        status int32 [n] -- utils.check_win of each position, terminal ones are evaluated too --, err int32 [n]). The planes
        are built on the device; a PVNet-shaped model runs on the native forward, any other model is called once on the
        whole plane batch. Ids with err != 0 (a move off the board or onto a stone) get zeros."""
        pb = self._position_batch()
        net = self._evaluator.native_net(self.model, self.board_size, self.inplanes)
        if net is not None:
            return pb.evaluate(net, root_ids)
        import torch
        d = pb.describe(root_ids)
        x = pb.planes(root_ids)
        if hasattr(self.model, "eval"):
            self.model.eval()
        with torch.no_grad():
            p, v = self.model(x.to(Evaluator._model_device(self.model)))
        n = d["err"].shape[0]
        p = np.ascontiguousarray(p.detach().reshape(n, -1).float().cpu().numpy())
        v = np.ascontiguousarray(v.detach().reshape(n).float().cpu().numpy())
        p[d["err"] != 0] = 0
        v[d["err"] != 0] = 0
        return p, v, d["status"], d["err"]


class _RolloutAgent(Agent):
    """Shared body of PUCTAgent / UCTAgent (agents.py:263-614): every get_pi is a fresh search of
    num_mcts + 1 simulations with random playouts, run as ONE kernel on the device with the
    process-global np.random state (moved in and out as ZeroAgent does)."""
    _MODE = 0

    def __init__(self, board_size, num_mcts, device=0):
        super(_RolloutAgent, self).__init__(board_size)
        self.board_size = board_size
        self.num_mcts = num_mcts
        self.win_mark = 3 if board_size == 3 else 5
        self.root_id = None
        self.board = None
        self.turn = None
        self.is_real_root = True
        self._device = device
        self._engine = None
        self.tree = {}     # the reference keeps its dict across calls but never reads old entries

    def reset(self):
        self.is_real_root = True
        self.root_id = None
        self.board = None
        self.turn = None
        self.tree.clear()

    def get_pi(self, root_id, board, turn, tau):
        from . import utils
        from .rollout import RolloutEngine
        if turn != utils.get_turn(root_id):
            raise ValueError("turn does not match root_id")
        if self._engine is None:
            self._engine = RolloutEngine(self.board_size, self.num_mcts, self._MODE, games=1, device=self._device)
        self.root_id, self.board, self.turn = root_id, board, turn
        start = time.time()
        st = np.random.get_state()
        self._engine.set_rng_state(0, st[1], st[2], st[3], st[4])
        pi, stat, _ = self._engine.search([root_id])
        mt, pos, hg, gs = self._engine.get_rng_state(0)
        np.random.set_state(('MT19937', mt, pos, hg, gs))
        if self._MODE == 0:
            self.visit = stat[0].copy()
        self.tree = {root_id: {'child': [a for a in range(self.board_size ** 2) if a not in root_id[1:]]}}
        if PRINT_MCTS:
            print("{} simulations end ({:0.0f}s)".format(self.num_mcts, time.time() - start))
        return pi[0].copy()

    def del_parents(self, root_id):
        self.tree = {k: v for k, v in self.tree.items() if len(k) >= len(root_id)}


class PUCTAgent(_RolloutAgent):
    """agents.py:263-441: PUCT over uniform priors, value from one random playout per expansion."""
    _MODE = 0


class UCTAgent(_RolloutAgent):
    """agents.py:443-614: UCB1 (unvisited children first), value from one random playout per expansion."""
    _MODE = 1
