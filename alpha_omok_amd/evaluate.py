"""Head-to-head evaluation of two ZeroAgents (the part of eval_main.py that sits on the hot path:
eval_main.py:137-170,191-198,229-333 without pygame / Flask).

Each player keeps its own tree; after the opponent's reply the next `get_pi(root_id)` re-roots two
plies down (known child, possibly unexpanded, or a fresh root when the reply was never reached),
exactly the call pattern of `Evaluator.get_action`. Players search with noise off and tau = 0.

`evaluate` plays the matches one after another through two drop-in agents, drawing every tie-break
from the process-global numpy stream like the reference. `evaluate_batched` plays all N_MATCH games
of eval_main.py:204-333 CONCURRENTLY on two G = n_match engines (one per network): per ply one
`ao_set_roots` launch moves every match's root in both trees and one fused search per side decides
the moves of the matches where that side is to move. Concurrent matches cannot share one stream, so
match i owns a stream seeded seed + i that both of its players draw from in turn -- match i is then
exactly `np.random.seed(seed + i); play_match(...)`.
"""
import numpy as np

from . import utils


def elo(player_elo, enemy_elo, p_winscore, e_winscore):
    """eval_main.py:191-198 (K = 32)."""
    elo_diff = enemy_elo - player_elo
    ex_pw = 1 / (1 + 10 ** (elo_diff / 400))
    ex_ew = 1 / (1 + 10 ** (-elo_diff / 400))
    player_elo += 32 * (p_winscore - ex_pw)
    enemy_elo += 32 * (e_winscore - ex_ew)
    return player_elo, enemy_elo


def _is_zero(agent):
    """ZeroAgent-style get_pi(root_id, tau) vs the rollout agents' get_pi(root_id, board, turn, tau)
    (the isinstance test of eval_main.py:139,146)."""
    inner = getattr(agent, "ag", agent)
    return not hasattr(inner, "_MODE")


def play_match(player, enemy, board_size, enemy_turn, max_plies=None, monitor=None):
    """One game; `enemy_turn` (0 black / 1 white) is the colour of `enemy` (eval_main.py:229-300). Players may be
    ZeroAgents or the rollout agents (PUCTAgent / UCTAgent); when the PLAYER is a rollout agent and a `monitor`
    ZeroAgent is given, the monitor searches the same root right after the player, as Evaluator.get_action does
    (eval_main.py:141-144: its tie-breaks come out of the shared stream). Returns (win_index, moves)."""
    win_mark = 3 if board_size == 3 else 5
    root_id = (0,)
    turn = 0
    win_index = 0
    moves = []
    while win_index == 0:
        agent = enemy if turn == enemy_turn else player
        if _is_zero(agent):
            pi = agent.get_pi(root_id, tau=0)
        else:
            pi = agent.get_pi(root_id, utils.get_board(root_id, board_size), turn, tau=0)
            if agent is player and monitor is not None:
                monitor.get_pi(root_id, tau=0)
        _, action_index = utils.argmax_onehot(pi)
        root_id = root_id + (int(action_index),)
        moves.append(int(action_index))
        win_index = utils.check_win(utils.get_board(root_id, board_size), win_mark)
        turn ^= 1
        if max_plies and len(moves) >= max_plies:
            break
    player.reset()
    enemy.reset()
    if monitor is not None:
        monitor.reset()
    return win_index, moves


def evaluate(player, enemy, board_size, n_match=12, player_elo=1500.0, enemy_elo=1500.0, return_games=False, monitor=None):
    """n_match games with the colours swapped every game (eval_main.py:213-333). Returns the result
    tally and the final ELO pair (and the [(win_index, moves)] list with return_games)."""
    result = {'Player': 0, 'Enemy': 0, 'Draw': 0}
    enemy_turn = 1
    games = []
    for _ in range(n_match):
        win_index, moves = play_match(player, enemy, board_size, enemy_turn, monitor=monitor)
        games.append((win_index, moves))
        if win_index == 3:
            result['Draw'] += 1
            pw = ew = 0.5
        elif (win_index == 1) == (enemy_turn == 1):   # black won and the player was black, or ...
            result['Player'] += 1
            pw, ew = 1.0, 0.0
        else:
            result['Enemy'] += 1
            pw, ew = 0.0, 1.0
        player_elo, enemy_elo = elo(player_elo, enemy_elo, pw, ew)
        enemy_turn ^= 1
    if return_games:
        return result, (player_elo, enemy_elo), games
    return result, (player_elo, enemy_elo)


last_proof_moves = {}        # evaluate_batched(proof_moves=): side index -> Engine.proof_move_stats() of that side's engine over the matches
last_search_totals = {}      # evaluate_batched: searches, simulations asked for, searches settled and simulations saved by early stop


class _ZeroSide:
    """One network's side of evaluate_batched: a G-game engine + evaluator; searches the masked matches at their ids."""

    def __init__(self, model, sims, board_size, inplanes, G, device, early_stop=False, tactics=None, forward_precision=None,
                 leaf_symmetry=None, seeds=None, leaf_tactics=None, proof_moves=False):
        from .engine import Engine
        from .evaluator import Evaluator
        self.eng = Engine(board_size, sims, inplanes, games=G, noise=False, device=device)
        if leaf_symmetry is not None:
            # the matches' streams are handed from side to side as states, not seeds: the keys are set from the matches' seeds directly
            self.eng.set_leaf_symmetry(leaf_symmetry, keys=[utils.leaf_key(leaf_symmetry, s) for s in seeds])
        limits = utils.leaf_tactics_limits(leaf_tactics)
        if limits is not None:
            self.eng.set_leaf_tactics(*limits)
        self.proof_moves = bool(proof_moves)
        if self.proof_moves:
            self.eng.set_proof_moves(True)                # the move follows what the root's tree proves (utils.proof_pi)
        self.ev, self.model = Evaluator(device), model
        if forward_precision is not None:
            self.ev.net_precision = forward_precision    # Net.precision of this side's exported network ("fp16": the opt-in one-product forward)
        self.tau0 = np.zeros(G, np.int8)
        self.early_stop = True if early_stop else None   # every search here has tau == 0: its result is the leader alone
        self.tactics = tactics if tactics else None      # Engine.search(tactics=): the forced-win solver restricts every root first
        self.sims, self.searches = sims, 0

    def seed(self, i, s):
        self.eng.seed(i, s)

    def get_rng_state(self, i):
        return self.eng.get_rng_state(i)

    def set_rng_state(self, i, mt, pos, hg, gs):
        self.eng.set_rng_state(i, mt, pos, hg, gs)

    def search(self, ids, mask):
        self.eng.set_roots(ids, mask)
        pi, _, _ = self.ev.search(self.eng, self.model, self.tau0, active=mask, early_stop=self.early_stop, tactics=self.tactics)
        self.searches += int(np.count_nonzero(mask))
        return pi

    def close(self):
        self.eng.close()


class _RolloutSide:
    """A PUCTAgent / UCTAgent side ('puct' / 'uct', agents.py:263-614): every get_pi is a fresh search, one kernel for
    all masked matches."""

    def __init__(self, kind, sims, board_size, G, device):
        from .rollout import PUCT, UCT, RolloutEngine
        self.eng = RolloutEngine(board_size, sims, PUCT if kind == 'puct' else UCT, games=G, device=device)

    def seed(self, i, s):
        self.eng.seed(i, s)

    def get_rng_state(self, i):
        return self.eng.get_rng_state(i)

    def set_rng_state(self, i, mt, pos, hg, gs):
        self.eng.set_rng_state(i, mt, pos, hg, gs)

    def search(self, ids, mask):
        pi, _, _ = self.eng.search(ids, active=mask)
        return pi

    def close(self):
        self.eng.close()


def check_forward_precision(forward_precision):
    """evaluate_batched's forward_precision as the pair (player's, enemy's); ValueError for anything that is not None, one of
    "fp32" / "fp16" / "fp16-all", or a pair of them. Host only."""
    if forward_precision is None or isinstance(forward_precision, str):
        forward_precision = (forward_precision, forward_precision)
    if len(forward_precision) != 2 or any(p not in (None, "fp32", "fp16", "fp16-all") for p in forward_precision):
        raise ValueError("forward_precision: 'fp32', 'fp16', 'fp16-all' or a pair (player, enemy) of them")
    return tuple(forward_precision)


def evaluate_batched(player_model, enemy_model, board_size, n_mcts_player, n_mcts_enemy=None, inplanes=5, n_match=12,
                     player_elo=1500.0, enemy_elo=1500.0, seed=0, device=0, max_plies=None, monitor_model=None,
                     n_mcts_monitor=None, early_stop=False, tactics=None, forward_precision=None, leaf_symmetry=None,
                     leaf_tactics=None, proof_moves=False):
    """All n_match games at once (colours swapped every game, eval_main.py:213-333). `*_model`: whatever
    ZeroAgent.model accepts (a PVNet-shaped module runs on the native forward), or 'puct' / 'uct' for the rollout
    agents (eval_main.py:68-73,106-111). With a rollout PLAYER and a `monitor_model`, the monitor ZeroAgent searches
    the same roots right after the player as Evaluator.get_action does (eval_main.py:141-144). Returns (result tally,
    (player_elo, enemy_elo), [(win_index, moves) per match]); the ELO updates are applied in match order.
    early_stop=True: the ZeroAgent sides (both of them) end a search once its move is decided (utils.move_decided): the same move,
    fewer simulations; the later plies then search on smaller inherited trees, so a match need not be the one full searches play.
    tactics: Engine.search(tactics=) for the ZeroAgent sides -- True or a dict for both, or a pair (player's, enemy's) with None for
    a side that searches plainly, so that the switch's strength can be measured against the same network without it.
    forward_precision: "fp32" / "fp16" / "fp16-all" (Net.precision of the exported networks of the ZeroAgent sides) for both, or a pair (player's,
    enemy's); None leaves the default. A side given as an engine.Net keeps the precision it was set to.
    leaf_symmetry: an int key -- the ZeroAgent sides evaluate every leaf under a symmetry of the board drawn per leaf
    (Engine.set_leaf_symmetry; match i's key is utils.leaf_key(key, seed + i)) -- for both, or a pair (player's, enemy's) with None
    for a side that searches plainly, as for tactics.
    leaf_tactics: True or dict(max_depth, max_nodes) -- the ZeroAgent sides value a leaf whose mover has a proven forced win +1
    (Engine.set_leaf_tactics) -- for both, or a pair (player's, enemy's) with None for a side that searches plainly. Each side
    has its own engine.
    proof_moves: True -- the ZeroAgent sides play what their root's tree proves (Engine.set_proof_moves: the fastest proven win,
    never a move that is proven lost while another is not) -- for both, or a pair (player's, enemy's) of bools; the verdicts are
    counted per side in evaluate.last_proof_moves."""
    forward_precision = check_forward_precision(forward_precision)
    n_mcts_enemy = n_mcts_player if n_mcts_enemy is None else n_mcts_enemy
    G = n_match
    win_mark = 3 if board_size == 3 else 5

    side_tactics = tuple(tactics) if isinstance(tactics, (tuple, list)) else (tactics, tactics)
    if len(side_tactics) != 2:
        raise ValueError("tactics: one value for both sides or a pair (player, enemy)")

    side_sym = tuple(leaf_symmetry) if isinstance(leaf_symmetry, (tuple, list)) else (leaf_symmetry, leaf_symmetry)
    if len(side_sym) != 2:
        raise ValueError("leaf_symmetry: one value for both sides or a pair (player, enemy)")
    side_leaf = tuple(leaf_tactics) if isinstance(leaf_tactics, (tuple, list)) else (leaf_tactics, leaf_tactics)
    if len(side_leaf) != 2:
        raise ValueError("leaf_tactics: one value for both sides or a pair (player, enemy)")
    for lt in side_leaf:
        utils.leaf_tactics_limits(lt)            # (a bad value is an argument error before any engine exists)
    side_proof = tuple(proof_moves) if isinstance(proof_moves, (tuple, list)) else (proof_moves, proof_moves)
    if len(side_proof) != 2 or any(not isinstance(pm, (bool, np.bool_, type(None))) for pm in side_proof):
        raise ValueError("proof_moves: one bool for both sides or a pair (player, enemy)")
    match_seeds = [(seed + i) & 0xFFFFFFFF for i in range(G)]

    def make(model, sims, tac, prec, sym, leaf, proof):
        if isinstance(model, str):
            return _RolloutSide(model, sims, board_size, G, device)
        return _ZeroSide(model, sims, board_size, inplanes, G, device, early_stop, tac, prec, sym, match_seeds, leaf, proof)

    sides = [make(player_model, n_mcts_player, side_tactics[0], forward_precision[0], side_sym[0], side_leaf[0], side_proof[0]),
             make(enemy_model, n_mcts_enemy, side_tactics[1], forward_precision[1], side_sym[1], side_leaf[1], side_proof[1])]
    monitor = None
    if monitor_model is not None and isinstance(player_model, str):
        monitor = _ZeroSide(monitor_model, n_mcts_monitor or n_mcts_enemy, board_size, inplanes, G, device)
        sides.append(monitor)                                       # index 2: searches right after side 0
    enemy_turn = np.array([1 - (i % 2) for i in range(G)])          # match 0: the player is black
    ids = [(0,) for _ in range(G)]
    wins = np.zeros(G, np.int64)
    running = np.ones(G, bool)
    # one stream per match, handed from the side that just searched to the side that searches next
    holder = np.where(enemy_turn == 0, 1, 0)                        # the side that moves first holds the stream
    for i in range(G):
        sides[holder[i]].seed(i, (seed + i) & 0xFFFFFFFF)

    def take_stream(side, mask):
        for i in np.nonzero(mask)[0]:
            if holder[i] != side:                                    # another side drew last: take the stream over
                mt, pos, hg, gs = sides[holder[i]].get_rng_state(int(i))
                sides[side].set_rng_state(int(i), mt, pos, hg, gs)
                holder[i] = side

    ply = 0
    while running.any():
        turn = ply % 2
        for side in (0, 1):                                          # 0 player, 1 enemy
            mask = running & ((enemy_turn == turn) == (side == 1))
            if not mask.any():
                continue
            m8 = mask.astype(np.uint8)
            take_stream(side, mask)
            pi = sides[side].search(ids, m8)
            if side == 0 and monitor is not None:
                take_stream(2, mask)
                monitor.search(ids, m8)
            for i in np.nonzero(mask)[0]:
                a = int(np.argmax(pi[i]))                            # argmax_onehot of a one-hot: no draw (utils.py:198-205)
                ids[i] = ids[i] + (a,)
                wins[i] = utils.check_win(utils.get_board(ids[i], board_size), win_mark)
                if wins[i] != 0 or (max_plies and len(ids[i]) - 1 >= max_plies):
                    running[i] = False
        ply += 1
    last_search_totals.clear()
    last_proof_moves.clear()
    for k, sd in enumerate(sides):
        if isinstance(sd, _ZeroSide) and sd.proof_moves:
            last_proof_moves[k] = sd.eng.proof_move_stats()
    for sd in sides:
        if isinstance(sd, _ZeroSide):                                # what early stop saved, over both sides (tools/time_early_stop.py)
            ran = sd.eng.sims_run()
            for k, v in (('searches', sd.searches), ('simulations', sd.searches * sd.sims), ('settled', ran['settled_total']),
                         ('saved', ran['saved_total'])):
                last_search_totals[k] = last_search_totals.get(k, 0) + int(v)
        sd.close()
    result = {'Player': 0, 'Enemy': 0, 'Draw': 0}
    games = []
    for i in range(G):
        w = int(wins[i])
        games.append((w, list(ids[i][1:])))
        if w == 3 or w == 0:
            result['Draw'] += 1
            pw = ew = 0.5
        elif (w == 1) == (enemy_turn[i] == 1):
            result['Player'] += 1
            pw, ew = 1.0, 0.0
        else:
            result['Enemy'] += 1
            pw, ew = 0.0, 1.0
        player_elo, enemy_elo = elo(player_elo, enemy_elo, pw, ew)
    return result, (player_elo, enemy_elo), games


def tactical_summary(games, board_size, win_mark=None, device=0):
    """What the games of an evaluation say about tactics, beyond who won: `games` is the [(win_index, moves)] list of
    evaluate(..., return_games=True) / evaluate_batched, audited in ONE PositionBatch.audit call (every ply of every game
    on the device). Returns {'black': {...}, 'white': {...}} by the ply parity of the flags, each with plies, wins_available,
    wins_missed, single_threats, blocks_missed, lost_positions (the definitions of utils.audit_moves)."""
    from . import positions as P
    records = [list(moves) for _, moves in games]
    with P.PositionBatch(board_size, win_mark=win_mark, capacity=max(1, min(len(records), 4096)), device=device) as pb:
        d = pb.audit(records, leading_zero=False)
    if d["err"].any():
        raise ValueError("games %s are not legal move lists" % np.flatnonzero(d["err"]).tolist())
    out = {}
    for colour, name in enumerate(("black", "white")):
        f = d["flags"][:, colour::2].astype(np.int64)
        plies = ((d["counts"][:, 0].astype(np.int64) + 1 - colour) // 2).sum()    # black has the even plies of the audited ones
        avail, taken = (f & P.WIN_AVAILABLE) != 0, (f & P.WIN_TAKEN) != 0
        threat, blocked, lost = (f & P.THREAT) != 0, (f & P.BLOCKED) != 0, (f & P.LOST) != 0
        out[name] = dict(plies=int(plies), wins_available=int(avail.sum()), wins_missed=int((avail & ~taken).sum()),
                         single_threats=int((threat & ~lost).sum()), blocks_missed=int((threat & ~lost & ~blocked).sum()),
                         lost_positions=int(lost.sum()))
    return out


def forced_win_summary(games, board_size, max_depth=8, max_nodes=2000, win_mark=None, device=0):
    """How the games of an evaluation dealt with forced wins by continuous fours: `games` as for tactical_summary; every
    prefix of every game before its end goes through ONE PositionBatch.forced_wins call. Returns {'black': {...}, 'white':
    {...}} by the side to move, each with plies (positions searched), forced_wins (result 1 with depth >= 2: a win in one
    is tactical_summary's business), followed (of those, the move played is one of `moves`), missed (the others) and
    unknown (the node budget ran out)."""
    from . import positions as P
    ids, played = [], []
    for _, moves in games:
        moves = [int(m) for m in moves]
        for t in range(len(moves)):
            ids.append(moves[:t])
            played.append(moves[t])
    with P.PositionBatch(board_size, win_mark=win_mark, capacity=max(1, min(len(ids), 4096)), device=device) as pb:
        d = pb.forced_wins(ids, max_depth, max_nodes, leading_zero=False)
    if d["err"].any():
        raise ValueError("games hold moves that are not legal (prefixes %s)" % np.flatnonzero(d["err"]).tolist()[:8])
    played = np.array(played, np.int64).reshape(len(ids))
    open_ = d["status"] == 0                                              # (moves after the end of a game are not plies)
    forced = open_ & (d["result"] == P.FW_WIN) & (d["depth"] >= 2)
    followed = forced & (d["moves"][np.arange(len(ids)), played] != 0) if len(ids) else forced
    out = {}
    for colour, name in enumerate(("black", "white")):
        side = d["turn"] == colour
        out[name] = dict(plies=int((open_ & side).sum()), forced_wins=int((forced & side).sum()),
                         followed=int((followed & side).sum()), missed=int((forced & ~followed & side).sum()),
                         unknown=int((open_ & side & (d["result"] == P.FW_UNKNOWN)).sum()))
    return out


def forced_defence_summary(games, board_size, max_depth=8, max_nodes=2000, win_mark=None, device=0):
    """How the games of an evaluation dealt with the OPPONENT's forced wins by continuous fours: `games` as for
    tactical_summary; every prefix of every game before its end goes through ONE PositionBatch.forced_defences call.
    Returns {'black': {...}, 'white': {...}} by the side to move, each with plies (positions searched), threats (the
    opponent would have a forced win after a pass, threat 1 with threat_depth >= 2: a threat in one is tactical_summary's
    business), threat_unknown (that search ran out of nodes), and the threats by the move played: defended (its reply is
    SAFE), blundered (LOSES although a SAFE cell existed), hopeless (LOSES with no SAFE and no UNKNOWN cell) and unknown
    (the rest)."""
    from . import positions as P
    ids, played = [], []
    for _, moves in games:
        moves = [int(m) for m in moves]
        for t in range(len(moves)):
            ids.append(moves[:t])
            played.append(moves[t])
    with P.PositionBatch(board_size, win_mark=win_mark, capacity=max(1, min(len(ids), 4096)), device=device) as pb:
        d = pb.forced_defences(ids, max_depth, max_nodes, leading_zero=False)
    if d["err"].any():
        raise ValueError("games hold moves that are not legal (prefixes %s)" % np.flatnonzero(d["err"]).tolist()[:8])
    played = np.array(played, np.int64).reshape(len(ids))
    open_ = d["status"] == 0                                              # (moves after the end of a game are not plies)
    threat = open_ & (d["threat"] == P.FW_WIN) & (d["threat_depth"] >= 2)
    reply = d["reply"][np.arange(len(ids)), played] if len(ids) else np.zeros(0, np.uint8)
    n_safe, n_unknown = d["counts"][:, 1], d["counts"][:, 3]
    defended = threat & (reply == P.FD_SAFE)
    blundered = threat & (reply == P.FD_LOSES) & (n_safe > 0)
    hopeless = threat & (reply == P.FD_LOSES) & (n_safe == 0) & (n_unknown == 0)
    out = {}
    for colour, name in enumerate(("black", "white")):
        side = d["turn"] == colour
        out[name] = dict(plies=int((open_ & side).sum()), threats=int((threat & side).sum()),
                         threat_unknown=int((open_ & side & (d["threat"] == P.FW_UNKNOWN)).sum()),
                         defended=int((defended & side).sum()), blundered=int((blundered & side).sum()),
                         hopeless=int((hopeless & side).sum()),
                         unknown=int((threat & ~defended & ~blundered & ~hopeless & side).sum()))
    return out
