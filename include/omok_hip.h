/*
 * omok_hip.h -- C ABI of libomok_hip.so, the MI355X-native AlphaZero self-play engine for Omok.
 *
 * The reference (reinforcement-learning-kr/alpha_omok) is pure Python and has no FFI; this is
 * the boundary a maintainer binds with ctypes. Each entry point names the
 * reference interface it replaces (paths relative to /root/reference/2_AlphaOmok/).
 *
 * Conventions: every function returns 0 on success, non-zero on failure (ao_last_error() gives
 * the message). Buffers are caller-owned. "dev" pointers are HIP device pointers on the handle's
 * device (e.g. torch.Tensor.data_ptr()); "host" pointers are ordinary memory. A handle is not
 * thread-safe; all its work is queued on one HIP stream (ao_stream()).
 *
 * A handle owns G concurrent games. Game g has: its move list (the reference's node id without
 * the leading 0), its search tree (structure-of-arrays arena in HBM), and its own numpy-legacy
 * MT19937 stream (the reference's process-global np.random, main.py:60, one per game here).
 */
#ifndef OMOK_HIP_H
#define OMOK_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AO_ABI_VERSION 2   /* 2: ao_config.arena_fraction (round 6); entry points added since (ao_roll_*) change no existing layout */

typedef struct ao_engine ao_engine; /* search engine: G games                       */
typedef struct ao_net ao_net;       /* policy/value ResNet (model.py PVNet) weights  */

typedef struct ao_config {
    int32_t board;      /* board edge: 3, 9 (env_small.py:18) or 15 (env_regular.py), any 3..15 */
    int32_t win_mark;   /* 0 = reference rule: 3 if board == 3 else 5 (agents.py:46); 1..5, or above
                           the board size (no line wins: only the full board ends a game)            */
    int32_t sims;       /* num_mcts (agents.py:43; main.py:27 N_MCTS = 400)                    */
    int32_t inplanes;   /* IN_PLANES = 2*history+1 (main.py:34); 3, 5, 7 or 9                  */
    int32_t games;      /* G concurrent games (1 for a drop-in ZeroAgent)                      */
    int32_t noise;      /* Dirichlet root noise on/off (agents.py:40,49)                       */
    int32_t node_cap;   /* expanded-node capacity of one game's arena; 0 = default: 16*(sims+1), bounded by 40 % of
                           the device's TOTAL memory for all games' arenas and never below 4*(sims+1) -- a deterministic
                           number per device model; -1 = grow into the HBM that is free now (a quarter of it, at most
                           16*(sims+1)); see ao_trim_stats, ao_node_cap                                       */
    int32_t device;     /* HIP device ordinal                                                  */
    double  c_puct;     /* 0 = 5 (agents.py:48)                                                */
    double  alpha;      /* 0 = 10/board^2 (agents.py:47)                                       */
    double  arena_fraction; /* node_cap == 0 only: the share of the device's TOTAL memory the default rule may give the two
                           arenas of all games; 0 = 0.40 (main.py's over-subscribed engines ask for 0.50); (0, 0.90]. The
                           default path keeps its shrink-on-allocation-failure retry and its clamps (ABI version 2)   */
} ao_config;

/* root status reported by ao_set_root / ao_begin_move (agents.py:82-111) */
enum { AO_ROOT_FRESH = 0,       /* id not in the tree: num_mcts+1 simulations                  */
       AO_ROOT_UNEXPANDED = 1,  /* id known (n == 0, no children): num_mcts simulations        */
       AO_ROOT_EXPANDED = 2 };  /* id known and expanded: children re-noised, num_mcts sims    */

const char *ao_version(void);
int         ao_abi_version(void);

/* ---- engine lifetime ---- replaces ZeroAgent.__init__ (agents.py:40-53) */
int  ao_create(const ao_config *cfg, ao_engine **out);
void ao_destroy(ao_engine *e);
const char *ao_last_error(const ao_engine *e);   /* e may be NULL: error of the failed ao_create */
void *ao_stream(ao_engine *e);                   /* hipStream_t all engine work is queued on     */
int  ao_sync(ao_engine *e);                      /* hipStreamSynchronize                          */
/* Queue all further engine work on `stream` (a hipStream_t, e.g. torch's current stream) so an
 * external evaluator running on that stream needs no extra synchronisation. NULL restores the
 * engine's own stream. */
int  ao_set_stream(ao_engine *e, void *stream);

/* ---- per-game RNG ---- replaces np.random.seed / get_state / set_state (main.py:60).
 * ao_seed == np.random.seed(seed) for game g (MT19937 init_genrand, pos 624, no cached gauss). */
int ao_seed(ao_engine *e, int game, uint32_t seed);
int ao_seed_all(ao_engine *e, const uint32_t *host_seeds /*[G]*/);
/* ao_seed for the n listed games with ONE synchronisation (the refill of finished self-play slots: main.py:248 + np.random.seed per episode) */
int ao_seed_games(ao_engine *e, const int32_t *host_games, const uint32_t *host_seeds, int32_t n);
int ao_get_rng_state(ao_engine *e, int game, uint32_t *host_mt /*[624]*/, int32_t *pos,
                     int32_t *has_gauss, double *gauss);
int ao_set_rng_state(ao_engine *e, int game, const uint32_t *host_mt, int32_t pos,
                     int32_t has_gauss, double gauss);

/* ---- leaf symmetries ---- (opt-in; off, every result is bit for bit what it is without these calls)
 * With the switch on, every leaf goes through the network under one of the eight symmetries of the square, drawn per leaf
 * as AlphaGo Zero does: the planes are written into the evaluation batch as sym_planes(planes, s) and the policy row comes
 * back through the same map (sym_policy_back), the value as it is. Symmetry s = 2*r + f is rot90 by r, then a flip if f --
 * the numbering of utils.augment_dataset and of the replay ring; s = 0 is the identity. s is a stateless function
 *   s = leaf_symmetry(key_g, ply, sim)       (csrc/symmetry.hpp; alpha_omok_amd/utils.py has the same function)
 * of the game's key, the number of stones on the leaf's board and the game's 0-based simulation index inside the current
 * move. Nothing else changes: not the games' MT19937 streams, not the noise, not the selection; a terminal leaf uses up a
 * simulation index and is not evaluated, as before. It holds for every forward mode, precision and batch plan, for the
 * step-wise protocol (ao_collect_leaves hands out the planes already transformed; ao_apply_evals takes the network's rows
 * as they are) and for the rolling search.
 *   key_g = leaf_key(base_key, seed_g) = base_key ^ (seed_g * 0xC2B2AE35), seed_g the seed most recently given to game g by
 * ao_seed / ao_seed_all / ao_seed_games (never seeded: g). The engine remembers the seeds: an episode's symmetries are a
 * function of its seed and the base key alone, in any slot, under carry-over and under rolling refills. enable == 0
 * switches off (base_key is ignored). ao_set_leaf_symmetry_keys sets the keys of the n listed games directly, for callers
 * that hand streams around with ao_set_rng_state; it needs the switch on, and a later seed call or ao_set_leaf_symmetry
 * replaces what it set.
 * Both fail inside a move (between ao_begin_move and ao_end_move) and, while a roll is open, for a game that is in a move
 * of the roll -- where ao_seed_games fails (ao_set_leaf_symmetry touches every game).
 * What does NOT carry the keys: tree snapshots (ao_tree_export) -- to resume bit for bit the importer sets the same base
 * key and seeds; ao_get_rng_state. ao_set_eval_log records the evaluation batch's rows as they are, in the NETWORK's frame:
 * a replay brings the policy back with the leaf's symmetry. */
int ao_set_leaf_symmetry(ao_engine *e, int enable, uint32_t base_key);
int ao_set_leaf_symmetry_keys(ao_engine *e, const int32_t *host_games, const uint32_t *host_keys, int32_t n);

/* ---- leaf tactics ---- (opt-in; no reference counterpart; off, every result is bit for bit what it is without these calls)
 * With the switch on, the forced-win solver of ao_positions_forced_wins (continuous fours, utils.forced_win) runs on every
 * leaf the search expands -- a fresh root included -- for the side to move there, and its PROOF overrides the value:
 *   leaf_tactics_value(moves, value) = 1.0f   if forced_win(moves, board, win_mark, max_depth, max_nodes).result == FW_WIN
 *                                      value  otherwise: FW_NONE, FW_UNKNOWN (the node budget ran out), a terminal position
 * (alpha_omok_amd/utils.py: leaf_tactics_value, leaf_tactics_evaluator). The value is the leaf mover's own (agents.py:223-239
 * backs up -value into the leaf's record), so a forced win for the side to move is +1. Nothing else changes: not the policy
 * row, the noise, the selection, the MT19937 streams or the terminal leaves -- a search with leaf tactics is the reference
 * search under the evaluator f(moves, planes, sim) = (p, leaf_tactics_value(moves, v)) with (p, v) the plain evaluation, and
 * that is all it is. The opponent's threats (a leaf that is proven LOST) are not looked for, and the network still evaluates
 * a proven leaf: its priors are needed.
 * max_depth 1..16, max_nodes 1..1024 (checked before the device is touched); max_depth == 0 switches off (max_nodes is
 * ignored). win_mark must be 3..5 and at most the board size. Fails inside a move and, while a roll is open, if any game is in
 * a move of the roll (the rules of ao_set_leaf_symmetry). It holds for ao_search*, the rolling search and the step-wise protocol
 * (ao_apply_evals reads the caller's values, which stay untouched, and expands from a copy), combines with leaf symmetries,
 * budgets, early stop, the root bar, over-subscription and every forward mode and precision; the fp16-range repeat searches its
 * move again under the same switch (the counters then count both runs). With the switch on the fused per-game step is not
 * planned (a handful of games pay the unfused launch sequence). Tree snapshots do not carry the switch. In ao_search* and the
 * roll the solver runs on a stream of the engine's own beside the network launch; the environment variable
 * AO_LEAF_TACTICS_SERIAL (read by every search) queues it on the engine's stream behind the network instead: the same bits.
 * ao_leaf_tactics_stats: out[4] = leaves searched, proven, searches that ran out of max_nodes, solver nodes, summed over the
 * games since the last reset (or since the switch first went on); per_game [G][4] the same per game, or NULL; reset != 0 zeroes
 * the counters afterwards. The per-game counters are int32. Synchronises. */
int ao_set_leaf_tactics(ao_engine *e, int32_t max_depth, int32_t max_nodes);
int ao_leaf_tactics_stats(ao_engine *e, int64_t out[4], int32_t *host_per_game, int reset);

/* ---- game / tree state ---- */
/* ZeroAgent.reset() (agents.py:55-58) for the games with mask[g] != 0 (NULL = all): clears the
 * tree and the move list (root id becomes (0,)). */
int ao_reset(ao_engine *e, const uint8_t *host_mask);
/* The root_id argument of ZeroAgent.get_pi (agents.py:60,82-84): moves = root_id[1:].
 * Re-roots the tree kept from the previous search if the new id extends the previous root id and
 * the node exists (tree reuse); otherwise the game starts a fresh tree. The engine keeps the
 * subtree of the last root only (what main.self_play / eval_main.del_parents ever revisit). */
int ao_set_root(ao_engine *e, int game, const int32_t *host_moves, int32_t n, int32_t *status);
/* The same for every game with mask[g] != 0 (NULL = all) in ONE launch: moves[g * stride .. + n[g]) is game g's
 * root_id[1:]; status[g] receives AO_ROOT_* (entries of unmasked games are left alone). This is the call pattern of
 * eval_main.Evaluator.get_action (eval_main.py:137-151, 243-252) for G concurrent matches: after the opponent's
 * reply every match's id has grown by two plies that this engine did not choose. */
int ao_set_roots(ao_engine *e, const uint8_t *host_mask, const int32_t *host_moves, int32_t stride,
                 const int32_t *host_n, int32_t *host_status);

/* ---- one move decision, stepwise (external evaluator) ---- replaces _init_mcts/_mcts
 * (agents.py:82-132). Protocol per move:
 *     ao_begin_move -> repeat ao_sims_left() times { ao_collect_leaves -> evaluate ->
 *     ao_apply_evals } -> ao_end_move
 * active[g] == 0 leaves game g untouched for this move (NULL = all games active). */
int ao_begin_move(ao_engine *e, const uint8_t *host_active);
/* ao_begin_move with a budget and a noise switch per game (no reference counterpart). host_sims int32 [G]: simulations of
 * game g in this move, 1 .. ao_config.sims (the arena, the descent bounds and the catch-up loop were sized by it); a fresh
 * root still gets one more, its own expansion. A game's search is strictly sequential, so a budget-k search is the first k
 * simulations of the full one from the same stream. host_noise uint8 [G]: 0 on an engine created with noise means that
 * for this game and this move there is no Dirichlet draw, the root is not re-noised and the game's MT19937 stream is not
 * touched -- what an engine created without noise does; 1 on an engine created without noise is an error. NULL = the
 * engine's configuration, for either array. A value out of range is an error that names the game; nothing has been
 * changed by then and the engine stays usable. Values of inactive games are not looked at. */
int ao_begin_move_opts(ao_engine *e, const uint8_t *host_active, const int32_t *host_sims, const uint8_t *host_noise);
/* Launches the step-wise protocol still has to run: the largest number of simulations any active game owes. Lowered by
 * ao_settle. ao_end_move's precondition is stated in these terms: every active game has done == target, which the step-wise
 * protocol reaches after exactly this many ao_collect_leaves / ao_apply_evals pairs; a game that is not there gets the error
 * word ERR_SHORT from k_end_move and the call fails (see ao_end_move). The rolling search (ao_roll_run) relies on the same
 * rule from the other side: it turns a game only when it has read done == target for it. */
int ao_sims_left(ao_engine *e);
/* Settling: lower the simulation targets of games whose move is decided, or of every masked game at once. Legal between
 * ao_begin_move and ao_end_move only. For an active game let r = target - done be the simulations it owes, pending = 1 if
 * a leaf was selected (ao_collect_leaves) and not yet backed up (ao_apply_evals), and n1 >= n2 the two largest visit
 * counts among the root's children (n2 = 0 with one child). The game is DECIDED iff its root is expanded and
 * n1 - n2 > r -- utils.move_decided(visits, remaining) in the Python package is this rule: every owed simulation adds one
 * visit to one root child, so the leader stays the only maximum and ao_end_move's tau == 0 result is the full search's.
 * A game with host_mask[g] != 0 (NULL = every game) that is decided, or any such game when stop_now != 0, gets
 * target = done + pending: the pending leaf is still backed up, nothing else runs. Finished, inactive and unmasked games
 * are left alone. Synchronises; ao_sims_left then reports the largest number still owed and *unfinished (may be NULL) the
 * number of active games that owe anything. stop_now is how a caller ends a move early and still gets a pi from
 * ao_end_move (see there); a game stopped before its root has a visit returns numpy's 0/0 = NaN there. */
int ao_settle(ao_engine *e, const uint8_t *host_mask, int stop_now, int32_t *unfinished);
/* _selection (agents.py:134-168) for every game with simulations left, + get_state_pt of the
 * leaf (utils.py:139-168). dev_planes_nchw: optional float32 [G][C][B][B] (the layout
 * Agent.model expects, agents.py:175); NULL if only the engine's own network is used. */
int ao_collect_leaves(ao_engine *e, float *dev_planes_nchw);
/* _expansion_evaluation + _backup (agents.py:170-239) with the evaluator's outputs:
 * dev_policy float32 [G][A] (softmax probabilities), dev_value float32 [G]. Rows of games whose
 * leaf was terminal (or that are inactive) are ignored. */
int ao_apply_evals(ao_engine *e, const float *dev_policy, const float *dev_value);
/* Tail of get_pi (agents.py:64-80): visit, policy (post-noise priors of the root children) and
 * pi = visit/visit.sum(), one-hot through utils.argmax_onehot where tau[g] == 0.
 * Outputs are host float64 [G][A]; any may be NULL. host_tau int8 [G] (NULL = all 1).
 * Precondition: every active game has run exactly its target (done == target). A game that is short -- a caller that
 * ends the move early -- makes the call fail with "search ended after d of t simulations" (no pi is built from fewer
 * visits than asked for, the game's stream is not touched) and ends the move. The way to stop early is ao_settle with
 * stop_now: it lowers the targets to what has been run. After a failed call the visits made so far stay in the tree: a
 * retried move (ao_begin_move again) searches on top of them. */
int ao_end_move(ao_engine *e, const int8_t *host_tau, double *host_pi, double *host_visit,
                double *host_policy);
/* utils.get_action (utils.py:189-195) on game g's stream + env step (env_small.py:154-176,196)
 * + re-rooting on the chosen child, for all active games. host_action int32 [G],
 * host_win int32 [G] (0 playing, 1 black, 2 white, 3 draw). Games that ended keep their final
 * position until ao_reset. Must follow ao_end_move. */
int ao_play(ao_engine *e, int32_t *host_action, int32_t *host_win);

/* ---- one move decision, fused (native network) ---- ZeroAgent.get_pi with Agent.model = net.
 * Runs begin_move, all simulations (select -> PVNet forward -> expand/backup on one stream) and
 * end_move. */
int ao_search(ao_engine *e, ao_net *net, const uint8_t *host_active, const int8_t *host_tau,
              double *host_pi, double *host_visit, double *host_policy);
/* ao_search with the per-game budgets and noise switches of ao_begin_move_opts (host_sims, host_noise; NULL = the engine's
 * configuration) and with settling: every settle_every simulations, and in every catch-up round of an over-subscribed
 * search, the games with host_early_stop[g] != 0 whose move is decided (ao_settle's rule) get their targets lowered, the
 * loop reads four counters back (a stream synchronisation) and goes on with the largest number of simulations still owed,
 * or ends. host_early_stop NULL or settle_every 0: nothing is launched or read, the loop is ao_search's. The budgets hold
 * in every regime of the search (the fused few-game step, rows packed per move, rows handed out per simulation) and for
 * the move that the fp16-range recovery repeats. An early-stopped search returns the pi and the move of the full one for
 * tau == 0 games and hands a smaller tree to the next move. */
int ao_search_opts(ao_engine *e, ao_net *net, const uint8_t *host_active, const int8_t *host_tau, const int32_t *host_sims,
                   const uint8_t *host_noise, const uint8_t *host_early_stop, int32_t settle_every, double *host_pi,
                   double *host_visit, double *host_policy);
/* The last move of the engine (either protocol), readable until the next one begins: host_sims_run int32 [G] simulations
 * run per game in budget units (a fresh root's own expansion not counted; 0 for inactive games), host_settled uint8 [G]
 * 1 where settling lowered the game's target; and the engine's running totals of games settled and simulations saved.
 * Any pointer may be NULL. */
int ao_search_sims(ao_engine *e, int32_t *host_sims_run, uint8_t *host_settled, int64_t *settled_total, int64_t *saved_total);

/* ---- rolling search (no reference counterpart) ---- every game moves on its own clock inside one launch loop.
 * ao_search searches one move of every game per call: its loop lasts until the LAST game has its simulations, then all games
 * end the move, play and begin the next one together. A ROLL keeps the launch loop running (select | net | expand + select |
 * net | ..., always on the rows-per-simulation path, the batch bounded by ao_set_row_cap) and every turn_every launches TURNS
 * the games that have their simulations: end of move, play, re-root, and the begin of the game's next move, for a compact
 * list of games, in O(listed games) work and host traffic; the other games are mid-search in the same launches. A game's
 * search stays strictly sequential, so each record is, to the bit, what ao_search_opts + ao_play return for that game's ply
 * from the same stream, budget and noise switch (pi, visit, policy, action, win, and the stream afterwards).
 * Protocol: ao_roll_begin -> repeat ao_roll_run (records come back as games turn; refill finished slots with ao_reset(mask),
 * ao_seed_games, ao_roll_join) -> ao_roll_drain -> ao_roll_run until nothing is in a move -> ao_roll_end.
 * Inside an open roll ao_begin_move*, ao_search*, ao_end_move, ao_play, ao_settle, ao_collect_leaves, ao_apply_evals,
 * ao_set_root(s), ao_set_root_bar, ao_set_row_cap, ao_set_eval_log, ao_tree_export, ao_tree_import, ao_root_tactics and
 * ao_roll_set_tactics fail with a message that says a roll is open (the forced-win solver combines with a roll through
 * ao_roll_set_tactics, called BEFORE ao_roll_begin: see below; the caller's own masks, the fp16-range repeat and a torch-module
 * evaluator do not); ao_reset, ao_seed*, ao_set_rng_state fail, naming the game, for a game that is in
 * a move, and work for the others. The tree read-outs (ao_tree_lookup, ao_tree_pv, ao_tree_stats, ao_get_root_children)
 * stay legal between ao_roll_run calls; ao_destroy is legal at any time. ao_search_sims' totals, ao_row_stats,
 * ao_trim_stats and ao_search_stats keep counting. */
typedef struct ao_roll_opts {
    const uint8_t *active;     /* [G] the games that begin a move; NULL = every game that is not over                        */
    const int32_t *tau_plies;  /* [G] tau = 1 while ply < tau_plies[g] (ply: moves on the board), else 0; NULL = tau 1 always */
    const int32_t *sims;       /* [G][sims_stride] budget by ply: column min(ply, sims_stride - 1); NULL = ao_config.sims     */
    int32_t sims_stride;
    const uint8_t *noise;      /* [G][noise_stride] noise switch by ply, looked up the same way; NULL = the engine's          */
    int32_t noise_stride;
    int32_t early_stop;        /* != 0: a look (ao_settle's rule, pending leaf counted) settles decided tau == 0 moves         */
    int32_t turn_every;        /* >= 1: launches between two turns                                                            */
    int32_t want_visit;        /* != 0: the records carry visit / policy                                                      */
    int32_t want_policy;
} ao_roll_opts;
/* Records of one ao_roll_run, caller-owned arrays of capacity G (a game turns at most once per turn): entry b < count is
 * game[b]'s move at ply[b] (moves on the board before it): action, win (0 playing, 1 black, 2 white, 3 draw), the tau it
 * was decided with, sims = simulations run in budget units (done - bonus, as ao_search_sims reports them), settled = 1
 * where a look lowered its target, pi [b][A], and visit / policy [b][A] where asked for (either may be NULL). */
typedef struct ao_roll_records {
    int32_t count;
    int32_t *game, *ply, *action, *win, *tau, *sims, *settled;
    double *pi, *visit, *policy;
} ao_roll_records;
/* Opens a roll on `net`: begins a move for every listed game and queues the first selection. Refused, with nothing touched:
 * inside a move or an open roll, with a pending root bar, with an eval log set, on a network that does not fit the engine,
 * turn_every < 1, or a budget outside 1..ao_config.sims / a noise switch on an engine without noise anywhere in a listed
 * game's table rows (the message names the game). */
int ao_roll_begin(ao_engine *e, ao_net *net, const ao_roll_opts *opts);
/* Runs the loop until a turn has produced at least one record, nothing is in a move, or max_launches launches of this call
 * are spent (0 = no bound). out->count may be 0. A game whose record has win != 0 is over and takes no further part; every
 * other turned game is already searching its next move, unless the roll is draining. Order of steps with early_stop, per
 * period of turn_every launches: turn_every - 1 launches, the look, one launch (it backs up the leaf a settled game still had
 * under way), the turn. At every turn the network's status word and the games' error words are read BEFORE any game is
 * turned: AO_NET_FP16_RANGE fails the call with a message that names it (there is no transparent repeat on the fp32-MFMA
 * trunk under rolling), a per-game error fails it as ao_end_move / ao_play would; either way no game is turned in that turn,
 * the error words are cleared, the roll is closed and the engine is outside any move. */
int ao_roll_run(ao_engine *e, int64_t max_launches, ao_roll_records *out);
/* Games that are not in a move (listed in opts->active; NULL = all that are not over) begin one and join the running loop;
 * only the per-game fields of opts are read (tau_plies, the sims / noise rows; strides as at ao_roll_begin) and replace the
 * listed games' rows. Typical: a slot refilled by ao_reset(mask) + ao_seed_games. A listed game that is in a move is refused. */
int ao_roll_join(ao_engine *e, const ao_roll_opts *opts);
/* From now on no turned game begins another move; ao_roll_run keeps returning records until nothing is in a move. */
int ao_roll_drain(ao_engine *e);
/* Closes the roll. Refused, naming how many games are affected, while any game is in a move. Afterwards the engine is
 * exactly between moves, as after ao_play: moves, root status, over flags, streams and the Gaussian cache of the host
 * draws; ao_search, ao_tree_export, ao_set_roots and the rest work again. */
int ao_roll_end(ao_engine *e);
/* Host traffic of the turns: turns taken, games turned, bytes copied between host and device by turns, looks and begins
 * since the engine was created, and the games / bytes of the LAST turn. Every copy a turn makes is counted. A turn's bytes
 * are 16 per game of the engine (the four words it decides from: simulations done, target, leaf status, error word) plus a
 * few KB per game it turns; the turned games' error words come back in their records -- never a second [G]-wide read, and
 * never a [G]-wide copy of pi, visit, policy or the streams. */
int ao_roll_stats(ao_engine *e, int64_t *turns, int64_t *games_turned, int64_t *bytes, int64_t *last_games, int64_t *last_bytes);
/* ---- the forced-win solver beside the rolling loop ----
 * Arms the solver for the rolls opened AFTERWARDS: every move a game begins inside such a roll (at ao_roll_begin, at
 * ao_roll_join, after a turn) is begun as ao_root_tactics(apply = 1) + ao_search_opts begin it -- utils.root_tactics of the
 * game's root gives the bar of that one move, and a proven RT_WIN lowers the move's budget to min(budget, solved_sims)
 * (solved_sims == 0: no cap). The sentence above still holds: per game and ply a record is, to the bit, what
 * ao_root_tactics(apply = 1) + ao_search_opts + ao_play return from the same stream, budget and noise switch.
 * The solver does not run inside a turn (one call lasts as long as its slowest wavefront, tens of milliseconds at the
 * default limits): it runs in BATCHES on a second stream that touches nothing but the batch's own buffers. The games listed
 * at a turn WAIT for their batch -- they count as in a move for ao_reset / ao_seed* / ao_roll_join / ao_roll_end -- while all
 * others go on searching; every later turn asks, oldest batch first, whether its event has been reached and then begins its
 * games. A ring of four batches; the host waits (for the oldest batch's recorded event, once) only when a batch is to be
 * started and all four are busy, or when nothing is searching and a batch is pending. Nothing of a record depends on when
 * a verdict arrived. Draining starts no batch; ao_roll_run returns "nothing is in a move" only when no batch is pending.
 * AO_ROLL_TACTICS_HOLD=<k> (read at ao_roll_begin; a test knob) holds every finished batch for at least k further turns.
 * max_depth == 0 disarms: the roll's launches, arguments and host traffic are then exactly those without this call.
 * Refused: inside an open roll; limits outside 1..16 / 1..65536; solved_sims outside 0..ao_config.sims. With the solver armed
 * ao_roll_begin also refuses a win_mark outside 3..5 or above the board size (as ao_root_tactics does). A pending root bar
 * still refuses ao_roll_begin, and ao_root_tactics / ao_set_root_bar still fail inside a roll: the caller's own masks do not
 * combine with a roll. ao_roll_end (and every failure that closes a roll) leaves the engine so that the next synchronous
 * move clears the sentinels of barred root children, as a move after a barred move does. */
int ao_roll_set_tactics(ao_engine *e, int32_t max_depth, int32_t max_nodes, int32_t solved_sims, int32_t want_allowed);
/* Index-aligned with the records of the LAST ao_roll_run: entry b is what the solver said at the root of the move that
 * record b played (verdict AO RT_*: 0 none, 1 win, 2 defend, 3 lost; depth; nodes; unknown bits, as ao_root_tactics;
 * allowed [count][A], which needs want_allowed). Any pointer may be NULL. */
int ao_roll_tactics_records(ao_engine *e, int32_t *verdict, int32_t *depth, int32_t *nodes, int32_t *unknown, uint8_t *allowed);
/* out[6], since the roll was opened: batches started, games solved, turns that games spent waiting for a verdict (summed
 * over the games), times the host had to wait for a batch, solver nodes summed over the records, and bytes moved between host
 * and device for tactics (also counted in ao_roll_stats' bytes). */
int ao_roll_tactics_stats(ao_engine *e, int64_t *out);

/* ---- root move restriction ("the bar", no reference counterpart) ----
 * host_allowed uint8 [G][A]: 1 = the cell may be searched at game g's root in the NEXT ao_begin_move* / ao_search*; NULL
 * clears a pending bar. That call consumes the bar: the move after it is unrestricted again. Ones on occupied cells are
 * ignored; a row that allows every empty cell restricts nothing, and with no game restricted the move's launches are those
 * of an engine that never heard of bars. A row of an active game that allows none of its empty cells makes the
 * ao_begin_move* / ao_search* fail before it touches anything ("the root bar allows no empty cell"). Rows of inactive games
 * are not looked at. The pending bar of a game is dropped when its position changes: ao_play, ao_reset, ao_set_root(s),
 * ao_tree_import.
 * A barred root child is never selected in that move and gets no visit: its pi and visit entries are 0, its policy entry is
 * the prior as always. It is data in the root's record, the selection does not know about it: the child is written with
 * q = AO_BAR_Q, n = 0, w = 0 (ao_get_root_children shows exactly that), and on a root that had been searched before it
 * forgets its statistics and its subtree. A child that carries the sentinel and is allowed in a later move of the same
 * root is an unvisited child again. The move that the fp16-range recovery of ao_search repeats runs under the same bar. */
#define AO_BAR_Q (-1.0e30f)
int ao_set_root_bar(ao_engine *e, const uint8_t *host_allowed);
/* The forced-win solver (ao_positions_forced_wins / _forced_defences) on the engine's own root positions, read on the device:
 * utils.root_tactics of the Python package is the definition. For every game with host_active[g] != 0 (NULL = all) that has
 * not ended: verdict AO_RT_WIN if the mover has a forced win by continuous fours within max_depth (allowed = the winning
 * first moves, depth = its depth); else, if the opponent has one after a pass, every empty cell is tried as a reply and
 * allowed = the replies not proven to lose: AO_RT_DEFEND (depth = the threat's depth), or AO_RT_LOST with allowed = every
 * empty cell when all replies lose; else AO_RT_NONE with allowed = every empty cell. nodes = the sum over the searches the
 * definition runs, each bounded by max_nodes (1..65536; max_depth 1..16); unknown = bit 0 / 1 / 2 set where the mover's /
 * the opponent's / a reply's search ran out of nodes (a reply whose search ran out stays allowed). Inactive, ended and
 * terminal games get zeros. The engine's win_mark must be 3..5 and at most the board size. Outputs are host arrays, int32 [G]
 * and uint8 [G][A]; any may be NULL. apply != 0: the bar of the next move (ao_set_root_bar) is set ON THE DEVICE to a pending
 * bar of the caller's intersected with `allowed`, game by game; a game whose intersection holds no empty cell keeps the
 * caller's. Fails between ao_begin_move and ao_end_move. */
enum { AO_RT_NONE = 0, AO_RT_WIN = 1, AO_RT_DEFEND = 2, AO_RT_LOST = 3 };
int ao_root_tactics(ao_engine *e, const uint8_t *host_active, int32_t max_depth, int32_t max_nodes, int32_t apply,
                    int32_t *host_verdict, int32_t *host_depth, uint8_t *host_allowed, int32_t *host_nodes, int32_t *host_unknown);

/* ---- introspection (tests, get_visit/get_policy, del_parents prints) ---- */
int ao_get_moves(ao_engine *e, int game, int32_t *host_moves /*[A]*/, int32_t *n);
/* statistics of the root's children in stored child order: action, n, w, q, p */
int ao_get_root_children(ao_engine *e, int game, int32_t *host_action, double *host_n,
                         double *host_w, double *host_q, double *host_p, int32_t *count);
int ao_tree_nodes(ao_engine *e, int game, int64_t *expanded, int64_t *dict_entries);

/* ---- tree read-out on the device ---- the reference's `self.tree` is a public dict (agents.py:52); these three read the
 * trees where they live, for many games in one launch, and download O(result) bytes. All three are read-only: the search
 * that follows is bit for bit the search that would have run without them. All three fail, with nothing touched, between
 * ao_begin_move and ao_end_move and on a game index out of range. Each: one upload, one launch, one download and one
 * synchronisation (ao_tree_lookup: per chunk of 1024 queries). */
enum { AO_NODE_ABSENT = 0,     /* not a key of the kept subtree: off the tree, an occupied or off-board move, an id that does
                                  not extend the game's root, any id of a fresh game                                    */
       AO_NODE_LEAF = 1,       /* a key with n == 0: the entry agents.py:206-210 made when its parent was expanded      */
       AO_NODE_TERMINAL = 2,   /* a visited key whose position ends the game (never expanded, agents.py:216-221)        */
       AO_NODE_EXPANDED = 3 }; /* a key with children                                                                   */
/* self.tree[node_id] (agents.py:52,206-210) for n ids. Query i asks game games[i] for the FULL id
 * (0, moves[i * stride], ..., moves[i * stride + m[i] - 1]); an id that does not extend the game's root id is ABSENT, not an
 * error. Host outputs, any may be NULL; A = board * board:
 *   status       int32   [n]     AO_NODE_*
 *   node_nwqp    float64 [n][4]  the node's own n, w, q, p (w and q are float32 values, n an integer). The engine keeps them
 *                                on the PARENT's edge and the root has none: an expanded root gets n = 1 + the sum of its
 *                                children's n (exact: the simulation that expands a node visits no child) and NaN for w, q, p;
 *                                a root that is known but not expanded (AO_ROOT_UNEXPANDED) is a LEAF with four NaN; ABSENT: NaN
 *   nchild       int32   [n]     len(tree[id]['child']); 0 unless EXPANDED
 *   child_action int32   [n][A]  tree[id]['child'] in stored order; -1 in unused slots
 *   child_n      int32   [n][A]  tree[id + (a,)]['n'] in the same order; child_w / child_q float32, child_p float64; 0 in
 *                                unused slots */
int ao_tree_lookup(ao_engine *e, const int32_t *host_games, const int32_t *host_moves, int32_t stride, const int32_t *host_m,
                   int32_t n, int32_t *status, double *node_nwqp, int32_t *nchild, int32_t *child_action, int32_t *child_n,
                   float *child_w, float *child_q, double *child_p);
/* The principal variation of every game with mask[g] != 0 (NULL = all): from the root, the edge with the most visits -- the
 * arg-max of the visit vector agents.py:67-69 builds, applied again at the child --, the lowest stored index on a tie. The
 * line ends when the best n is 0, behind an edge whose child is not expanded, or after max_len (1..A) plies. Host outputs, any
 * may be NULL: action int32 [G][max_len], n int32 [G][max_len], q float32 [G][max_len] (the stored q of the edge), len int32
 * [G]. Entries beyond len[g] and the rows of unmasked games are left as they are. */
int ao_tree_pv(ao_engine *e, const uint8_t *host_mask, int32_t max_len, int32_t *action, int32_t *n, float *q, int32_t *len);
/* del_parents' prints (agents.py:241-250) for every game with mask[g] != 0 (NULL = all), from a breadth-first walk on the
 * device: out int32 [G][4] = { expanded nodes the root reaches, dict entries (1 + the sum of their child counts: the numbers
 * of ao_tree_nodes), tree depth (the longest key of the kept subtree minus one: the largest ply + (nchild > 0) over the
 * reachable expanded nodes; the root's ply if the root is only known; 0 without a tree), nodes_used (records the arena
 * holds: what exceeds the first number is dead until the next compaction) }. Rows of unmasked games are left as they are. */
int ao_tree_stats(ao_engine *e, const uint8_t *host_mask, int32_t *out);

/* ---- proven outcomes ---- (no reference counterpart; beside get_pi, agents.py:64-80) A visited child whose position ends the
 * game is stored as such, so a tree can hold a complete proof that its root is won, lost or drawn; backup only folds those facts
 * into w / q. ao_tree_proofs runs an exact minimax over what each masked game's root reaches (the walk of ao_tree_stats, then a
 * sweep over its ply levels from the deepest to the root) and is read-only like the other read-outs. The definition is
 * alpha_omok_amd/utils.py: tree_proofs. Every expanded node gets a status for its side to move and the plies to the end:
 *   edge of a node, seen from the node's mover:  a terminal child that wins for the mover (WIN, 1), that fills the board
 *   (DRAW, 1); an expanded child c: its status with WIN and LOSS swapped, plies[c] + 1; an unvisited child -- a barred root
 *   child is one -- UNKNOWN
 *   node:  any WIN edge -> (WIN, fewest plies); else any UNKNOWN edge -> UNKNOWN; else any DRAW edge -> (DRAW, fewest plies
 *   among the draws); else (LOSS, most plies). An expanded node owns an edge for every legal move.
 *   line:  from the root, while the node is proven, the first edge in stored order that carries the node's own status and plies;
 *   its length is the root's plies (cut at max_len) and it ends on a terminal edge.
 * Host outputs, any may be NULL; rows of unmasked games are left as they are; a masked game without an expanded root gets
 * zeros, -1 in child_status and an empty line:
 *   root         int32 [G][4]        status, plies, proven nodes, nodes walked
 *   child_status int8  [G][A]        AO_PROOF_* of the root's edge that plays the action, -1 where the root has no such edge
 *   child_plies  int16 [G][A]        its plies, 0 where unknown or no edge
 *   line         int32 [G][max_len]  the actions of the proof line, -1 beyond it;  line_len int32 [G]
 * max_len in 1..A. Fails, with nothing touched, between ao_begin_move and ao_end_move and while a roll is open. One upload, one
 * launch, one download, one synchronisation. The proofs feed nothing back into selection or backup. */
enum { AO_PROOF_UNKNOWN = 0, AO_PROOF_WIN = 1, AO_PROOF_LOSS = 2, AO_PROOF_DRAW = 3 };
int ao_tree_proofs(ao_engine *e, const uint8_t *host_mask, int32_t max_len, int32_t *root, int8_t *child_status,
                   int16_t *child_plies, int32_t *line, int32_t *line_len);
/* Proof moves (opt-in; off, no kernel of this section is launched and every result is what it is without these calls). With
 * the switch on, ao_end_move -- and so ao_search*, and the repeat of a move after an fp16-range event -- runs the proofs of
 * the active games behind k_end_move and rewrites pi on the device before it is copied out (utils.proof_pi):
 *   AO_PM_WIN     some root edge is WIN: pi is one-hot on the WIN edge with the fewest plies, ties to the larger visit count,
 *                 then to the lowest action
 *   AO_PM_PRUNED  no WIN edge, some edge is LOSS, some is not, and some LOSS edge has pi > 0: with s the sum of pi over the
 *                 edges that are not LOSS (sequential, ascending action, fp64), pi = pi / s there and 0 elsewhere; if s == 0 (a
 *   AO_PM_MOVED   tau == 0 one-hot on a lost move) pi is one-hot on the non-lost edge with the most visits, lowest action on ties
 *   AO_PM_NONE    everything else, a root proven LOSS included: pi is untouched, bit for bit
 * ao_play then draws from that pi, so the recorded pi is no longer pure visit counts. visit and policy are untouched, and the
 * games' MT19937 streams advance exactly as without the switch (the tau == 0 tie draw has happened before, ao_play draws its
 * one double either way). Inactive games keep their rows; a game short of its simulations gets AO_PM_NONE. ao_set_proof_moves
 * fails inside a move and while a roll is open; ao_roll_begin fails while the switch is on (the roll's turn does not know it).
 * Tree snapshots do not carry the switch.
 * ao_proof_move_records: verdict int32 [G] of each game's most recent ao_end_move under the switch (0 before any), totals
 * int64 [4] = moves that got NONE, WIN, PRUNED, MOVED since the last reset, over the active games of every ao_end_move under
 * the switch (a move that the fp16-range recovery repeats is ended once and counts once); either may be NULL; reset != 0 zeroes
 * the totals. */
enum { AO_PM_NONE = 0, AO_PM_WIN = 1, AO_PM_PRUNED = 2, AO_PM_MOVED = 3 };
int ao_set_proof_moves(ao_engine *e, int enable);
int ao_proof_move_records(ao_engine *e, int32_t *verdict, int64_t totals[4], int reset);

/* ---- tree snapshots ---- the reference's `self.tree` lives as long as its process and can be pickled like any dict
 * (agents.py:52); these move the engine's trees and streams out of an engine and back in. A snapshot is host data without
 * device pointers: what the root of each game reaches, breadth first with the root as node 0 (the numbering of a re-rooting),
 * the game's move list, root status and MT19937 stream. Positions are not stored: a node's position is its parent's plus one
 * move, and the import rebuilds it. A search resumed from a snapshot is bit for bit the search that never stopped. Per-move
 * buffers (the Dirichlet draw, pi / visit / policy) are not part of a snapshot: it captures trees and streams, not a move in
 * progress, and ao_play must follow a search on the importing engine as on a fresh one.
 * All arrays are caller-owned host memory. Games are stored one after the other: game i owns hdr[i][0] nodes and hdr[i][1]
 * edges, behind those of the games before it; a node's first edge follows from the running sum of nchild over its game. A
 * game packs to exactly 25 * edges + 12 * nodes bytes behind its fixed-size header row. */
enum { AO_SNAP_HDR = 8 };
typedef struct ao_tree_snapshot {
    int32_t board, inplanes, win_mark;   /* of the exporting engine; the importing engine must have the same              */
    int32_t sims, noise;                 /* of the exporting engine: information only                                      */
    int32_t games;                       /* games in the snapshot                                                          */
    double  c_puct;                      /* information only                                                               */
    int64_t nodes, edges;                /* lengths of the node / edge arrays. ao_tree_export reads them as the capacity of
                                            the caller's arrays and writes back what it used                              */
    int32_t  *hdr;          /* [games][8] nodes, edges, number of moves, AO_ROOT_* status, over (win index of a finished
                               game, else 0), MT19937 pos, has_gauss, 0                                                   */
    double   *gauss;        /* [games]      cached gaussian of the numpy-legacy stream                                    */
    uint32_t *mt;           /* [games][624] MT19937 state                                                                 */
    int32_t  *moves;        /* [games][A]   the root id without its leading 0 (ao_get_moves)                              */
    int32_t  *nchild;       /* [nodes]      edges of the node: 1 .. A - ply                                               */
    int32_t  *parent;       /* [nodes]      the node's parent, as a node number inside its game; -1 for the root          */
    int32_t  *parent_edge;  /* [nodes]      stored index of the edge of `parent` that leads here; -1 for the root         */
    uint8_t  *act;          /* [edges]      action of the edge, in stored child order; no padding                         */
    int32_t  *n;            /* [edges]                                                                                    */
    float    *w, *q;        /* [edges]                                                                                    */
    double   *p;            /* [edges]                                                                                    */
    int32_t  *child;        /* [edges]      the child's node number inside its game, -1 unvisited, -2 terminal            */
} ao_tree_snapshot;
/* Packs the games with mask[g] != 0 (NULL = all), in ascending game order, into the caller's arrays (size them with
 * ao_tree_stats: nodes = expanded, edges = dict entries - 1). One stats pass over the masked games, then one pack launch and
 * one download per chunk of games. The device workspace is the read-out workspace, grown on demand: a chunk is closed when
 * its packed games reach 64 MiB, so the workspace is bounded by 64 MiB plus one game's packed size (plus 16 bytes per game),
 * whatever node_cap is; nothing transferred scales with node_cap. Read-only on the trees: the search that follows is bit for
 * bit the search without the export. Fails, with nothing touched, between ao_begin_move and ao_end_move, when a capacity is
 * too small, and when the breadth-first queue of a node_cap arena does not fit the LDS of a workgroup (as ao_tree_stats). */
int ao_tree_export(ao_engine *e, const uint8_t *host_mask, ao_tree_snapshot *out);
/* Imports snapshot game i into slot host_games[i], i < n = snap->games (other games are untouched): node i becomes record i
 * of the game's current arena, the positions are rebuilt level by level, the stream, the move list, the root status and the
 * root position are restored. The destination may be another slot, another engine, or an engine with other `games`,
 * node_cap or sims; board, inplanes and win_mark must be the snapshot's. Refused with every game left as it was: a call
 * between ao_begin_move and ao_end_move, a game index out of range or listed twice, a snapshot that fails
 * ao_tree_snapshot_check (checked before anything is uploaded), and a game with more nodes than node_cap - sims - 1 (the
 * next move's expansions must fit; nothing is trimmed silently). An action that lands on an occupied cell when the positions
 * are rebuilt resets that game and fails the call; the other games of the call are imported. Trim and search counters keep
 * the importing engine's values. One upload and one launch per chunk of games (chunks as in ao_tree_export). */
int ao_tree_import(ao_engine *e, const int32_t *host_games, int32_t n, const ao_tree_snapshot *snap);
/* Consistency of a snapshot; needs no engine and no device. Per game: the sizes and running sums agree; 1 <= nchild <= A - ply;
 * actions are < A and distinct within a node; n >= 0, and >= 1 on an edge with an expanded or terminal child; w, q, p are
 * finite; every child is -1, -2 or a later node number; every node but the root is named by exactly one edge, the one its
 * parent / parent_edge name; child numbers increase in scan order (breadth first); 0 <= pos <= 624; moves are < A and
 * distinct. Non-zero on the first violation; ao_last_error(NULL) describes it. */
int ao_tree_snapshot_check(const ao_tree_snapshot *snap);

/* HIP-event timing of the per-simulation tree kernel of ao_search (k_expand_select: expansion + backup of one
 * simulation, selection + terminal test + plane encoding of the next -- agents.py:134-239 for every game), recorded
 * on the engine's launch stream. Returns the total and the number of TIMED launches since the previous call and
 * enables / disables the timing (bench.py's roofline_tree); enable = n > 1: every n-th launch carries the event pair. */
int ao_tree_timing(ao_engine *e, int enable, double *ms_total, int64_t *launches);
/* Arena pressure, cumulative since ao_create. A game's arena holds node_cap expanded nodes; the tree kept across
 * moves (main.py:171 -> agents.py:84) grows by up to `sims` nodes per move when the visits keep following the played
 * line. Re-rooting therefore keeps at most node_cap - sims - 1 nodes, breadth first: a child subtree beyond that
 * becomes an unvisited child again (its n / w / q are forgotten -- the one place the engine departs from the
 * reference's never-pruned dict, and only in games that hit the limit). subtrees_dropped / reroots_trimmed count the
 * events; both stay 0 while node_cap is large enough (raise ao_config.node_cap otherwise). */
int ao_trim_stats(ao_engine *e, int64_t *subtrees_dropped, int64_t *reroots_trimmed);
/* the arena capacity this engine runs with (ao_config.node_cap after defaults) and whether it was derived from the free
 * HBM at creation (node_cap = -1): what decides if agents.py's never-pruned dict (agents.py:52) is reproduced in full. */
int ao_node_cap(ao_engine *e, int32_t *node_cap, int32_t *from_free_memory);
/* Host threads this PROCESS uses for the per-move np.random.dirichlet replay (agents.py:97-98,194-195 need glibc log / pow,
 * so the draws of all games are made on the host at the start of a move): one persistent pool per process of
 * min(32, hardware threads / LOCAL_WORLD_SIZE) threads, the caller included (LOCAL_WORLD_SIZE as torchrun exports it: the
 * ranks of a node share the host; AO_HOST_THREADS overrides). Needs no device. */
int ao_host_threads(void);
/* ao_search repeats a move on the fp32-MFMA trunk when the split-fp16 trunk met an activation beyond the fp16 range
 * (ao_net_status): the games of that move get their pre-move streams back and fresh trees at their positions, the
 * caller gets the repeated move's result. Counted here since ao_create: moves repeated, games searched again. The
 * network returns to the mode ao_net_set_mode asked for after the repeated move; from the third such move with the SAME
 * weights (counted per ao_net since its last ao_net_finalize) it stays on the fp32-MFMA trunk -- ao_net_get_mode then says
 * 2 -- until new weights are finalized or ao_net_set_mode is called. */
int ao_fp16_range_events(ao_engine *e, int64_t *moves_repeated, int64_t *games_redone);
/* search-shape counters since the last ao_begin_move, summed over games: PUCT levels traversed,
 * k>1 random tie-breaks, terminal leaves, evaluated leaves */
int ao_search_stats(ao_engine *e, int64_t *levels, int64_t *ties, int64_t *terminal,
                    int64_t *evaluated);

/* Rows of the evaluation batch per simulation in ao_search (new; the reference evaluates one leaf at a time and runs the net on
 * terminal leaves only to throw the result away, agents.py:171-178,216-221 -- SURVEY Q9).
 *   rows == 0 (default): the host packs the active games to the front of the batch once per move; a game whose leaf is terminal
 *     keeps its (stale) row in that simulation's batch.
 *   rows > 0: the tree kernel hands out the rows PER SIMULATION -- terminal leaves take none -- and counts the live rows in a
 *     device word the trunk kernels read (groups without a live row exit at once). `rows` bounds the batch of one simulation; with
 *     MORE active games than rows (over-subscription, e.g. 5120 games on the 4096 rows the resident trunk fills the chip with)
 *     a share of the games sits out every launch in turn and a leaf that still finds the batch full is evaluated one launch
 *     later; ao_search runs until every game has its simulations. Every game's search stays strictly sequential: visits,
 *     priors, actions and RNG streams are bit-identical to rows == 0 for a network whose result does not depend on a board's
 *     neighbours in the batch. */
int ao_set_row_cap(ao_engine *e, int32_t rows);
/* since ao_create, over the ao_search calls that handed out rows per simulation: network launches, live rows they evaluated,
 * rows they were launched for (launches x batch capacity), leaves that found their simulation's batch full */
int ao_row_stats(ao_engine *e, int64_t *launches, int64_t *rows_live, int64_t *rows_launched, int64_t *waits);
/* Test / debugging hook: what the network returned to the listed games during ao_search. Network launch s (counted from 0
 * when this function was called, over all ao_search calls since) writes, for listed game k, a record of A + 3 floats to dev_log[(s * n + k) * (A + 3) ...]: the policy row
 * and the value at the game's row of the evaluation batch, the number of simulations the game has completed, and its leaf
 * status (1 / 2: the leaf waits for exactly this evaluation; 3: terminal leaf, no evaluation -- the reference evaluates and
 * discards; 0 / 4 / 5: nothing of this game was evaluated in this launch). Launches beyond capacity_floats are not recorded;
 * n == 0 switches the log off; dev_log must stay valid until then (or until ao_destroy). ao_eval_log_count: the launches
 * recorded so far. With leaf tactics on (ao_set_leaf_tactics) the log records what the NETWORK said: the override of a
 * proven leaf's value is written behind it. */
int ao_set_eval_log(ao_engine *e, const int32_t *host_games, int32_t n, float *dev_log, int64_t capacity_floats);
int ao_eval_log_count(ao_engine *e);

/* ---- policy/value network ---- replaces model.PVNet(...).forward in eval() mode
 * (model.py:76-104). Parameters are given under their state_dict names.
 * planes: a multiple of 32 in 32 .. 512 (model.py:76-85 takes any width; the Python layer zero-pads other widths to the next
 * multiple). 128 planes (the reference's OUT_PLANES, main.py:35) run on the split-fp16 MFMA kernels; 160 .. 512 planes on the
 * row-chunked fp32-MFMA layer kernels for every batch size, whatever ao_net_set_mode asks for. */
int  ao_net_create(int n_block, int inplanes, int planes, int board, int device, ao_net **out);
void ao_net_destroy(ao_net *n);
const char *ao_net_last_error(const ao_net *n);
/* host float32 data in PyTorch layout (conv OIHW, linear [out][in]); num_batches_tracked is
 * accepted and ignored. */
int  ao_net_set_param(ao_net *n, const char *name, const float *host_data, int64_t numel);
int  ao_net_finalize(ao_net *n); /* fold BN running stats, repack weights for the MFMA kernels */
/* forward for `batch` positions. dev_planes_nchw float32 [batch][C][B][B] -> dev_policy
 * [batch][A], dev_value [batch]; `stream` is a hipStream_t (NULL = default stream). */
int  ao_net_forward(ao_net *n, const float *dev_planes_nchw, int batch, float *dev_policy,
                    float *dev_value, void *stream);
/* Trunk execution: 0 = auto (by batch size), 1 = one kernel per 3x3 conv over groups of 32 boards
 * (medium batches), 2 = group-resident trunk: one workgroup carries 16 boards through every conv
 * layer in a single launch (4096 boards = 256 groups = one per CU), 3 = per-board NHWC with the
 * cells as the MFMA N dimension (latency path for a handful of games), 4 = one launch per layer
 * over (16-board group x row chunk) for the batch sizes in between -- all fp32 MFMA --, 5 = the
 * group-resident trunk with the fp32 contraction carried by fp16 MFMAs: every operand is split in
 * two halves (x = xh + xl) and x*w = xh*wh + xh*wl + xl*wh with fp32 accumulation (the dropped
 * xl*wl term is <= 2^-22 of a product; measured error against an fp64 evaluation equals the fp32
 * path's; activations are clamped to the fp16 range, 65504). Mode 5 needs 128 planes and at least one
 * ResBlock; it runs as one resident launch (boards up to 9x9, >= 3072 boards) or as one launch per conv
 * over (16-board group x row chunk x column tile) (any board up to 15x15, smaller batches), and is
 * what mode 0 picks on such a net for batches of more than ~7800 cells (96 9x9 boards; 5400 cells on wider boards). 6 = mode 5 restricted to
 * the per-layer kernels for EVERY batch size: slower at both ends, but the arithmetic that evaluates a position is then
 * the same whatever else shares the batch, so a game's trajectory under ao_search depends on its own stream and moves
 * only (modes 0 / 5 switch kernel families with the number of active games; all within 1e-4 of model.py:76-104). */
int  ao_net_set_mode(ao_net *n, int mode);
int  ao_net_get_mode(const ao_net *n);
/* Status word of the network, read on `stream` (which is synchronised): AO_NET_FP16_RANGE is set when the
 * split-fp16 trunk (modes 0 / 5 at 128 planes) met an activation beyond the fp16 range and clamped it to 65504 --
 * the outputs of such a forward are finite but not the fp32-equivalent evaluation of model.py:76-104. clear != 0
 * resets the word. ao_search checks it after every move and repeats such a move on the fp32-MFMA trunk (mode 2),
 * see ao_fp16_range_events. */
enum { AO_NET_FP16_RANGE = 1 };
int  ao_net_status(ao_net *n, void *stream, int32_t *flags, int clear);
/* total device time (ms) and count of the TIMED launches of the dominant trunk kernel since the last call
 * (HIP events on the launch stream); used by bench.py's roofline. enable = n > 1: every n-th forward is timed. */
int  ao_net_conv_timing(ao_net *n, int enable, double *ms_total, int64_t *launches);
/* MFMA products per multiply-add of the split-fp16 conv kernels (model.py:6-31,97-104: the 3x3 convs of PVNet). The kernels
 * compute x*w = xh*wh + xh*wl + xl*wh on fp16 halves of both operands (three products, fp32 accumulate). When every conv weight
 * of the loaded network, scaled by its layer's power of two, IS an fp16 number -- ao_net_finalize checks, per export -- wl is zero
 * everywhere and the middle product adds exact zeros: the two-product kernels leave it out (same bits, a third fewer MFMAs).
 * request: 0 = two products whenever the weights allow (default), 3 = always three, -1 = query only. in_force: 2 or 3;
 * weights_fp16: 1 when the loaded weights qualify. A checkpoint gets there by keeping its conv weights on the fp16 grid
 * (tools/train_omok.py --fp16-grid-weights); nothing else about the state_dict changes. */
int  ao_net_products(ao_net *n, int32_t request, int32_t *in_force, int32_t *weights_fp16);
/* Precision of the network forward. AO_NET_PRECISION_FP32 (the default) is everything described above: fp32-equivalent, within
 * 1e-4 of model.py:76-104. AO_NET_PRECISION_FP16 is the opt-in plain-fp16 forward: the operands of every 3x3 conv of the trunk
 * are fp16 -- the weight fp16(w * 2^s) (the high half the library packs anyway), the activation rounded ONCE to fp16, to nearest
 * even, after ReLU and the clamp at 65504 -- with fp32 accumulation: one MFMA product per multiply-add and one fp16 per stored
 * activation. BatchNorm, the residual add, ReLU, the clamp and the heads stay fp32; the next conv, the block's residual add and the
 * heads all read the rounded activation. Float input planes that are not fp16 numbers are rounded to nearest by the resident
 * trunk and taken with all their bits by conv1 in front of the board-resident trunk (the engine's 0/1 planes are exact either way).
 * request: -1 = query only, AO_NET_PRECISION_FP32, AO_NET_PRECISION_FP16, AO_NET_PRECISION_FP16_ALL. in_force: the setting;
 * supported: 1 for networks the split-fp16 kernels cover (128 planes, at least one ResBlock) -- either fp16 setting on any other
 * network is an error and leaves the setting as it was. The setting belongs to the ao_net, survives ao_net_finalize and is
 * independent of ao_net_products, which keeps answering for the fp32-equivalent kernels.
 * What runs under each setting:
 *   AO_NET_PRECISION_FP32      the fp32-equivalent kernels, at every batch size and in every mode.
 *   AO_NET_PRECISION_FP16      exactly the batches that modes 0 / 5 plan onto the resident trunk (boards up to 9x9, >= 192 groups
 *                              of 16) or the board-resident trunk (wider boards, >= 64 boards) run that kernel's one-product form
 *                              (k_trunk16h_f16 / k_trunk16hb_f16 / k_boardh_f16; ao_net_dominant_kernel names it). Every other
 *                              batch size and mode runs the fp32-equivalent kernel it runs anyway -- more accurate, never less.
 *                              CONSEQUENCE: a position's evaluation depends on which kernel its batch is planned onto, to about
 *                              5e-3 in a logit; mode 6 (one arithmetic for every batch size) plans no one-product kernel under
 *                              this setting and must not be combined with it.
 *   AO_NET_PRECISION_FP16_ALL  EVERY forward of the net is the fp16 arithmetic above. The batches of modes 0 / 5 on the resident
 *                              or board-resident trunk run what AO_NET_PRECISION_FP16 runs there; every other batch of modes
 *                              0 / 5 / 6 runs the one-product per-layer kernel k_layer16h_f16 for every layer, conv1 included
 *                              (float planes that are not fp16 numbers are rounded to nearest), and heads that read the rounded
 *                              activation alone. k_layer16hk, k_row16hk and the per-board path have no one-product form and are
 *                              not planned: in mode 0 their batches take the per-layer kernel (16-board groups, bit planes for
 *                              up to 8 input planes). Under mode 6 this is ONE arithmetic for every batch size -- a position's
 *                              evaluation no longer depends on how many others share its batch --, so it may be combined with
 *                              reproducible play. Where it displaces the per-board path or k_row16hk it can be SLOWER than the
 *                              fp32-equivalent kernel.
 * The fp16-range event is reported as ever (AO_NET_FP16_RANGE), and ao_search's recovery on the fp32-MFMA trunk (mode 2) is
 * unchanged under every setting. */
enum { AO_NET_PRECISION_FP32 = 0, AO_NET_PRECISION_FP16 = 1, AO_NET_PRECISION_FP16_ALL = 2 };
int  ao_net_precision(ao_net *n, int32_t request, int32_t *in_force, int32_t *supported);
/* name and algorithmic FLOPs per launch (2*MAC, zero padding counted) of the kernel the timing
 * refers to, for a batch of `boards` positions. */
int  ao_net_dominant_kernel(ao_net *n, int boards, char *name, int name_cap, double *flop_per_launch);
/* the same answer without a network object or a device (pure planning logic): which kernel would carry the conv
 * stack of a PVNet(n_block, inplanes, planes, board) (model.py:76-85) for `boards` positions, trunk_mode as in
 * ao_net_set_mode, in_kind 1 = fp32 plane batch (ao_net_forward), 2 = the engine's bit planes (ao_search).
 * bench.py and tests/test_host_side.py use it to tie a committed rocprofv3 summary to the kernel that runs. */
int  ao_net_plan_kernel(int n_block, int inplanes, int planes, int board, int trunk_mode, int boards, int in_kind,
                        char *name, int name_cap, double *flop_per_launch);

/* ---- replay memory ---- replaces rep_memory = deque(maxlen=MEMORY_SIZE) (main.py:55), its
 * rep_memory.extend(utils.augment_dataset(cur_memory, board_size)) (main.py:229-231,
 * utils.py:226-239) and the mini-batch assembly of main.train (main.py:262-292). The ring lives in
 * HBM; entries are in deque order (index 0 = oldest), the oldest are dropped when full. */
typedef struct ao_replay ao_replay;
int  ao_replay_create(int board, int inplanes, int64_t capacity, int device, ao_replay **out);
void ao_replay_destroy(ao_replay *r);
const char *ao_replay_last_error(const ao_replay *r);  /* r may be NULL: failed ao_replay_create */
int64_t ao_replay_size(const ao_replay *r);            /* len(rep_memory)                        */
int64_t ao_replay_capacity(const ao_replay *r);        /* rep_memory.maxlen                      */
int  ao_replay_clear(ao_replay *r);
/* Appends n samples given as host arrays: states float32 [n][C][B][B] (utils.get_state_pt planes,
 * 0/1: exact in float32), pi float64 [n][A], z float32 [n]. augment != 0 appends the eight
 * symmetries of every sample in the reference's order (rot90 k = 0..3, each followed by its
 * left-right flip), computed on the device; augment == 0 appends the samples as they are. */
int  ao_replay_extend(ao_replay *r, const float *states, const double *pi, const float *z, int64_t n,
                      int augment, void *stream);
/* the same for a call whose first `skipped` samples are NOT supplied: main.self_play(n) appends every sample of its n
 * games (main.py:229-231), but a deque(maxlen) keeps the newest entries only -- when the supplied n samples alone fill
 * the memory (n * 8 >= capacity with augment), the earlier ones of the same call only move the ring position. */
int  ao_replay_extend_skip(ao_replay *r, const float *states, const double *pi, const float *z, int64_t n,
                           int augment, int64_t skipped, void *stream);
/* Device-side sample emission: the same append as ao_replay_extend_skip, but the states are BUILT ON THE DEVICE from the
 * episodes' move lists instead of being uploaded -- replaces the per-ply utils.get_state_pt calls of main.py:159-166 /
 * 219-227 (utils.py:139-168). moves int16 [n_episodes][max_len] (action indices in playing order, anything outside
 * [0, board * board) is padding), sample i = the position of episode ep_of[i] after ply_of[i] of its moves (the root the
 * search of that ply started from); pi / z / augment / skipped as above. */
int  ao_replay_extend_moves(ao_replay *r, const int16_t *moves, int64_t n_episodes, int64_t max_len,
                            const int32_t *ep_of, const int32_t *ply_of, const double *pi, const float *z,
                            int64_t n, int augment, int64_t skipped, void *stream);
/* Mini-batch for m deque indices (host int64; e.g. random.sample(range(len), m)): writes float32
 * device buffers states [m][C][B][B], pi [m][A], z [m] -- the tensors main.train feeds the net. */
int  ao_replay_gather(ao_replay *r, const int64_t *idx, int64_t m, float *dev_states, float *dev_pi,
                      float *dev_z, void *stream);
/* Reads entries [first, first+n) back to host float64 arrays (any may be NULL); this is what
 * main.save_dataset pickles. */
int  ao_replay_read(ao_replay *r, int64_t first, int64_t n, double *states, double *pi, double *z);

/* ---- replay snapshots ---- the reference keeps its memory by pickling the deque (main.save_dataset, main.py:345-348) and
 * rebuilds the deque from the pickle (main.load_data, main.py:351-365); these move the ring, or a range of it, out
 * of HBM and back in, packed and unpacked by kernels on the ring itself, bit for bit. A snapshot is host data without device
 * pointers and holds entries only -- (state, pi, z) in deque order, oldest first. The engine's planes are 0/1, so a plane
 * packs to one bit per cell; pi is exact float64 but sparse, so it packs to a cell mask and its non-zero values. An entry is
 * kind 0 only when every plane value has the bit pattern of +0.0f or 1.0f; anything else (-0.0f, 0.5f, the arbitrary floats
 * ao_replay_extend accepts) makes it kind 1, whose planes are kept raw. A packed entry is 5 + 8 * W * (C + 1) + 8 * nnz bytes
 * (W = words, nnz its non-zero pi cells), plus 4 * C * A for kind 1. The form is canonical: one ring content has exactly
 * one snapshot. All arrays are caller-owned host memory. */
typedef struct ao_replay_snapshot {
    int32_t board, inplanes;          /* of the exporting memory; the importing memory must have the same                  */
    int32_t format, words;            /* format = 1; words = W = (board * board + 63) / 64                                 */
    int64_t entries;                  /* ao_replay_export reads it as the capacity of the per-entry arrays, writes n back  */
    int64_t pi_values, raw_entries;   /* lengths of pi_val / raw (raw counted in entries). ao_replay_export reads them as the
                                         capacity of the caller's arrays and writes back what it used                      */
    uint8_t  *kind;     /* [entries]        0 = planes as bits, 1 = planes raw                                             */
    float    *z;        /* [entries]        the stored float32, bits preserved                                             */
    uint64_t *bits;     /* [entries][C][W]  bit (c % 64) of word c / 64 is set when the plane's cell c holds exactly 1.0f;
                                            all zero for kind 1                                                            */
    uint64_t *pi_mask;  /* [entries][W]     bit set when the 64-bit PATTERN of pi[c] is non-zero (-0.0 and NaN are values)   */
    double   *pi_val;   /* [pi_values]      the non-zero patterns, ascending cell order, entry after entry; an entry owns
                                            popcount(its mask) of them                                                     */
    float    *raw;      /* [raw_entries][C][A]  the planes of the kind-1 entries, in entry order                           */
} ao_replay_snapshot;
/* The count pass of an export over deque entries [first, first + n): what pi_val and raw must hold. Synchronises like
 * ao_replay_read; read-only on the ring. */
int  ao_replay_export_size(ao_replay *r, int64_t first, int64_t n, int64_t *pi_values, int64_t *raw_entries);
/* Packs deque entries [first, first + n) on the device into the caller's arrays and downloads only packed bytes. A count pass
 * sizes the variable-length parts; a chunk of entries is closed when its packed size reaches chunk_bytes (0 = 64 MiB, at most
 * 1 GiB), so the device workspace is bounded by chunk_bytes plus one entry (plus 13 bytes per entry of a chunk), whatever the
 * capacity of the ring. Read-only on the ring; sees everything queued before it (synchronises like ao_replay_read) and returns
 * with the arrays complete; `stream` carries its launches and copies. Fails with nothing written when the range is outside
 * the memory or a capacity (entries, pi_values, raw_entries) is too small. */
int  ao_replay_export(ao_replay *r, int64_t first, int64_t n, ao_replay_snapshot *snap, int64_t chunk_bytes, void *stream);
/* deque.extend(entries of the snapshot) -- on a cleared memory, main.load_data's deque(pickle.load(f), maxlen) (main.py:365): appended in order behind what the ring holds, only the newest `capacity`
 * survive; entries of the snapshot that cannot survive are neither uploaded nor unpacked. The destination may have any
 * capacity and any fill. Every byte of every slot it claims is written. Refused with the ring untouched when board or
 * inplanes differ or when the snapshot fails ao_replay_snapshot_check (checked before anything is uploaded). Chunks as in
 * ao_replay_export. */
int  ao_replay_import(ao_replay *r, const ao_replay_snapshot *snap, int64_t chunk_bytes, void *stream);
/* Holds a snapshot to the canonical form; needs no memory and no device. board 3..15, inplanes 1..32, format 1, words as
 * derived from the board; no mask or plane bit at or above cell A; kind is 0 or 1; bits is zero on kind-1 rows; pi_values
 * equals the sum of the mask popcounts; raw_entries equals the number of kind-1 entries; no all-zero pattern in pi_val.
 * Non-zero on the first violation; ao_replay_last_error(NULL) describes it. */
int  ao_replay_snapshot_check(const ao_replay_snapshot *snap);

/* ---- rollout agents ---- replace PUCTAgent.get_pi (agents.py:263-441) and UCTAgent.get_pi
 * (agents.py:443-614): net-free searches with random playouts. One handle owns G independent
 * games, each with its own numpy-legacy MT19937 stream; a search runs entirely in one kernel. */
typedef struct ao_rollout ao_rollout;
typedef struct ao_rollout_config {
    int32_t board;     /* board edge 3..15                                                     */
    int32_t win_mark;  /* 0 = reference rule: 3 if board == 3 else 5 (agents.py:270)           */
    int32_t sims;      /* num_mcts; every get_pi runs num_mcts + 1 simulations (agents.py:318) */
    int32_t games;     /* G                                                                    */
    int32_t mode;      /* 0 = PUCTAgent, 1 = UCTAgent                                          */
    int32_t device;
    double  c_puct;    /* 0 = 5 (agents.py:271); PUCT only                                     */
} ao_rollout_config;
int  ao_rollout_create(const ao_rollout_config *cfg, ao_rollout **out);
void ao_rollout_destroy(ao_rollout *r);
const char *ao_rollout_last_error(const ao_rollout *r); /* r may be NULL: failed create          */
int  ao_rollout_seed(ao_rollout *r, int game, uint32_t seed);            /* np.random.seed(seed) */
int  ao_rollout_get_rng_state(ao_rollout *r, int game, uint32_t *mt624, int32_t *pos,
                              int32_t *has_gauss, double *gauss);
int  ao_rollout_set_rng_state(ao_rollout *r, int game, const uint32_t *mt624, int32_t pos,
                              int32_t has_gauss, double gauss);
/* get_pi(root_id, board, turn, tau) for every active game: moves [G][A] (row g = root_id[1:] of
 * game g, first nmoves[g] entries used; board and turn follow from the id). Host outputs
 * (any may be NULL): pi float64 [G][A] one-hot; stat float64 [G][A] = visit counts of the root's
 * children (PUCT, 0 elsewhere) or their q (UCT, -inf elsewhere); action int32 [G]. */
int  ao_rollout_search(ao_rollout *r, const int32_t *moves, const int32_t *nmoves,
                       const uint8_t *active, double *pi, double *stat, int32_t *action);

/* ---- 3x3 UCT of 1_tictactoe_MCTS ---- replaces the per-move search loop of mcts_vs.py:153-183
 * (MCTS.selection / expansion / simulation / backup, mcts_vs.py:15-131; BASELINE configs[0]).
 * Randomness is Python's `random` module stream (MT19937 words + index, random.getstate()[1]). */
typedef struct ao_ttt ao_ttt;
typedef struct ao_ttt_config {
    int32_t board;     /* state_size (env.py: 3); any 3..15                                    */
    int32_t win_mark;  /* 0 = 3 on a 3x3 board, else 5                                         */
    int32_t sims;      /* num_mcts (mcts_vs.py:144: 1500)                                      */
    int32_t games;     /* G independent searches per call                                      */
    int32_t device;
} ao_ttt_config;
int  ao_ttt_create(const ao_ttt_config *cfg, ao_ttt **out);
void ao_ttt_destroy(ao_ttt *r);
const char *ao_ttt_last_error(const ao_ttt *r);   /* r may be NULL: failed create */
int  ao_ttt_seed(ao_ttt *r, int game, uint32_t seed);                       /* random.seed(seed)     */
int  ao_ttt_get_rng_state(ao_ttt *r, int game, uint32_t *mt624, int32_t *pos);   /* random.getstate() */
int  ao_ttt_set_rng_state(ao_ttt *r, int game, const uint32_t *mt624, int32_t pos);
/* boards int8 [G][A] row-major (+1 = O / first player, -1 = X), turns int32 [G] (0 = O to move).
 * Host outputs (any may be NULL): q float64 [G][A] of the root's children (-inf elsewhere), n float64
 * [G][A] their visit counts, action int32 [G] = max_action (first maximum of q). */
int  ao_ttt_search(ao_ttt *r, const int8_t *boards, const int32_t *turns, const uint8_t *active,
                   double *q, double *n, int32_t *action);

/* ---- position batch ---- stateless questions about positions the caller names; no game, no tree. Replaces the
 * per-position host calls around the search: utils.check_win (utils.py:30-59), utils.get_board / get_turn /
 * legal_actions (utils.py:171-186, 22-27), utils.get_state_pt (utils.py:139-168) and ZeroAgent.get_pv
 * (agents.py:252-260; the monitor of eval_main.py:243 calls it for every ply of every match). One wavefront per
 * position; a call takes any n and works through it in chunks of `capacity` positions (one upload, one launch, one
 * download per chunk) on the workspace's own stream, and returns with everything complete.
 * board 3..15; win_mark 3..5 and <= board; inplanes 1..9: what ao_net_create accepts, as far as the plane encoder of the
 * search reaches (eight plies of history); capacity >= 1. */
typedef struct ao_positions ao_positions;   /* device workspace for up to `capacity` positions per launch */
int  ao_positions_create(int board, int inplanes, int win_mark, int capacity, int device, ao_positions **out);
void ao_positions_destroy(ao_positions *p);
const char *ao_positions_last_error(const ao_positions *p);   /* p may be NULL: failed create */
/* utils.check_win(board, win_mark) (utils.py:30-59) for n raw boards: host int8 [n][B][B], +1 black, -1 white, 0 empty
 * (any other value counts as empty). The boards need not be reachable in play: the reference's scan is reproduced --
 * win_mark x win_mark windows in row-major order, the first window with a complete row, column or diagonal decides,
 * black before white inside it; no line: 3 on a full board, else 0. host_win int32 [n]. */
int  ao_positions_check_win(ao_positions *p, const int8_t *host_boards, int32_t n, int32_t *host_win);
/* Position i is the id (0, moves[i * stride], ..., moves[i * stride + n[i] - 1]): its moves are placed in order, black
 * first. Outputs (any may be NULL):
 *   host_status  int32 [n]        utils.check_win of the final board (utils.py:30-59); moves past a win are placed too
 *   host_end_ply int32 [n]        index of the first move after which check_win is non-zero, -1 if there is none
 *   host_turn    int32 [n]        utils.get_turn of the id (utils.py:182-186)
 *   host_board   int8  [n][B][B]  utils.get_board (utils.py:171-179)
 *   host_legal   uint8 [n][A]     1 on empty cells: utils.legal_actions as a mask (utils.py:22-27), not its set order
 *   dev_planes_nchw float32 [n][C][B][B] on the device: utils.get_state_pt (utils.py:139-168), the layout Agent.model
 *                                 expects (agents.py:175); the device is synchronised before it is written
 *   host_err     int32 [n]        0 ok, 1 a move outside 0..A-1, 2 a move onto an occupied cell, 3 n[i] < 0 or n[i] > A
 * A position with an error has every output of its own zeroed (end_ply included) and touches no other position; the
 * call still returns 0. Non-zero: n[i] in 1..A exceeds stride, or a HIP error. */
int  ao_positions_from_moves(ao_positions *p, const int32_t *host_moves, int32_t stride, const int32_t *host_n, int32_t n,
                             int32_t *host_status, int32_t *host_end_ply, int32_t *host_turn, int8_t *host_board,
                             uint8_t *host_legal, float *dev_planes_nchw, int32_t *host_err);
/* ZeroAgent.get_pv (agents.py:252-260) for n positions: the planes are built on the device and every chunk runs ONE
 * ao_net_forward on the workspace's stream, so the result is bit for bit what ao_net_forward gives for the same planes in
 * the same batch. host_policy float32 [n][A]: the softmax over all A cells, nothing masked; host_value float32 [n].
 * Terminal positions are evaluated like any other (agents.py:171-178); host_status (may be NULL) says which they are.
 * A position with an error (host_err, may be NULL; codes as above) is fed as the empty board, so that its row cannot
 * disturb the rest of its chunk, and gets a zero policy and a zero value. The network must be finalized and match in
 * board, inplanes and device (as for ao_search); the device is synchronised first, the network's workspace is shared. */
int  ao_positions_evaluate(ao_positions *p, ao_net *net, const int32_t *host_moves, int32_t stride, const int32_t *host_n,
                           int32_t n, float *host_policy /*[n][A]*/, float *host_value /*[n]*/,
                           int32_t *host_status, int32_t *host_err);
/* ao_positions_evaluate with the 8-fold symmetry ensemble. nsym is 1 or 8; nsym 1 returns the bits of
 * ao_positions_evaluate. nsym 8: row 8 i + s of the forward's batch is sym_planes(planes of position i, s) (numbering as
 * for ao_set_leaf_symmetry), ONE forward runs over the eight rows of every position of a chunk -- a chunk holds
 * capacity / 8 positions, so capacity must be at least 8 -- and a kernel brings each policy row back into the board's own
 * frame and takes the mean in fp32, in this order: policy[i][c] = 0.125f * (((p_0 + p_1) + p_2) + ... + p_7), p_s the
 * value of row 8 i + s at the cell c went to under s; host_value likewise. Everything else as ao_positions_evaluate. */
int  ao_positions_evaluate_sym(ao_positions *p, ao_net *net, const int32_t *host_moves, int32_t stride, const int32_t *host_n,
                               int32_t n, int32_t nsym, float *host_policy /*[n][A]*/, float *host_value /*[n]*/,
                               int32_t *host_status, int32_t *host_err);
/* The cells that win at once. No reference counterpart: the definition is utils.check_win (utils.py:30-59) and nothing
 * else. P is the position of id i (moves as for ao_positions_from_moves), k its side to move (black on even plies). A
 * cell c is a WINNING CELL of colour j in P if check_win(P) == 0, c is empty, and check_win of P's board with a stone of
 * colour j on c returns j's win index (1 black, 2 white). Overlines count, as in the reference; a move that fills the
 * board without a line (win index 3) is not a winning move; on a terminal position no cell is a winning cell for anyone.
 * Outputs (any may be NULL):
 *   host_mine    uint8 [n][A]     1 on the winning cells of k
 *   host_theirs  uint8 [n][A]     1 on the winning cells of the opponent, as if it were to move: the cells k must occupy
 *   host_status  int32 [n]        check_win(P)
 *   host_turn    int32 [n]        utils.get_turn of the id
 *   host_err     int32 [n]        as ao_positions_from_moves; a position with an error has every output of its own zeroed
 * Chunks, staging and return value as ao_positions_from_moves; n == 0 is a no-op. */
int  ao_positions_win_cells(ao_positions *p, const int32_t *host_moves, int32_t stride, const int32_t *host_n, int32_t n,
                            uint8_t *host_mine, uint8_t *host_theirs, int32_t *host_status, int32_t *host_turn,
                            int32_t *host_err);
/* The tactical audit of n game records (move lists as above), every ply of each: with mine(P) / theirs(P) the winning
 * cells of the side to move / of its opponent as defined above (through utils.check_win, utils.py:30-59), the flag byte
 * of the move m_t played in P_t, set only while check_win(P_t) == 0, is
 *    1 WIN_AVAILABLE  mine(P_t) is not empty            2 WIN_TAKEN  m_t is in mine(P_t)
 *    4 THREAT         mine(P_t) is empty and theirs(P_t) is not
 *    8 BLOCKED        THREAT and m_t is in theirs(P_t)
 *   16 LOST           THREAT and theirs(P_t) holds two or more cells (one stone cannot answer both)
 * Plies from the first terminal position on get 0; their moves are still placed and validated. Outputs (any may be NULL):
 *   host_flags   uint8 [n][A]     flag byte of ply t at [i][t], zeros beyond the record
 *   host_counts  int32 [n][8]     0 plies audited, 1 WIN_AVAILABLE, 2 wins missed (WIN_AVAILABLE without WIN_TAKEN),
 *                                 3 single threats (THREAT without LOST), 4 blocks missed (single threat without BLOCKED),
 *                                 5 LOST, 6 end_ply and 7 status as ao_positions_from_moves
 *   host_err     int32 [n]        as ao_positions_from_moves; a record with an error has all-zero outputs
 * Chunks, staging and return value as ao_positions_from_moves; n == 0 is a no-op. */
int  ao_positions_audit(ao_positions *p, const int32_t *host_moves, int32_t stride, const int32_t *host_n, int32_t n,
                        uint8_t *host_flags, int32_t *host_counts, int32_t *host_err);
/* Forced wins by continuous fours (VCF) for n positions (ids as above). No reference counterpart: the definition asks
 * utils.check_win (utils.py:30-59) and nothing else, through the winning cells defined above. a is the side to move (the
 * attacker), cells are always tried in ascending order:
 *   wins_within(P, d)  a to move, at most d attacker moves. No if check_win(P) != 0. With mine / theirs the winning cells of
 *                      a / of its opponent in P: yes if mine is not empty; no if d == 1 or theirs holds two or more cells;
 *                      otherwise yes if four(P, c, d) for some c of theirs or, theirs empty, of all empty cells -- the
 *                      first such c.
 *   four(P, c, d)      P1 = P with a on c. No if check_win(P1) != 0, if the defender has a winning cell in P1 or if a has
 *                      none (c made no four); yes if wins_within(P1 with the defender on b, d - 1) for EVERY winning cell
 *                      b of a in P1 (the forced replies).
 *   for D = 1 .. max_depth, no iteration skipped: the root is wins_within(P, D), except that it tries every candidate and
 *                      collects those that succeed (mine, if that is not empty); the first D with any ends the search.
 * `nodes` counts the wins_within calls of all iterations; the call number max_nodes + 1 ends the search as UNKNOWN.
 * utils.forced_win of the Python package is this text on the host. 1 <= max_depth <= 16, 1 <= max_nodes <= 65536 (the
 * node cap bounds the launch: there is no unlimited mode); outside: non-zero return. Outputs (any may be NULL):
 *   host_result     int32 [n]     0 no forced win within max_depth, 1 forced win, 2 UNKNOWN: nodes is then max_nodes and
 *                                 every other output of the search is as for 0, even if a winning move had been found
 *   host_depth      int32 [n]     the smallest D, in attacker moves; 0 unless result is 1
 *   host_move       int32 [n]     the lowest cell of host_moves_mask, -1 if there is none
 *   host_moves_mask uint8 [n][A]  1 on every first move that wins within depth
 *   host_line       int16 [n][2 * max_depth - 1]  the principal line, padded with -1: host_move, the lowest forced reply,
 *                                 then at every later attacker node the first c that succeeded (or the lowest cell of
 *                                 mine) and the lowest forced reply to it; it ends on the stone that makes the line
 *   host_line_len   int32 [n]     stones in host_line; may be less than 2 * depth - 1
 *   host_nodes      int32 [n]
 *   host_status, host_turn, host_err  int32 [n]  as ao_positions_win_cells; a terminal position has result 0, a position
 *                                 with an error has every output zeroed, move -1 and line -1
 * One wavefront walks one position depth first (explicit stack in LDS, no recursion). Chunks, staging and return value
 * as ao_positions_from_moves; n == 0 is a no-op. */
int  ao_positions_forced_wins(ao_positions *p, const int32_t *host_moves, int32_t stride, const int32_t *host_n, int32_t n,
                              int32_t max_depth, int32_t max_nodes, int32_t *host_result, int32_t *host_depth,
                              int32_t *host_move, uint8_t *host_moves_mask, int16_t *host_line, int32_t *host_line_len,
                              int32_t *host_nodes, int32_t *host_status, int32_t *host_turn, int32_t *host_err);
/* Which replies hold against a forced win by continuous fours, for n positions (ids as above). No reference counterpart:
 * the definition is forced_win above, which asks utils.check_win (utils.py:30-59) and nothing else. P is the position of
 * id i, m its side to move, o the opponent, and forced_win(Q, a) the search above on the board Q with a as the attacker
 * (nothing in it depends on whose turn the stone count says it is). If check_win(P) != 0 every output but status and turn
 * is zero. Otherwise
 *   the threat         forced_win(P, o): what o could do if m passed;
 *   for every empty c  r = forced_win(P with m on c, o); reply[c] = 1 + r.result, depth[c] = r.depth. A stone that makes
 *                      a line or fills the board leaves a terminal position, and forced_win says no: such a reply holds.
 * Each of the A + 1 searches has its own budget of max_nodes and none is skipped on the strength of another one's answer
 * (no "no threat, hence all replies hold": host_nodes pins that). utils.forced_defences of the Python package is this
 * text on the host. Limits of max_depth and max_nodes as above. Outputs (any may be NULL):
 *   host_threat       int32 [n]     result of the threat search: 0, 1 or 2 (UNKNOWN)
 *   host_threat_depth int32 [n]     its depth, 0 unless the threat is 1
 *   host_threat_moves uint8 [n][A]  1 on every first move of o that wins within that depth
 *   host_reply        uint8 [n][A]  0 NONE not an empty cell, 1 SAFE the reply holds, 2 LOSES, 3 UNKNOWN the search of
 *                                   that reply ran out of nodes
 *   host_depth        uint8 [n][A]  attacker moves of o's forced win after the reply; 0 unless the reply is LOSES
 *   host_counts       int32 [n][4]  empty cells, SAFE, LOSES, UNKNOWN
 *   host_nodes        int32 [n]     the sum of `nodes` over the searches run (at most 226 x 65536)
 *   host_status, host_turn, host_err  int32 [n]  as ao_positions_win_cells; a position with an error has every output zeroed
 * One wavefront per (position, reply) pair and one for the pass, each the search of ao_positions_forced_wins, then one
 * wavefront per position gathers them: `capacity` positions, hence capacity x (A + 1) wavefronts, per launch. Chunks,
 * staging and return value as ao_positions_from_moves; n == 0 is a no-op. */
int  ao_positions_forced_defences(ao_positions *p, const int32_t *host_moves, int32_t stride, const int32_t *host_n, int32_t n,
                                  int32_t max_depth, int32_t max_nodes, int32_t *host_threat, int32_t *host_threat_depth,
                                  uint8_t *host_threat_moves, uint8_t *host_reply, uint8_t *host_depth, int32_t *host_counts,
                                  int32_t *host_nodes, int32_t *host_status, int32_t *host_turn, int32_t *host_err);

/* ---- guarded device allocations (a test mode of the host code; off by default) -------------------------------------------
 * Two environment variables, read at every device allocation of every handle (ao_engine, ao_net, ao_replay, ao_rollout,
 * ao_ttt, ao_positions):
 *   AO_POOL_GUARD=<bytes>  unset or 0: plain hipMalloc, as ever. Otherwise the value is rounded up to a multiple of 4096 and
 *                          every block gets that many guard bytes in front and behind.
 *   AO_POOL_FILL=<0..255>  default 255: the byte written to both guards and to the whole body of a guarded block, before the
 *                          owner sees it (hipMemset, hipDeviceSynchronize).
 * The mode costs allocation-time and free-time work only; no kernel and no launch differs. A guard byte that differs from the
 * fill is a stray write; outputs that differ between two fills, or from the plain mode, are stale or stray reads.
 *
 * ao_guard_check waits for every device that has guarded blocks (the current device is the same afterwards), reads all guards
 * back and reports in *blocks how many guarded blocks are alive and in *damaged how many are damaged -- including those whose
 * damage was found when they were freed, which are kept until this call reports them. msg (cap bytes, always terminated)
 * describes the first few, one per line:
 *   block #<allocation ordinal> (<bytes> B, device <d>): <n> damaged byte(s), first at start-<k>|end+<k>, found 0x.. (fill 0x..)
 * start-k is k bytes before the block's first byte, end+k is k bytes after the first byte behind it (end+0). Reported guards are
 * filled again: the next call reports only new damage. Returns non-zero on a HIP error (its text in msg).
 * ao_guard_block names the index-th live guarded block in allocation order (pointer to the body, its bytes, its guard
 * bytes); non-zero past the end. ao_guard_mode reports what an allocation made now would use: the guard bytes after rounding
 * (0: mode off) and the fill byte. Any output may be NULL. */
int  ao_guard_check(int32_t *blocks, int32_t *damaged, char *msg, int cap);
int  ao_guard_block(int32_t index, void **ptr, int64_t *bytes, int64_t *guard);
int  ao_guard_mode(int64_t *guard, int32_t *fill);

#ifdef __cplusplus
}
#endif
#endif
