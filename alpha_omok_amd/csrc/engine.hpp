// engine.hpp -- what the files that drive an ao_engine share: the engine itself, the launch loop both search drivers run on, the
// state of the rolling search, and the few helpers that more than one of those files calls. engine.hip has the lifecycle, the
// step-wise protocol and ao_search; every other subsystem's host driver stands beside its kernels: roll.hip (ao_roll_*),
// tree_readout.hip, tree_proofs.hip, root_tactics.hip, tree_snapshot.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "../../include/omok_hip.h"
#include "engine_types.hpp"
#include "host_handle.hpp"
#include "roll_schedule.hpp"
#include "search_schedule.hpp"

// The developer switches of the search driver (MoveSearch, engine.hip; INTEGRATION.md has the table). They have two lifetimes:
//  * read ONCE per process, by its first search: they pick a code path for an experiment or a profile and hold for the run;
//  * read ANEW by every search that enters the catch-up rounds: tests/test_gpu_production_loop.py sets and unsets them between
//    the searches of one process.
struct DevSwitches {
    bool static_rows;     // AO_STATIC_ROWS: the per-move packing of rounds 3 - 4 everywhere
    bool dynamic_rows;    // AO_DYNAMIC_ROWS: hand out rows per simulation without ao_set_row_cap
    int descent_budget;   // AO_DESCENT_BUDGET (experiment): levels of a descent per launch, 0 = no bound
    bool row_trace;       // AO_ROW_TRACE: rows asked for, launch by launch, on stderr
    bool launch_timing;   // AO_LAUNCH_TIMING: is the simulation loop host-bound?
    static const DevSwitches& process() {
        static const DevSwitches s{getenv("AO_STATIC_ROWS") != nullptr, getenv("AO_DYNAMIC_ROWS") != nullptr,
                                   getenv("AO_DESCENT_BUDGET") ? atoi(getenv("AO_DESCENT_BUDGET")) : 0,
                                   getenv("AO_ROW_TRACE") != nullptr, getenv("AO_LAUNCH_TIMING") != nullptr};
        return s;
    }
    // per search: cut the catch-up loop short (-1 = not set; tests: 0 = a short search must be an error) / run its rounds
    // without a sit-out window from the start
    static int catchup_rounds() { const char* v = getenv("AO_CATCHUP_ROUNDS"); return v ? atoi(v) : -1; }
    static bool catchup_window_off() { return getenv("AO_CATCHUP_WINDOW_OFF") != nullptr; }
};

// What both search drivers run on: the launch plan (the network's input, the driver's copy of the tree parameters) and the ring
// of row counters d_live[kLive]. With rows handed out per simulation (engine_types.hpp, TreeParams::live) selection launch i
// counts the rows its leaves ask for in word i % kLive, the network launch behind it reads that word, and the host sums the
// words up into ao_row_stats where the ring wraps and when a driver asks (search_schedule.hpp). The methods are engine.hip's.
struct ao_engine;
struct LaunchLoop {
    ao_engine* e = nullptr;
    bool per_sim = false;          // rows are handed out and counted per simulation (otherwise: packed per move by the host, no ring)
    int cap_rows = 0, in_kind = 1; // rows of one network launch; the input the network wants (net_plan): 2 = bit planes, otherwise the interleaved fp32 batch
    const float* net_in = nullptr;
    ao::TreeParams p{};            // the driver's copy of e->tp; `live` changes per launch
    int64_t launch = 0, harvested = 0;   // selection launches so far; ... of which the row counters are summed up already
    int64_t* traffic = nullptr;    // where the bytes of a harvest are charged (the rolling search's ao_roll_stats), or null
    int plan(ao_engine* e, ao_net* net, int rows);   // a fresh loop with the plan for launches of `rows` rows
    int zero_ring();                     // where a driver sets per_sim, and at every wrap
    unsigned* slot(int64_t i) const;     // the counter word of launch i (null without per_sim)
    bool wraps(int64_t i) const { return per_sim && i > 0 && slot(i) == slot(0); }   // launch i counts in the ring's first word again
    unsigned counted(int64_t i) const;   // what launch i counted, once harvested (until the ring wraps again)
    int advance();                       // behind a network launch: the next selection launch and its counter word
    int harvest(int64_t upto);           // sums up the launches [harvested, upto); synchronises if there are any
    // Leaf tactics (ao_set_leaf_tactics), called on either side of every network launch that a tree launch follows; nothing at
    // all with the switch off. before_net: the solver on the leaves of the last selection, on the engine's second stream behind
    // an event recorded here -- it runs beside the network. Otherwise (behind the network launch and the eval log): the engine's
    // stream waits for the solver's event and writes +1 into the rows of the proven leaves. lt_serial (AO_LEAF_TACTICS_SERIAL,
    // read by plan()): both kernels on the engine's own stream behind the network launch instead; the same bits.
    bool lt_serial = false;
    int leaf_tactics(bool before_net);
};

// what k_roll_verdict (roll.hip) reads of a finished batch of the solver beside the rolling search: RollBatch below holds one
namespace ao {
struct RollBatchView {
    const uint64_t* bar;      // [n][kBBWords]
    const int32_t* verdict;   // [4][n]: verdict, depth, nodes, unknown
    const uint8_t* allowed;   // [n][A] or null
    int n;
};
}  // namespace ao

// The rolling search (ao_roll_*, roll.hip): what lives from ao_roll_begin to ao_roll_end. The rules are roll_schedule.hpp's.
// The forced-win solver beside the loop (ao_roll_set_tactics). A BATCH is the solver's run on the roots of the games that were
// to begin a move at one turn (or begin / join): queued on `stream`, which touches nothing but the batch's own buffer, between two
// events. Its games wait (ROLL_WAITING) until a later turn finds the second event reached; then they begin their move on the
// engine's stream with the batch's bar rows and verdicts (k_roll_verdict in front of k_roll_begin).
struct RollBatch {
    bool busy = false;
    int n = 0, age = 0;                   // games; turns since it was started
    hipEvent_t ready = nullptr, done = nullptr;   // engine stream: the position rows are written; solver stream: the verdicts are
    std::vector<int32_t> games;           // [n]
    std::vector<uint8_t> bonus;           // [n] the root was fresh when the game was listed
    std::vector<uint32_t> mt; std::vector<int32_t> pos;   // [n][624], [n] the games' streams as gathered when they were listed
    ao::DevBuf<unsigned char> buf{nullptr};   // position rows, won / stage / pair words, verdict words, bar rows, allowed rows: O(n A)
    ao::RollBatchView view{};
};
struct RollTactics {
    int max_depth = 0, max_nodes = 0, solved_sims = 0;   // ao_roll_set_tactics; max_depth == 0: disarmed
    bool want_allowed = false;
    bool on = false;                      // the open roll runs with the solver
    int hold = 0;                         // AO_ROLL_TACTICS_HOLD, read at ao_roll_begin
    hipStream_t stream = nullptr;
    RollBatch slot[ao::kRollBatchSlots];
    std::vector<int> pending;             // busy slots, oldest first
    int n_waiting = 0;
    int32_t* d_words = nullptr; uint8_t* d_allowed = nullptr;      // [G][4], [G][A]: what the solver said at the root of each game's current move
    int32_t* d_out_words = nullptr; uint8_t* d_out_allowed = nullptr;   // compact rows of a turn's records
    int32_t* h_words = nullptr; uint8_t* h_allowed = nullptr;      // pinned, [G][4], [G][A]
    std::vector<int32_t> rec_words; std::vector<uint8_t> rec_allowed; int rec_count = 0;   // of the last ao_roll_run
    int64_t stats[6] = {0, 0, 0, 0, 0, 0};   // ao_roll_tactics_stats
};

struct RollState {
    bool open = false, draining = false;
    RollTactics tac;
    ao_net* net = nullptr;
    bool early = false, want_visit = false, want_policy = false;
    ao::RollCadence cad;
    bool look_pending = false;            // a look's counters have not been read yet
    std::vector<uint8_t> in_move;         // [G] ao::RollGame: out of a move, searching, or waiting for the solver's verdict
    int n_in_move = 0;
    std::vector<int32_t> tau_plies;       // [G], empty: tau 1 always
    std::vector<int32_t> sims; int sims_stride = 0;      // [G][stride] budgets by ply, empty: ao_config.sims
    std::vector<uint8_t> noise; int noise_stride = 0;    // [G][stride] noise switches by ply, empty: the engine's
    LaunchLoop loop;                      // always rows per simulation; no sit-out window, no launch order, no fused step
    // compact buffers of a turn, allocated by the first roll of the engine: [G] games, [G][kRollItem], [G][kRollRec], [3][G][A], [G][Ap]
    int32_t* d_games = nullptr; int32_t* d_items = nullptr; int32_t* d_rec = nullptr; double* d_out = nullptr; double* d_noise = nullptr;
    int32_t* h_i32 = nullptr;             // pinned: [4][G] done, target, leaf status, error words; [G] games; [G][kRollItem]; [G][kRollRec]
    // ao_roll_stats
    int64_t turns = 0, games_turned = 0, bytes = 0, last_games = 0, last_bytes = 0;
};

struct ao_engine : ao::HandleBase {
    ao_config cfg{};
    ao::TreeParams tp{};
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;
    int A = 0, Ap = 0, G = 0, Gp = 0, S = 0;
    ao::DevPool pool;
    // device scratch
    uint8_t* d_active = nullptr; int8_t* d_tau = nullptr; int32_t* d_extra = nullptr;
    uint8_t* d_mask = nullptr;
    std::vector<int32_t> h_walk;     // staging of ao_set_root(s): [G][A] moves + games, counts, prev_known, status
    float* d_policy = nullptr; float* d_value = nullptr;  // native-net outputs [Gp][A], [Gp]
    uint8_t* d_planes_u8 = nullptr;                       // bit planes [Gp][u8_row] (input of the split-fp16 kernels)
    int32_t* d_row = nullptr;                             // [2G] batch row of each game in ao_search (active games packed, or handed out per simulation by the tree kernel), then the game of each row
    std::vector<int32_t> h_row;
    // rows handed out per simulation: LaunchLoop's ring of counter words, one per launch; row_cap = rows one simulation may take
    // (0: as many as there are active games)
    static constexpr int kLive = 2048;
    unsigned* d_live = nullptr;
    int32_t* d_order = nullptr;      // [G] launch order of k_expand_select's slots for over-subscribed searches (k_order, per move); AO_TREE_ORDER=0: off
    bool order_on = true;
    unsigned* h_live = nullptr;                           // pinned [kLive]
    unsigned* d_ctl = nullptr;                            // [2][4] the sit-out window of the current / the next launch (tree_device.hpp, sit_window)
    int row_cap = 0;
    double ask_frac = 1.0;                                // rows asked for per simulation of a game in the last over-subscribed move (1 - terminal share)
    ao::RowLedger rs;                                     // ao_row_stats
    // ao_set_eval_log: what the network returned to the listed games, per simulation of the current ao_search
    int32_t* d_log_games = nullptr; int log_n = 0; float* log_dev = nullptr; int64_t log_cap = 0; int64_t log_sim = 0;
    size_t il_bytes = 0; int il_group_zeroed = -1, il_nchq_zeroed = -1;  // layout for which batch_il's padding is zero
    // host mirrors
    std::vector<std::vector<int32_t>> moves;
    std::vector<int32_t> status;     // AO_ROOT_*
    std::vector<int32_t> over;       // win index once the game ended
    std::vector<uint8_t> active;
    std::vector<int32_t> has_gauss; std::vector<double> gauss;
    uint32_t* h_mt = nullptr; int32_t* h_pos = nullptr; double* h_noise = nullptr;  // pinned
    double* h_out = nullptr;         // pinned [3][G][A]
    int32_t* h_i32 = nullptr;        // pinned [4][G]
    int sims_left = 0;
    bool in_move = false, ended = false;
    // per-game budgets and settling (ao_begin_move_opts, ao_settle, ao_search_opts, ao_search_sims)
    std::vector<int32_t> bonus;      // [G] 1 where this move's root was fresh (its expansion is one simulation more than the budget)
    int64_t target_sum = 0;          // simulations the current move set out to run, over the active games
    int64_t move_saved = 0;          // ... and how many of them settling took away
    bool leaf_open = false;          // a selection has been launched whose leaves are not backed up yet (k_settle's `pending`)
    uint8_t* d_settled = nullptr;    // [G] 1 where k_settle lowered the game's target in this move
    bool settled_dirty = false;      // d_settled may hold ones
    uint8_t* d_early = nullptr;      // [G] ao_search_opts' early_stop mask
    int32_t* d_settle = nullptr;     // [4] k_settle's counters of one launch
    int32_t* h_settle = nullptr;     // pinned [4]
    int64_t settled_total = 0, saved_total = 0;
    // the root bar (ao_set_root_bar, ao_root_tactics with apply): what the NEXT ao_begin_move* / ao_search* is restricted to.
    // Either the caller's masks on the host (bar_allowed / bar_has), turned into bitboards and uploaded by begin_move_impl, or
    // bitboards that ao_root_tactics left in d_bar (bar_on_device). begin_move_impl consumes it; `used_*` is what the current
    // move consumed, for the move the fp16-range recovery repeats.
    uint64_t* d_bar = nullptr;              // [G][kBBWords] barred actions of the current move
    std::vector<uint64_t> h_bar;            // staging of d_bar
    std::vector<uint8_t> bar_allowed;       // [G][A] the caller's masks
    std::vector<uint8_t> bar_has;           // [G] 1 where the game has a row in bar_allowed
    bool bar_pending = false;               // some bar_has is set
    bool bar_on_device = false;             // d_bar holds the next move's bar
    bool bar_dirty = false;                 // a root may hold kBarQ children: the next move passes the bar array (zeros, if no game
                                            // is barred) so that k_begin_move turns them back into unvisited children
    std::vector<uint8_t> used_allowed, used_has;
    bool used_pending = false, used_on_device = false;
    bool bar_keep = false;                  // the fp16-range recovery resets its games and sets their roots again: the bar stays
    // fp16-range recovery of ao_search: the games' MT19937 states as they were before the move (device copy), the host
    // half of the stream (legacy gauss cache), the number of recovered moves and of games searched again
    uint32_t* d_mt_backup = nullptr; int32_t* d_pos_backup = nullptr;
    std::vector<int32_t> has_gauss_backup; std::vector<double> gauss_backup;
    int64_t fp16_events = 0, fp16_games_redone = 0;
    int node_cap_auto = 0;           // 1: node_cap was derived from the free HBM (ao_config.node_cap == -1)
    // tree read-out (ao_tree_lookup / ao_tree_pv / ao_tree_stats): one device workspace, grown on demand, and its host mirror
    ao::DevBuf<unsigned char> d_ro{&pool};
    std::vector<unsigned char> h_ro;
    // HIP-event timing of the per-simulation tree kernel (k_expand_select) on the launch stream (ao_tree_timing)
    ao::EventTimer timer{256};
    RollState roll;
    // leaf symmetries (ao_set_leaf_symmetry): the seed most recently given to each game (never seeded: g), the keys made of
    // them -- or set one by one, ao_set_leaf_symmetry_keys -- and their device copy, which tp.sym_key names while the switch is on
    std::vector<uint32_t> sym_seed, sym_keys;
    uint32_t* d_sym_key = nullptr;
    bool sym_on = false;
    uint32_t sym_base = 0;
    // leaf tactics (ao_set_leaf_tactics): the solver's limits (lt_depth == 0: off), its stream and the two events of a launch
    // pair, the byte and the counters of every game; all made by the first call that switches it on
    int lt_depth = 0, lt_nodes = 0;
    hipStream_t lt_stream = nullptr;
    hipEvent_t lt_ready = nullptr, lt_done = nullptr;   // engine stream: the leaves are written; solver stream: the bytes are
    uint8_t* d_lt_proven = nullptr;                     // [G]
    int32_t* d_lt_counts = nullptr;                     // [G][4] searched, proven, out of nodes, nodes
    // proven outcomes (ao_tree_proofs, ao_set_proof_moves): the proof words' workspace and the root's edge values, made by the
    // first call that needs them (proofs_alloc); the switch, the verdicts of the last ao_end_move under it and the totals
    int32_t* d_pf_ws = nullptr;                         // [G][cap] a node's proof word, by arena node
    int32_t* d_pf_root = nullptr;                       // [G][4]
    int8_t* d_pf_status = nullptr;                      // [G][A]
    int16_t* d_pf_plies = nullptr;                      // [G][A]
    int32_t* d_pf_verdict = nullptr;                    // [G]
    bool proof_moves = false;
    std::vector<int32_t> pm_verdict;                    // [G]
    int64_t pm_totals[4] = {0, 0, 0, 0};
};

// The helpers that more than one of the engine's files calls; each is described where it is defined. They are in namespace ao, the
// namespace of ao_engine's base: a call with the engine as an argument finds them unqualified.
namespace ao {
// engine.hip
int roll_refuses(ao_engine* e, const char* who);
int roll_refuses_game(ao_engine* e, const char* who, int g);
int queue_refused(ao_engine* e, const char* who);
void clear_game_errors(ao_engine* e);
int report_game_errors(ao_engine* e, const int32_t* herr);
void draw_noise(ao_engine* e, const std::vector<std::pair<int32_t, size_t>>& draws);
int move_refused(ao_engine* e, const char* who, int g, const RollMove& m, const std::string& at_ply = "");
void settle_harvest(ao_engine* e, int* unfinished, int* owed);
int bar_forget(ao_engine* e, const uint8_t* mask);
int bar_build(ao_engine* e, const std::vector<uint8_t>& act, bool* any, const char* who);
// roll.hip: what ao_destroy leaves to the rolling search -- the solver's stream and events, the pinned rows
void roll_destroy(ao_engine* e);
// tree_readout.hip: the read-out workspace (d_ro / h_ro) of at least `bytes`, and the per-game mask a read-out kernel takes
int readout_begin(ao_engine* e, const char* who, size_t bytes);
void readout_mask(const ao_engine* e, const uint8_t* mask, uint8_t* out);
// tree_proofs.hip: the proof buffers, made by the first call that needs them
int proofs_alloc(ao_engine* e);
}  // namespace ao
