// roll_schedule.hpp -- the host rules of the moves a game makes one after the other: roll_next_move, what the move a game
// begins is (budget, target, noise, refusals), is the rule of BOTH drivers: ao_begin_move* / ao_search* ask it once per game and
// call, the rolling search (ao_roll_*) per game and turn. The rest is the rolling search's own: which games are turned (their
// move ended, played, the next one begun) while the others go on searching, when a run call returns, what draining means, and
// in which order looks, launches and turns follow each other. No HIP, no engine: plain C++17, tested on the host
// (tests/host/roll_schedule_main.cpp).
#pragma once
#include <algorithm>
#include <cstdint>

namespace ao {

// ---- who turns ------------------------------------------------------------------------------------------------------------------
// A game is turned when it is in a move, has run exactly its target and has no leaf under way (a settled game's pending leaf is
// backed up by the launch behind the look, after which done == target). done != target in a turned game would be ERR_SHORT.
inline bool roll_turns(bool in_move, int done, int target, bool leaf_idle) { return in_move && leaf_idle && done == target; }

// ---- the next move of a game ----------------------------------------------------------------------------------------------------
// the column of a by-ply table row of `stride` entries: plies beyond the table read its last column
inline int roll_ply_column(int ply, int stride) { return std::min(ply, stride - 1); }

// refuse: 0 the move can begin; 1 the budget is outside 1..S; 2 noise asked for on an engine created without noise
struct RollMove { int tau, budget, target, gflags, draw, refuse; };

// ply: moves on the board; tau_plies: tau is 1 for the first tau_plies moves of the game (negative: always); sims_row /
// noise_row: the game's rows of the by-ply tables (null: the engine's S / the engine's noise); root_status: AO_ROOT_* of the
// position (0 fresh, 1 known, 2 expanded). target counts a fresh root's own expansion; gflags are TreeParams::gflags (bit 0:
// re-noise the inherited root when the move begins, bit 1: no noise at this move's root); draw: the game's stream pays for a
// Dirichlet draw before the move. (ao_begin_move_opts passes its one budget and its one switch per game as rows of stride 1
// and tau_plies = -1: its tau arrives with ao_end_move.)
inline RollMove roll_next_move(int ply, int tau_plies, const int32_t* sims_row, int sims_stride, const uint8_t* noise_row,
                               int noise_stride, bool engine_noise, int S, int root_status) {
    RollMove m{};
    m.tau = (tau_plies < 0 || ply < tau_plies) ? 1 : 0;
    m.budget = sims_row ? sims_row[roll_ply_column(ply, sims_stride)] : S;
    const bool wants = noise_row ? noise_row[roll_ply_column(ply, noise_stride)] != 0 : engine_noise;
    if (m.budget < 1 || m.budget > S) m.refuse = 1;
    else if (wants && !engine_noise) m.refuse = 2;
    m.target = m.budget + (root_status == 0 ? 1 : 0);
    const bool quiet = engine_noise && !wants;      // this game, this move: as on an engine created without noise
    m.gflags = quiet ? 2 : ((engine_noise && root_status == 2) ? 1 : 0);
    m.draw = (engine_noise && !quiet) ? 1 : 0;
    return m;
}

// ---- tactics beside the loop (ao_roll_set_tactics) ------------------------------------------------------------------------------
// With the forced-win solver armed a game that is to begin a move first WAITS for the solver's verdict on its root: the solver
// runs in batches on a stream of its own while the other games go on searching. A game of an open roll is in one of three states;
// "in a move" for ao_reset / ao_seed* / ao_roll_end is everything but ROLL_OUT.
enum RollGame : uint8_t { ROLL_OUT = 0, ROLL_SEARCHING = 1, ROLL_WAITING = 2 };

// A waiting game is never turned, whatever its counters say: done == target is left over from the move it just played.
inline bool roll_game_turns(int state, int done, int target, bool leaf_idle) {
    return roll_turns(state == ROLL_SEARCHING, done, target, leaf_idle);
}

// The budget of a move whose root the solver has looked at: a proven win (verdict 1, RT_WIN) is capped at solved_sims
// simulations; solved_sims == 0 is no cap; every other verdict leaves the budget alone. One rule for the host (ao_search's
// callers, the tests) and the device (k_roll_begin works out the target of a game from the verdict words of its batch).
#if defined(__HIPCC__)
#define AO_ROLL_HD __host__ __device__
#else
#define AO_ROLL_HD
#endif
AO_ROLL_HD inline int roll_solved_budget(int budget, int verdict, int solved_sims) {
    return (verdict == 1 && solved_sims > 0 && solved_sims < budget) ? solved_sims : budget;
}

// The ring of solver batches. A batch is started at a turn (or at begin / join) and asked about at every LATER turn, oldest
// first: `age` counts the turns since it was started. Its games begin their move once its event has been reached and it has been
// held for `hold` further turns (AO_ROLL_TACTICS_HOLD, a test knob; 0: none) -- or at once when the host had to block on it.
inline bool roll_batch_begins(bool event_done, int age, int hold, bool blocked) {
    return blocked || (event_done && age >= 1 + hold);
}
// The host blocks on the OLDEST batch's event when a batch is to be started and every slot is busy, or when nothing is searching
// and a batch is pending (the loop would launch empty batches until the verdict arrives).
inline bool roll_must_block(int busy_slots, int slots, bool starts_batch, int searching, int pending) {
    return (starts_batch && busy_slots >= slots) || (searching == 0 && pending > 0);
}
constexpr int kRollBatchSlots = 4;

// ---- drain ----------------------------------------------------------------------------------------------------------------------
// a turned game begins another move unless its game is over or the roll is draining
inline bool roll_begins_next(int win, bool draining) { return win == 0 && !draining; }

// ---- when a run call returns ----------------------------------------------------------------------------------------------------
// asked behind every turn (records: what it produced) and behind every launch that no turn follows (records = 0):
// at least one record; nothing in a move any more; the launch bound (0: none) is spent
inline bool roll_run_returns(int records, int in_move, int64_t launches, int64_t max_launches) {
    return records > 0 || in_move == 0 || (max_launches > 0 && launches >= max_launches);
}

// ---- look / launch / turn -------------------------------------------------------------------------------------------------------
// A period is turn_every launches and one turn. With early stop the look (k_settle) stands in front of the period's LAST launch:
// that launch backs up the leaf a settled game still had under way, the turn behind it ends the game's move and begins the next,
// and the launch after the turn selects the new move's first leaf -- a settled game idles in no launch.
enum RollStep { ROLL_LAUNCH = 0, ROLL_LOOK = 1, ROLL_TURN = 2 };
struct RollCadence {
    int turn_every = 1;
    bool early = false;
    int since = 0;         // launches since the last turn
    bool looked = false;   // this period's look has been queued
    bool turn_due() const { return since >= turn_every; }
    RollStep next() {      // the next step, taken
        if (turn_due()) { since = 0; looked = false; return ROLL_TURN; }
        if (early && !looked && since == turn_every - 1) { looked = true; return ROLL_LOOK; }
        ++since;
        return ROLL_LAUNCH;
    }
};

}  // namespace ao
