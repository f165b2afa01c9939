// roll.hip -- the rolling search (ao_roll_*): its kernels, then its host driver. The device side is a TURN for a compact list of
// games while the others are mid-search in the same launch loop. Every kernel is one wavefront per LISTED game and touches that
// game's state only; what the host reads and writes per turn is O(listed games). The state (RollState, RollTactics, RollBatch)
// is engine.hpp's, the rules are roll_schedule.hpp's.
//
//   k_roll_turn     end of move + play of a listed game, in one wave: end_move_game then play_game (move_device.hpp -- the
//                   bodies of k_end_move and k_play) on ONE open stream, so the tie-break draw (tau == 0) and the action draw
//                   come in the order and from the words that k_end_move followed by k_play take them. The result is a
//                   compact record: eight words, the game's error word among them, + pi[A] (+ visit[A], policy[A]).
//                   k_reroot (tree_kernels.hip) follows with the same list.
//   k_roll_gather   the listed games' MT19937 states into compact rows (the host draws their Dirichlet noise: host_rng.hpp)
//   k_roll_begin    the states and the noise rows back, then the begin of the next move: targets, flags, tau, the settle
//                   mask, and begin_move_game (the body of k_begin_move: re-noise of an inherited root)
//   k_roll_mask     the games a look may settle: early-stop games that have run a simulation of their move
// With the forced-win solver beside the loop (ao_roll_set_tactics; root_tactics.hip runs on a stream of its own, on a batch's rows):
//   k_roll_rootpos  the listed games' root positions into the batch's compact rows: the solver reads nothing of the engine
//   k_roll_verdict  in front of k_roll_begin, for the games of a finished batch: the bar row of the move into TreeParams::bar, the
//                   verdict words (and the allowed row) into the game's own row, and the target of the begin item from the verdict
//                   (roll_solved_budget, roll_schedule.hpp)
//   k_roll_words    the verdict words (and allowed rows) of the turned games into compact rows, for their records
#include <algorithm>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "engine.hpp"
#include "launchers.hpp"
#include "move_device.hpp"
#include "tactics_limits.hpp"

namespace ao {

constexpr int kRollRec = 8;    // words of a turn record: game, action (-1: short of its simulations), win, tau, simulations done, settled, AO_ROOT_* of the new root, the game's error word behind the turn (0: none)
constexpr int kRollItem = 6;   // words of a begin item: game, target, gflags, tau, settle mask, row of its stream and noise in the compact buffers (-1: no draw)

template <int NCH>
__global__ __launch_bounds__(64) void k_roll_turn(TreeParams p, const int32_t* games, uint8_t* active, const uint8_t* settled,
                                                  int32_t* rec, double* rec_pi, double* rec_visit, double* rec_policy) {
    __shared__ uint32_t s_mt[624];
    __shared__ int s_vis[256];
    __shared__ double s_pol[256];
    __shared__ double s_pi[256];
    __shared__ double s_cdf[256];
    const int b = blockIdx.x;
    const int g = games[b];
    const int lane = lane_id();
    const int tau = p.tau[g];
    const int done = p.sims_done[g];
    const size_t row = static_cast<size_t>(b) * p.A;
    int32_t* r = rec + static_cast<size_t>(b) * kRollRec;
    MtDev mt;
    mt.open(p.mt + static_cast<size_t>(g) * 624, p.mtpos + g, s_mt);   // (reads only: a short game's stream stays untouched)
    const bool ok = end_move_game<NCH>(p, g, tau, &mt, s_mt, s_vis, s_pol, rec_pi + row, rec_visit ? rec_visit + row : nullptr,
                                       rec_policy ? rec_policy + row : nullptr, s_pi);
    if (!ok) {                                                          // (uniform over the wave) ERR_SHORT is set: the host fails the call
        if (lane == 0) { r[0] = g; r[1] = -1; r[2] = 0; r[3] = tau; r[4] = done; r[5] = 0; r[6] = 0; r[7] = atomicOr(&p.err[g], 0); }
        return;
    }
    __syncthreads();                                                    // s_pi is read by lane 0
    const Played pl = play_game<NCH>(p, g, s_pi, &mt, s_mt, s_cdf);
    mt.close();
    if (lane == 0) {
        // (word 7: the game's error word behind its turn -- lane 0 set ERR_BAD_MOVE itself, in play_game)
        r[0] = g; r[1] = pl.action; r[2] = pl.win; r[3] = tau; r[4] = done; r[5] = settled[g]; r[6] = pl.status; r[7] = atomicOr(&p.err[g], 0);
        active[g] = 0;                                                  // outside a move until k_roll_begin
    }
}

// 624 words = 156 x 16 B per row, rows 16-byte aligned on both sides
__device__ __forceinline__ void copy_mt_row(uint32_t* dst, const uint32_t* src) {
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    uint4* d4 = reinterpret_cast<uint4*>(dst);
    for (int i = lane_id(); i < 156; i += 64) d4[i] = s4[i];
}

__global__ __launch_bounds__(64) void k_roll_gather(TreeParams p, const int32_t* games, uint32_t* out_mt, int32_t* out_pos) {
    const int b = blockIdx.x;
    const int g = games[b];
    copy_mt_row(out_mt + static_cast<size_t>(b) * 624, p.mt + static_cast<size_t>(g) * 624);
    if (lane_id() == 0) out_pos[b] = p.mtpos[g];
}

// items [n][kRollItem]: game, target, gflags, tau, settle mask, row of the game in in_mt / in_pos / in_noise (-1: no draw)
template <int NCH>
__global__ __launch_bounds__(64) void k_roll_begin(TreeParams p, const int32_t* items, const uint32_t* in_mt, const int32_t* in_pos,
                                                   const double* in_noise, int8_t* tau, uint8_t* active, uint8_t* settled, uint8_t* early) {
    const int32_t* it = items + static_cast<size_t>(blockIdx.x) * kRollItem;
    const int g = it[0];
    const int gflags = it[2];
    const int src = it[5];
    const int lane = lane_id();
    if (src >= 0) {                                                     // (uniform over the wave)
        copy_mt_row(p.mt + static_cast<size_t>(g) * 624, in_mt + static_cast<size_t>(src) * 624);
        // lane l writes the entries l, l + 64, ... of the noise row: the ones it reads again in begin_move_game
        for (int i = lane; i < p.Ap; i += 64) p.noise_buf[static_cast<size_t>(g) * p.Ap + i] = in_noise[static_cast<size_t>(src) * p.Ap + i];
    }
    if (lane == 0) {
        if (src >= 0) p.mtpos[g] = in_pos[src];
        p.sims_target[g] = it[1];
        p.gflags[g] = gflags;
        tau[g] = static_cast<int8_t>(it[3]);
        early[g] = static_cast<uint8_t>(it[4]);
        settled[g] = 0;
        active[g] = 1;
    }
    begin_move_game<NCH>(p, g, (gflags & 1) != 0);
}

// A look settles a game on the visits of ITS move: a game that has not finished a simulation of the move yet (its counts are all
// inherited) waits for the next look, as in ao_search_opts, whose first look comes after settle_every simulations.
__global__ void k_roll_mask(TreeParams p, const uint8_t* early, uint8_t* out) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < p.G) out[g] = (early[g] && p.sims_done[g] >= 1) ? 1 : 0;
}

__global__ __launch_bounds__(64) void k_roll_rootpos(TreeParams p, const int32_t* games, Pos* rows) {
    static_assert(sizeof(Pos) % 4 == 0, "a position row is copied in words");
    const int g = __builtin_amdgcn_readfirstlane(games[blockIdx.x]);
    const uint32_t* src = reinterpret_cast<const uint32_t*>(p.rootpos + g);
    uint32_t* dst = reinterpret_cast<uint32_t*>(rows + blockIdx.x);
    for (int i = lane_id(); i < static_cast<int>(sizeof(Pos) / 4); i += 64) dst[i] = src[i];
}

// Item k of `items` is the begin item of the game in row k of the batch. Word 4 carries the settle mask in bit 0 and, in bit 1,
// whether the target counts a fresh root's own expansion on top of the budget: the cap of a proven win applies to the budget.
__global__ __launch_bounds__(64) void k_roll_verdict(int32_t* items, RollBatchView b, int A, int solved_sims, uint64_t* bar, int32_t* game_words,
                                                     uint8_t* game_allowed) {
    const int k = blockIdx.x;
    int32_t* it = items + static_cast<size_t>(k) * kRollItem;
    const int g = __builtin_amdgcn_readfirstlane(it[0]);
    const int lane = lane_id();
    if (lane < kBBWords) bar[static_cast<size_t>(g) * kBBWords + lane] = b.bar[static_cast<size_t>(k) * kBBWords + lane];
    if (lane < 4) game_words[static_cast<size_t>(g) * 4 + lane] = b.verdict[static_cast<size_t>(lane) * b.n + k];
    if (game_allowed)                                                   // (uniform over the wave)
        for (int i = lane; i < A; i += 64) game_allowed[static_cast<size_t>(g) * A + i] = b.allowed[static_cast<size_t>(k) * A + i];
    if (lane == 0) {
        const int bonus = (it[4] >> 1) & 1;
        it[1] = roll_solved_budget(it[1] - bonus, b.verdict[k], solved_sims) + bonus;
        it[4] &= 1;
    }
}

__global__ __launch_bounds__(64) void k_roll_words(const int32_t* games, int A, const int32_t* game_words, const uint8_t* game_allowed,
                                                   int32_t* out_words, uint8_t* out_allowed) {
    const int b = blockIdx.x;
    const int g = __builtin_amdgcn_readfirstlane(games[b]);
    const int lane = lane_id();
    if (lane < 4) out_words[static_cast<size_t>(b) * 4 + lane] = game_words[static_cast<size_t>(g) * 4 + lane];
    if (out_allowed)                                                    // (uniform over the wave)
        for (int i = lane; i < A; i += 64) out_allowed[static_cast<size_t>(b) * A + i] = game_allowed[static_cast<size_t>(g) * A + i];
}

// ----------------------------------------------------------------------------------------------
// launchers: a turn of the rolling search for a compact list of n games (one wave per listed game)
// ----------------------------------------------------------------------------------------------
static void launch_roll_rootpos(const TreeParams& p, const int32_t* games, int n, Pos* rows, hipStream_t s) {
    hipLaunchKernelGGL(k_roll_rootpos, dim3(n), dim3(64), 0, s, p, games, rows);
}
static void launch_roll_verdict(int32_t* items, const RollBatchView& b, int A, int solved_sims, uint64_t* bar, int32_t* game_words,
                                uint8_t* game_allowed, hipStream_t s) {
    hipLaunchKernelGGL(k_roll_verdict, dim3(b.n), dim3(64), 0, s, items, b, A, solved_sims, bar, game_words, game_allowed);
}
static void launch_roll_words(const int32_t* games, int n, int A, const int32_t* game_words, const uint8_t* game_allowed, int32_t* out_words,
                              uint8_t* out_allowed, hipStream_t s) {
    hipLaunchKernelGGL(k_roll_words, dim3(n), dim3(64), 0, s, games, A, game_words, game_allowed, out_words, out_allowed);
}
static void launch_roll_turn(const TreeParams& p, const int32_t* games, int n, uint8_t* active, const uint8_t* settled, int32_t* rec,
                             double* rec_pi, double* rec_visit, double* rec_policy, hipStream_t s) {
    AO_DISPATCH_NCH(nch_of_cells(p.A), hipLaunchKernelGGL(k_roll_turn<NCH>, dim3(n), dim3(64), 0, s, p, games, active, settled, rec, rec_pi,
                                                          rec_visit, rec_policy));
}
static void launch_roll_gather(const TreeParams& p, const int32_t* games, int n, uint32_t* out_mt, int32_t* out_pos, hipStream_t s) {
    hipLaunchKernelGGL(k_roll_gather, dim3(n), dim3(64), 0, s, p, games, out_mt, out_pos);
}
static void launch_roll_begin(const TreeParams& p, const int32_t* items, int n, const uint32_t* in_mt, const int32_t* in_pos,
                              const double* in_noise, int8_t* tau, uint8_t* active, uint8_t* settled, uint8_t* early, hipStream_t s) {
    AO_DISPATCH_NCH(nch_of_cells(p.A), hipLaunchKernelGGL(k_roll_begin<NCH>, dim3(n), dim3(64), 0, s, p, items, in_mt, in_pos, in_noise, tau,
                                                          active, settled, early));
}
static void launch_roll_mask(const TreeParams& p, const uint8_t* early, uint8_t* out, hipStream_t s) {
    hipLaunchKernelGGL(k_roll_mask, dim3((p.G + 255) / 256), dim3(256), 0, s, p, early, out);
}

// (before any buffer of the engine goes: a batch may still be running)
void roll_destroy(ao_engine* e) {
    RollTactics& t = e->roll.tac;
    if (t.stream) {
        hipStreamSynchronize(t.stream);
        for (RollBatch& b : t.slot) {
            if (b.ready) hipEventDestroy(b.ready);
            if (b.done) hipEventDestroy(b.done);
        }
        hipStreamDestroy(t.stream);
    }
    if (t.h_words) hipHostFree(t.h_words);
    if (t.h_allowed) hipHostFree(t.h_allowed);
    if (e->roll.h_i32) hipHostFree(e->roll.h_i32);
}

}  // namespace ao

// ---- the host driver ---------------------------------------------------------------------------
// ao_search moves every game of the engine through one move per call: the launch loop of a move lasts until its LAST game has its
// simulations. Here the launch loop never stops for a move: every turn_every launches the games that have their simulations are
// TURNED -- move ended and played (k_roll_turn, k_reroot), the next one begun (k_roll_begin) -- while the others are mid-search
// in the same launches. A game's search stays strictly sequential: the records equal ao_search + ao_play of that game to the bit.
// Which games turn, what their next move is, when a run returns and the order of looks, launches and turns: roll_schedule.hpp.
static void roll_count(ao_engine* e, size_t bytes) { e->roll.bytes += static_cast<int64_t>(bytes); }

// every way out of a roll, the failures included: no game is in a move and the engine is between moves
static void roll_close(ao_engine* e) {
    RollState& r = e->roll;
    if (r.tac.on) {   // the solver's stream first: no batch runs on when the buffers are reused; roots may hold the sentinels of a bar
        (void)hipStreamSynchronize(r.tac.stream);
        for (RollBatch& b : r.tac.slot) b.busy = false;
        r.tac.pending.clear();
        r.tac.n_waiting = 0;
        r.tac.on = false;
        e->bar_dirty = true;
    }
    r.open = false;
    r.draining = false;
    std::fill(r.in_move.begin(), r.in_move.end(), 0);
    r.n_in_move = 0;
    e->in_move = false;
    e->ended = false;
}

// what a failure inside the loop leaves behind: error words cleared, the roll closed (check_game_errors does the same for its own)
static int roll_fail(ao_engine* e, const std::string& m) {
    clear_game_errors(e);
    roll_close(e);
    return e->fail(m);
}

// Takes the per-game fields of `o` for the games of `act` into the roll's tables -- after every column of theirs has been found in
// range: a refused call has touched nothing. fresh: the tables of a roll that begins (what an earlier roll left is dropped).
static int roll_take_tables(ao_engine* e, const ao_roll_opts* o, const std::vector<uint8_t>& act, bool fresh, const char* who) {
    RollState& r = e->roll;
    const int G = e->G;
    if (o->sims && o->sims_stride < 1) return e->fail(std::string(who) + ": sims_stride must be >= 1");
    if (o->noise && o->noise_stride < 1) return e->fail(std::string(who) + ": noise_stride must be >= 1");
    if (!fresh && o->sims && !r.sims.empty() && o->sims_stride != r.sims_stride) return e->fail(std::string(who) + ": sims_stride differs from the open roll's");
    if (!fresh && o->noise && !r.noise.empty() && o->noise_stride != r.noise_stride) return e->fail(std::string(who) + ": noise_stride differs from the open roll's");
    for (int g = 0; g < G; ++g) {
        if (!act[g]) continue;
        const int cols = std::max(o->sims ? o->sims_stride : 1, o->noise ? o->noise_stride : 1);
        for (int c = 0; c < cols; ++c) {
            const ao::RollMove m = ao::roll_next_move(c, -1, o->sims ? o->sims + static_cast<size_t>(g) * o->sims_stride : nullptr, o->sims_stride,
                                                      o->noise ? o->noise + static_cast<size_t>(g) * o->noise_stride : nullptr, o->noise_stride,
                                                      e->tp.noise != 0, e->S, AO_ROOT_EXPANDED);
            if (move_refused(e, who, g, m, " at ply " + std::to_string(c))) return 1;
        }
    }
    if (fresh) {
        r.tau_plies.clear(); r.sims.clear(); r.noise.clear();
        r.sims_stride = r.noise_stride = 0;
    }
    if (o->tau_plies && r.tau_plies.empty()) r.tau_plies.assign(G, -1);
    if (o->sims && r.sims.empty()) { r.sims_stride = o->sims_stride; r.sims.assign(static_cast<size_t>(G) * r.sims_stride, e->S); }
    if (o->noise && r.noise.empty()) { r.noise_stride = o->noise_stride; r.noise.assign(static_cast<size_t>(G) * r.noise_stride, e->tp.noise ? 1 : 0); }
    for (int g = 0; g < G; ++g) {
        if (!act[g]) continue;
        if (o->tau_plies) r.tau_plies[g] = std::max(o->tau_plies[g], 0);
        if (o->sims) std::copy(o->sims + static_cast<size_t>(g) * r.sims_stride, o->sims + static_cast<size_t>(g + 1) * r.sims_stride, r.sims.begin() + static_cast<size_t>(g) * r.sims_stride);
        if (o->noise) std::copy(o->noise + static_cast<size_t>(g) * r.noise_stride, o->noise + static_cast<size_t>(g + 1) * r.noise_stride, r.noise.begin() + static_cast<size_t>(g) * r.noise_stride);
    }
    return 0;
}

// Begins the next move of the listed games (not in a move, not over). rows: where game games[k]'s stream lies in the compact
// staging rows (h_mt / h_pos, gathered by the turn that just played it), or null: the streams are gathered here. The Dirichlet
// draw of the games that search with noise is the host's (host_rng.hpp), on the pool; everything travels in compact rows.
// batches (with the solver beside the loop): the games are those of the listed finished batches, in order, and were waiting;
// k_roll_verdict takes each batch's bar rows and verdicts to its games in front of k_roll_begin.
static int roll_begin_games(ao_engine* e, const std::vector<int32_t>& games, const int32_t* rows, const std::vector<int>* batches = nullptr) {
    RollState& r = e->roll;
    const int n = static_cast<int>(games.size()), G = e->G, Ap = e->Ap;
    if (n == 0) return 0;
    int32_t* h_games = r.h_i32 + 4 * static_cast<size_t>(G);
    int32_t* h_items = h_games + G;
    std::vector<ao::RollMove> mv(n);
    bool any_draw = false;
    for (int k = 0; k < n; ++k) {   // the move each game begins now (roll_schedule.hpp), from the roll's tables and the host mirrors
        const int g = games[k];
        mv[k] = ao::roll_next_move(static_cast<int>(e->moves[g].size()), r.tau_plies.empty() ? -1 : r.tau_plies[g],
                                   r.sims.empty() ? nullptr : r.sims.data() + static_cast<size_t>(g) * r.sims_stride, r.sims_stride,
                                   r.noise.empty() ? nullptr : r.noise.data() + static_cast<size_t>(g) * r.noise_stride, r.noise_stride,
                                   e->tp.noise != 0, e->S, e->status[g]);
        any_draw = any_draw || mv[k].draw;
    }
    if (!rows) {
        AO_HIP(e, hipStreamSynchronize(e->stream));   // (the pinned staging rows are free)
        if (any_draw) {
            std::copy(games.begin(), games.end(), h_games);
            AO_HIP(e, hipMemcpyAsync(r.d_games, h_games, sizeof(int32_t) * n, hipMemcpyHostToDevice, e->stream));
            ao::launch_roll_gather(e->tp, r.d_games, n, e->d_mt_backup, e->d_pos_backup, e->stream);
            AO_HIP(e, hipGetLastError());
            AO_HIP(e, hipMemcpyAsync(e->h_mt, e->d_mt_backup, sizeof(uint32_t) * 624 * n, hipMemcpyDeviceToHost, e->stream));
            AO_HIP(e, hipMemcpyAsync(e->h_pos, e->d_pos_backup, sizeof(int32_t) * n, hipMemcpyDeviceToHost, e->stream));
            AO_HIP(e, hipStreamSynchronize(e->stream));
            roll_count(e, static_cast<size_t>(n) * (4 + 624 * 4 + 4));
        }
    }
    int nrows = 0;   // staging rows in use: [0, nrows)
    std::vector<std::pair<int32_t, size_t>> draws;   // (no draw for a game without noise: its stream is not touched)
    for (int k = 0; k < n; ++k) {
        const int g = games[k];
        const int row = rows ? rows[k] : k;
        int32_t* it = h_items + static_cast<size_t>(k) * ao::kRollItem;
        it[0] = g; it[1] = mv[k].target; it[2] = mv[k].gflags; it[3] = mv[k].tau;
        it[4] = (r.early && mv[k].tau == 0) ? 1 : 0;
        if (batches && mv[k].target != mv[k].budget) it[4] |= 2;   // (k_roll_verdict caps the budget, not the root's own expansion)
        it[5] = mv[k].draw ? row : -1;
        if (mv[k].draw) {
            nrows = std::max(nrows, row + 1);
            draws.emplace_back(g, row);
        }
    }
    if (any_draw) {
        draw_noise(e, draws);
        AO_HIP(e, hipMemcpyAsync(e->d_mt_backup, e->h_mt, sizeof(uint32_t) * 624 * nrows, hipMemcpyHostToDevice, e->stream));
        AO_HIP(e, hipMemcpyAsync(e->d_pos_backup, e->h_pos, sizeof(int32_t) * nrows, hipMemcpyHostToDevice, e->stream));
        AO_HIP(e, hipMemcpyAsync(r.d_noise, e->h_noise, sizeof(double) * Ap * nrows, hipMemcpyHostToDevice, e->stream));
        roll_count(e, static_cast<size_t>(nrows) * (624 * 4 + 4 + sizeof(double) * Ap));
    }
    AO_HIP(e, hipMemcpyAsync(r.d_items, h_items, sizeof(int32_t) * ao::kRollItem * n, hipMemcpyHostToDevice, e->stream));
    roll_count(e, sizeof(int32_t) * ao::kRollItem * n);
    if (batches) {
        RollTactics& t = r.tac;
        size_t at = 0;
        for (int i : *batches) {
            RollBatch& b = t.slot[i];
            AO_HIP(e, hipStreamWaitEvent(e->stream, b.done, 0));   // (reached already: the host saw it, or waited for it)
            ao::launch_roll_verdict(r.d_items + at * ao::kRollItem, b.view, e->A, t.solved_sims, e->d_bar, t.d_words, t.d_allowed, e->stream);
            at += static_cast<size_t>(b.n);
        }
    }
    ao::launch_roll_begin(r.loop.p, r.d_items, n, e->d_mt_backup, e->d_pos_backup, r.d_noise, e->d_tau, e->d_active, e->d_settled, e->d_early, e->stream);
    AO_HIP(e, hipGetLastError());
    e->settled_dirty = true;
    for (int k = 0; k < n; ++k) {
        const int g = games[k];
        e->bonus[g] = mv[k].target - mv[k].budget;
        e->active[g] = 1;
        if (r.in_move[g] == ao::ROLL_OUT) ++r.n_in_move;   // (a game that waited for its verdict has been in a move since it was listed)
        r.in_move[g] = ao::ROLL_SEARCHING;
    }
    return 0;
}

// ---- the solver beside the loop ----
// the batch's buffer for n games, carved up: the solver's RootTacticsBufs, the position rows, the games; *view: what k_roll_verdict reads
static int roll_batch_layout(ao_engine* e, RollBatch& b, int n, ao::RootTacticsBufs* bufs, ao::Pos** rows) {
    RollTactics& t = e->roll.tac;
    const size_t N = static_cast<size_t>(n), A = static_cast<size_t>(e->A);
    auto up = [](size_t x) { return (x + 15) & ~static_cast<size_t>(15); };
    const size_t at_pos = 0, at_won = up(at_pos + N * sizeof(ao::Pos)), at_bar = up(at_won + N * ao::kBBWords * 8), at_stage = up(at_bar + N * ao::kBBWords * 8),
                 at_pair = up(at_stage + N * 8), at_words = up(at_pair + N * A * 4), at_allowed = up(at_words + N * 16),
                 bytes = at_allowed + (t.want_allowed ? N * A : 0);
    if (!b.buf.p || bytes > b.buf.n) {   // (grows: the slot's last batch was read by kernels queued on the engine's stream)
        AO_HIP(e, hipStreamSynchronize(e->stream));
        b.buf.pool = &e->pool;
        if (b.buf.reserve(e, bytes)) return 1;
    }
    unsigned char* p = b.buf.p;
    *rows = reinterpret_cast<ao::Pos*>(p + at_pos);
    *bufs = ao::RootTacticsBufs{};
    bufs->won = reinterpret_cast<uint64_t*>(p + at_won);
    bufs->bar = reinterpret_cast<uint64_t*>(p + at_bar);
    bufs->stage = reinterpret_cast<uint32_t*>(p + at_stage);
    bufs->pair = reinterpret_cast<uint32_t*>(p + at_pair);
    bufs->verdict = reinterpret_cast<int32_t*>(p + at_words);
    bufs->depth = bufs->verdict + N; bufs->nodes = bufs->depth + N; bufs->unknown = bufs->nodes + N;
    bufs->allowed = t.want_allowed ? p + at_allowed : nullptr;
    b.view = ao::RollBatchView{bufs->bar, bufs->verdict, bufs->allowed, n};
    return 0;
}

// Starts a batch for the listed games in a free slot: their root positions into the batch's rows on the engine's stream, the
// three solver launches behind an event on the solver's. streams: the games' MT19937 states and positions ([n][624], [n]) as the
// host holds them now -- the Dirichlet draw of the move comes from them when the batch's games begin.
static int roll_batch_start(ao_engine* e, const std::vector<int32_t>& games, std::vector<uint32_t>&& mt, std::vector<int32_t>&& pos) {
    RollState& r = e->roll;
    RollTactics& t = r.tac;
    const int n = static_cast<int>(games.size());
    int i = 0;
    while (i < ao::kRollBatchSlots && t.slot[i].busy) ++i;
    if (i == ao::kRollBatchSlots) return e->fail("ao_roll: no free solver batch slot");   // (roll_must_block keeps one free)
    RollBatch& b = t.slot[i];
    ao::RootTacticsBufs bufs;
    ao::Pos* rows = nullptr;
    if (roll_batch_layout(e, b, n, &bufs, &rows)) return 1;
    if (!b.ready) {
        AO_HIP(e, hipEventCreateWithFlags(&b.ready, hipEventDisableTiming));
        AO_HIP(e, hipEventCreateWithFlags(&b.done, hipEventDisableTiming));
    }
    b.games = games;
    b.mt = std::move(mt);
    b.pos = std::move(pos);
    b.n = n;
    b.age = 0;
    // (d_games is free: whatever listed these games -- a turn, a begin, a join -- has synchronised behind its last use)
    AO_HIP(e, hipMemcpyAsync(r.d_games, b.games.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, e->stream));
    ao::launch_roll_rootpos(e->tp, r.d_games, n, rows, e->stream);
    AO_HIP(e, hipGetLastError());
    AO_HIP(e, hipEventRecord(b.ready, e->stream));
    AO_HIP(e, hipStreamWaitEvent(t.stream, b.ready, 0));
    AO_HIP(e, hipMemsetAsync(bufs.bar, 0, sizeof(uint64_t) * ao::kBBWords * n, t.stream));   // (no caller's bar under rolling)
    ao::launch_root_tactics_rows(rows, n, e->tp.B, e->A, e->tp.win_mark, t.max_depth, t.max_nodes, bufs, t.stream);
    AO_HIP(e, hipGetLastError());
    AO_HIP(e, hipEventRecord(b.done, t.stream));
    b.busy = true;
    t.pending.push_back(i);
    for (int g : games) {
        if (r.in_move[g] == ao::ROLL_OUT) ++r.n_in_move;
        r.in_move[g] = ao::ROLL_WAITING;
    }
    t.n_waiting += n;
    t.stats[0] += 1;
    t.stats[5] += static_cast<int64_t>(sizeof(int32_t)) * n;
    roll_count(e, sizeof(int32_t) * n);
    return 0;
}

// The games of the taken batches begin their move, in one k_roll_begin: their streams go back into the staging rows first.
static int roll_batches_begin(ao_engine* e, const std::vector<int>& taken) {
    RollTactics& t = e->roll.tac;
    if (taken.empty()) return 0;
    std::vector<int32_t> games, rows;
    for (int i : taken) {
        RollBatch& b = t.slot[i];
        for (int k = 0; k < b.n; ++k) {
            const size_t row = games.size();
            if (!b.mt.empty()) {
                std::memcpy(e->h_mt + row * 624, b.mt.data() + static_cast<size_t>(k) * 624, sizeof(uint32_t) * 624);
                e->h_pos[row] = b.pos[k];
            }
            games.push_back(b.games[k]);
            rows.push_back(static_cast<int32_t>(row));
        }
    }
    const int rc = roll_begin_games(e, games, rows.data(), &taken);
    for (int i : taken) {
        t.slot[i].busy = false;
        t.n_waiting -= t.slot[i].n;
        t.stats[1] += t.slot[i].n;
    }
    return rc;
}

// What a turn (at_turn), a begin or a join does about the solver once it knows which games are to begin a move (`next`; rows:
// where their streams lie in the staging rows, or null: they are gathered here). The order matters: the streams of `next` leave
// the staging rows first; the batches whose verdicts are in begin their games (which uses the staging rows, and reads the
// batches' buffers on the engine's stream); only then does the new batch take a slot. The engine's stream has been synchronised
// by the caller. The host waits for nothing but the oldest batch's recorded event, and only where roll_must_block says so.
static int roll_tactics_step(ao_engine* e, const std::vector<int32_t>& next, const int32_t* rows, bool at_turn) {
    RollState& r = e->roll;
    RollTactics& t = r.tac;
    const int n = static_cast<int>(next.size());
    std::vector<uint32_t> mt;
    std::vector<int32_t> pos;
    if (!at_turn) AO_HIP(e, hipStreamSynchronize(e->stream));   // (the pinned staging rows are free)
    if (n > 0 && e->tp.noise != 0) {
        if (!rows) {
            int32_t* h_games = r.h_i32 + 4 * static_cast<size_t>(e->G);
            std::copy(next.begin(), next.end(), h_games);
            AO_HIP(e, hipMemcpyAsync(r.d_games, h_games, sizeof(int32_t) * n, hipMemcpyHostToDevice, e->stream));
            ao::launch_roll_gather(e->tp, r.d_games, n, e->d_mt_backup, e->d_pos_backup, e->stream);
            AO_HIP(e, hipGetLastError());
            AO_HIP(e, hipMemcpyAsync(e->h_mt, e->d_mt_backup, sizeof(uint32_t) * 624 * n, hipMemcpyDeviceToHost, e->stream));
            AO_HIP(e, hipMemcpyAsync(e->h_pos, e->d_pos_backup, sizeof(int32_t) * n, hipMemcpyDeviceToHost, e->stream));
            AO_HIP(e, hipStreamSynchronize(e->stream));
            roll_count(e, static_cast<size_t>(n) * (4 + 624 * 4 + 4));
        }
        mt.resize(static_cast<size_t>(n) * 624);
        pos.resize(n);
        for (int k = 0; k < n; ++k) {
            const size_t row = rows ? rows[k] : k;
            std::memcpy(mt.data() + static_cast<size_t>(k) * 624, e->h_mt + row * 624, sizeof(uint32_t) * 624);
            pos[k] = e->h_pos[row];
        }
    }
    std::vector<int> taken;
    auto take_oldest = [&]() { taken.push_back(t.pending.front()); t.pending.erase(t.pending.begin()); };
    if (at_turn)
        for (int i : t.pending) { ++t.slot[i].age; t.stats[2] += t.slot[i].n; }
    const int searching = r.n_in_move - t.n_waiting;
    if (!t.pending.empty() && ao::roll_must_block(static_cast<int>(t.pending.size()), ao::kRollBatchSlots, n > 0, searching, static_cast<int>(t.pending.size()))) {
        AO_HIP(e, hipEventSynchronize(t.slot[t.pending.front()].done));
        ++t.stats[3];
        take_oldest();
    }
    while (at_turn && !t.pending.empty()) {
        const RollBatch& b = t.slot[t.pending.front()];
        const hipError_t q = hipEventQuery(b.done);
        if (q != hipSuccess && q != hipErrorNotReady) return e->fail(std::string("ao_roll: hipEventQuery: ") + hipGetErrorString(q));
        if (!ao::roll_batch_begins(q == hipSuccess, b.age, t.hold, false)) break;
        take_oldest();
    }
    if (roll_batches_begin(e, taken)) return 1;
    if (n == 0) return 0;
    if (roll_batch_start(e, next, std::move(mt), std::move(pos))) return 1;
    if (ao::roll_must_block(static_cast<int>(t.pending.size()), ao::kRollBatchSlots, false, r.n_in_move - t.n_waiting, static_cast<int>(t.pending.size()))) {
        // (nothing was pending before, or its games would be searching now: the staging rows are not in use)
        AO_HIP(e, hipEventSynchronize(t.slot[t.pending.front()].done));
        ++t.stats[3];
        taken.clear();
        take_oldest();
        if (roll_batches_begin(e, taken)) return 1;
    }
    return 0;
}

// the games of a begin / join: listed (null: all), not over; a listed game that is in a move already is refused by name
static int roll_listed(ao_engine* e, const uint8_t* active, std::vector<uint8_t>* act, const char* who) {
    act->assign(e->G, 0);
    for (int g = 0; g < e->G; ++g) {
        if ((active && !active[g]) || e->over[g]) continue;
        if (e->roll.open && e->roll.in_move[g]) {
            if (active) return e->fail(std::string(who) + ": game " + std::to_string(g) + " is in a move already");
            continue;
        }
        (*act)[g] = 1;
    }
    return 0;
}

// one launch of the loop: the network on the rows the last selection handed out, then expansion + backup and the next selection
static int roll_launch(ao_engine* e) {
    LaunchLoop& loop = e->roll.loop;
    if (loop.leaf_tactics(true)) return 1;
    if (ao::net_forward_il(e->roll.net, loop.net_in, loop.cap_rows, e->d_policy, e->d_value, e->stream, loop.in_kind, 7, loop.slot(loop.launch),
                           static_cast<unsigned>(loop.cap_rows)))
        return roll_fail(e, std::string("ao_roll_run: network forward failed: ") + ao_net_last_error(e->roll.net));
    if (loop.leaf_tactics(false)) return 1;
    const bool timed = e->timer.tick();   // (see ao_tree_timing)
    if (timed) e->timer.begin(e->stream);
    if (loop.advance()) return 1;
    ao::launch_expand_select(loop.p, e->stream);
    if (timed) e->timer.end(e->stream);
    AO_HIP(e, hipGetLastError());
    return 0;
}

// the look: k_settle over the early-stop games (tau == 0 moves) that have run a simulation of their move; a leaf is under way
static int roll_look(ao_engine* e) {
    RollState& r = e->roll;
    ao::launch_roll_mask(r.loop.p, e->d_early, e->d_mask, e->stream);
    AO_HIP(e, hipMemsetAsync(e->d_settle, 0, sizeof(int32_t) * 4, e->stream));
    ao::launch_settle(r.loop.p, e->d_mask, 0, 1, e->d_settled, e->d_settle, e->stream);
    AO_HIP(e, hipGetLastError());
    AO_HIP(e, hipMemcpyAsync(e->h_settle, e->d_settle, sizeof(int32_t) * 4, hipMemcpyDeviceToHost, e->stream));
    roll_count(e, sizeof(int32_t) * 4);
    r.look_pending = true;
    return 0;
}

// A turn. Reads the network's status word and the games' words first: on either kind of error no game is turned.
static int roll_turn(ao_engine* e, ao_roll_records* out) {
    RollState& r = e->roll;
    const int G = e->G, A = e->A;
    const int64_t bytes0 = r.bytes;
    int32_t nflags = 0;
    if (ao_net_status(r.net, e->stream, &nflags, 1)) return roll_fail(e, std::string("ao_roll_run: ao_net_status: ") + ao_net_last_error(r.net));
    if (nflags & AO_NET_FP16_RANGE)
        return roll_fail(e, "ao_roll_run: AO_NET_FP16_RANGE: an activation left the fp16 range (|x| > 65504) in the split-fp16 trunk; the rolling search does not "
                            "repeat moves on the fp32-MFMA trunk (ao_search does). No game was turned, the roll is closed");
    int32_t* h_done = r.h_i32;
    int32_t* h_target = h_done + G;
    int32_t* h_leaf = h_target + G;
    int32_t* h_err = h_leaf + G;
    int32_t* h_games = h_err + G;
    int32_t* h_rec = h_games + G + static_cast<size_t>(G) * ao::kRollItem;
    AO_HIP(e, hipMemcpyAsync(h_done, e->tp.sims_done, sizeof(int32_t) * G, hipMemcpyDeviceToHost, e->stream));
    AO_HIP(e, hipMemcpyAsync(h_target, e->tp.sims_target, sizeof(int32_t) * G, hipMemcpyDeviceToHost, e->stream));
    AO_HIP(e, hipMemcpyAsync(h_leaf, e->tp.leaf_status, sizeof(int32_t) * G, hipMemcpyDeviceToHost, e->stream));
    AO_HIP(e, hipMemcpyAsync(h_err, e->tp.err, sizeof(int32_t) * G, hipMemcpyDeviceToHost, e->stream));
    roll_count(e, sizeof(int32_t) * 4 * G);
    if (r.loop.harvest(r.loop.launch)) return 1;
    AO_HIP(e, hipStreamSynchronize(e->stream));
    if (r.look_pending) {
        int unfinished = 0, owed = 0;
        settle_harvest(e, &unfinished, &owed);
        r.look_pending = false;
    }
    if (report_game_errors(e, h_err)) { roll_close(e); return 1; }
    int n = 0;
    for (int g = 0; g < G; ++g)
        if (ao::roll_game_turns(r.in_move[g], h_done[g], h_target[g], h_leaf[g] == ao::LS_IDLE)) h_games[n++] = g;
    ++r.turns;
    r.last_games = n;
    out->count = 0;
    RollTactics& t = r.tac;
    if (n == 0) {
        if (t.on && roll_tactics_step(e, std::vector<int32_t>(), nullptr, true)) return roll_fail(e, e->err);   // (verdicts may be in)
        r.last_bytes = r.bytes - bytes0;
        return 0;
    }
    const size_t nA = static_cast<size_t>(n) * A;
    double* d_pi = r.d_out;
    double* d_visit = r.want_visit ? r.d_out + nA : nullptr;
    double* d_policy = r.want_policy ? r.d_out + 2 * nA : nullptr;
    AO_HIP(e, hipMemcpyAsync(r.d_games, h_games, sizeof(int32_t) * n, hipMemcpyHostToDevice, e->stream));
    ao::launch_roll_turn(r.loop.p, r.d_games, n, e->d_active, e->d_settled, r.d_rec, d_pi, d_visit, d_policy, e->stream);
    (void)ao::launch_reroot(r.loop.p, n, r.d_games, e->stream);   // (cannot refuse: ao_roll_begin checked reroot_fits)
    AO_HIP(e, hipGetLastError());
    AO_HIP(e, hipMemcpyAsync(h_rec, r.d_rec, sizeof(int32_t) * ao::kRollRec * n, hipMemcpyDeviceToHost, e->stream));
    AO_HIP(e, hipMemcpyAsync(e->h_out, d_pi, sizeof(double) * nA, hipMemcpyDeviceToHost, e->stream));
    if (d_visit) AO_HIP(e, hipMemcpyAsync(e->h_out + nA, d_visit, sizeof(double) * nA, hipMemcpyDeviceToHost, e->stream));
    if (d_policy) AO_HIP(e, hipMemcpyAsync(e->h_out + 2 * nA, d_policy, sizeof(double) * nA, hipMemcpyDeviceToHost, e->stream));
    roll_count(e, sizeof(int32_t) * (1 + ao::kRollRec) * n + sizeof(double) * nA * (1 + (d_visit ? 1 : 0) + (d_policy ? 1 : 0)));
    if (t.on) {   // what the solver said at the root of the move each turned game just played: 16 B (+ A) per game
        ao::launch_roll_words(r.d_games, n, A, t.d_words, t.d_allowed, t.d_out_words, t.want_allowed ? t.d_out_allowed : nullptr, e->stream);
        AO_HIP(e, hipGetLastError());
        AO_HIP(e, hipMemcpyAsync(t.h_words, t.d_out_words, sizeof(int32_t) * 4 * n, hipMemcpyDeviceToHost, e->stream));
        if (t.want_allowed) AO_HIP(e, hipMemcpyAsync(t.h_allowed, t.d_out_allowed, nA, hipMemcpyDeviceToHost, e->stream));
        const size_t bytes = static_cast<size_t>(n) * 16 + (t.want_allowed ? nA : 0);
        t.stats[5] += static_cast<int64_t>(bytes);
        roll_count(e, bytes);
    }
    const bool gather = e->tp.noise != 0 && !r.draining;   // the streams of the played games, for the draws of their next moves
    if (gather) {
        ao::launch_roll_gather(r.loop.p, r.d_games, n, e->d_mt_backup, e->d_pos_backup, e->stream);
        AO_HIP(e, hipGetLastError());
        AO_HIP(e, hipMemcpyAsync(e->h_mt, e->d_mt_backup, sizeof(uint32_t) * 624 * n, hipMemcpyDeviceToHost, e->stream));
        AO_HIP(e, hipMemcpyAsync(e->h_pos, e->d_pos_backup, sizeof(int32_t) * n, hipMemcpyDeviceToHost, e->stream));
        roll_count(e, static_cast<size_t>(n) * (624 * 4 + 4));
    }
    AO_HIP(e, hipStreamSynchronize(e->stream));
    // The turned games' error words came back in their records (ERR_SHORT, ERR_BAD_MOVE): no second [G]-wide read. Any of them
    // fails the call as ao_end_move / ao_play would, before a host mirror is touched; the roll is closed.
    bool bad = false;
    for (int b = 0; b < n; ++b) {
        const int32_t* rec = h_rec + static_cast<size_t>(b) * ao::kRollRec;
        h_err[rec[0]] = rec[7];   // (h_err was all zero: report_game_errors passed it above)
        bad = bad || rec[7] != 0;
    }
    if (bad && report_game_errors(e, h_err)) { roll_close(e); return 1; }
    std::vector<int32_t> next, next_rows;
    for (int b = 0; b < n; ++b) {
        const int32_t* rec = h_rec + static_cast<size_t>(b) * ao::kRollRec;
        const int g = rec[0];
        out->game[b] = g;
        out->ply[b] = static_cast<int32_t>(e->moves[g].size());
        out->action[b] = rec[1];
        out->win[b] = rec[2];
        out->tau[b] = rec[3];
        out->sims[b] = std::max(0, rec[4] - e->bonus[g]);
        out->settled[b] = rec[5];
        e->moves[g].push_back(rec[1]);
        e->status[g] = rec[6];
        e->over[g] = rec[2];
        e->active[g] = 0;
        r.in_move[g] = ao::ROLL_OUT;
        --r.n_in_move;
        if (ao::roll_begins_next(rec[2], r.draining)) { next.push_back(g); next_rows.push_back(b); }
    }
    std::memcpy(out->pi, e->h_out, sizeof(double) * nA);
    if (out->visit && d_visit) std::memcpy(out->visit, e->h_out + nA, sizeof(double) * nA);
    if (out->policy && d_policy) std::memcpy(out->policy, e->h_out + 2 * nA, sizeof(double) * nA);
    out->count = n;
    r.games_turned += n;
    if (t.on) {
        t.rec_count = n;
        t.rec_words.assign(t.h_words, t.h_words + 4 * static_cast<size_t>(n));
        if (t.want_allowed) t.rec_allowed.assign(t.h_allowed, t.h_allowed + nA);
        for (int b = 0; b < n; ++b) t.stats[4] += t.rec_words[4 * static_cast<size_t>(b) + 2];
        // (with noise the streams of `next` lie in the staging rows; without, nothing of them is needed)
        if (roll_tactics_step(e, next, gather ? next_rows.data() : nullptr, true)) return roll_fail(e, e->err);
        r.last_bytes = r.bytes - bytes0;
        return 0;
    }
    if (roll_begin_games(e, next, gather ? next_rows.data() : nullptr)) return roll_fail(e, e->err);
    r.last_bytes = r.bytes - bytes0;
    return 0;
}

extern "C" {

int ao_roll_begin(ao_engine* e, ao_net* net, const ao_roll_opts* o) {
    RollState& r = e->roll;
    if (roll_refuses(e, "ao_roll_begin")) return 1;
    if (e->in_move) return e->fail("ao_roll_begin inside a move (between ao_begin_move and ao_end_move)");
    if (!net || !o) return e->fail("ao_roll_begin: null argument");
    if (e->bar_pending || e->bar_on_device) return e->fail("ao_roll_begin: a root bar is pending (ao_set_root_bar / ao_root_tactics with apply): the rolling search has no root bar");
    if (e->log_n > 0) return e->fail("ao_roll_begin: an eval log is set (ao_set_eval_log): the rolling search does not feed it");
    if (e->proof_moves) return e->fail("ao_roll_begin: proof moves are on (ao_set_proof_moves): the roll's turn on the device does not apply them");
    if (o->turn_every < 1) return e->fail("ao_roll_begin: turn_every must be >= 1");
    RollTactics& t = r.tac;
    const bool armed = t.max_depth > 0;
    if (armed && (e->tp.win_mark < 3 || e->tp.win_mark > 5 || e->tp.win_mark > e->cfg.board))
        return e->fail("ao_roll_begin: the solver (ao_roll_set_tactics) needs win_mark in 3..5 and at most the board size");
    std::string why;
    if (ao::net_check(net, e->cfg.board, e->cfg.inplanes, e->cfg.device, &why)) return e->fail("ao_roll_begin: " + why);
    // (every turn re-roots: the bound is fixed per engine, so it is checked here, where the call can still be refused)
    if (!ao::reroot_fits(e->tp)) return queue_refused(e, "ao_roll_begin");
    const int G = e->G, A = e->A;
    std::vector<uint8_t> act;
    if (roll_listed(e, o->active, &act, "ao_roll_begin")) return 1;
    AO_HIP(e, hipSetDevice(e->cfg.device));
    if (!r.h_i32) {   // the compact buffers of the engine's first roll (a failed allocation refuses the call; what it got stays in the pool)
        if (e->pool.alloc(e, &r.d_games, G) || e->pool.alloc(e, &r.d_items, static_cast<size_t>(G) * ao::kRollItem) ||
            e->pool.alloc(e, &r.d_rec, static_cast<size_t>(G) * ao::kRollRec) || e->pool.alloc(e, &r.d_out, 3 * static_cast<size_t>(G) * A) ||
            e->pool.alloc(e, &r.d_noise, static_cast<size_t>(G) * e->Ap))
            return 1;
        AO_HIP(e, hipHostMalloc(reinterpret_cast<void**>(&r.h_i32), sizeof(int32_t) * G * (5 + ao::kRollItem + ao::kRollRec), hipHostMallocDefault));
    }
    if (armed && !t.stream) {   // the solver's stream and the per-game verdict rows, by the first roll that runs with it
        if (e->pool.alloc(e, &t.d_words, static_cast<size_t>(G) * 4) || e->pool.alloc(e, &t.d_out_words, static_cast<size_t>(G) * 4)) return 1;
        AO_HIP(e, hipHostMalloc(reinterpret_cast<void**>(&t.h_words), sizeof(int32_t) * 4 * G, hipHostMallocDefault));
        AO_HIP(e, hipStreamCreateWithFlags(&t.stream, hipStreamNonBlocking));
    }
    if (armed && t.want_allowed && !t.d_allowed) {
        if (e->pool.alloc(e, &t.d_allowed, static_cast<size_t>(G) * A) || e->pool.alloc(e, &t.d_out_allowed, static_cast<size_t>(G) * A)) return 1;
        AO_HIP(e, hipHostMalloc(reinterpret_cast<void**>(&t.h_allowed), static_cast<size_t>(G) * A, hipHostMallocDefault));
    }
    if (roll_take_tables(e, o, act, true, "ao_roll_begin")) return 1;
    // nothing can refuse the call any more
    r.in_move.assign(G, 0);
    r.net = net;
    r.early = o->early_stop != 0;
    r.want_visit = o->want_visit != 0;
    r.want_policy = o->want_policy != 0;
    r.cad = ao::RollCadence{};
    r.cad.turn_every = o->turn_every;
    r.cad.early = r.early;
    r.look_pending = false;
    r.n_in_move = 0;
    r.draining = false;
    t.on = armed;
    t.hold = (armed && getenv("AO_ROLL_TACTICS_HOLD")) ? std::max(0, atoi(getenv("AO_ROLL_TACTICS_HOLD"))) : 0;
    t.pending.clear();
    t.n_waiting = 0;
    t.rec_count = 0;
    std::fill(t.stats, t.stats + 6, 0);
    // the plan: rows per simulation for every G, the batch bounded by ao_set_row_cap
    if (r.loop.plan(e, net, (e->row_cap > 0 && e->row_cap < G) ? e->row_cap : G)) return 1;
    r.loop.per_sim = true;
    r.loop.traffic = &r.bytes;   // (the row counters a harvest reads count as the roll's traffic, one word per launch)
    ao::TreeParams& p = r.loop.p;
    p.row_cap = static_cast<unsigned>(r.loop.cap_rows);
    p.row_target = p.row_cap;
    p.ctl = nullptr; p.live_prev = nullptr; p.order = nullptr; p.max_levels = 0;
    // (a root may still hold kBarQ children of an earlier barred move: an all-zero bar turns them back where a move begins)
    // (with the solver every game's row is the bar of its current move: k_roll_verdict writes it before the move begins)
    p.bar = nullptr;
    if (e->bar_dirty || t.on) {
        AO_HIP(e, hipMemsetAsync(e->d_bar, 0, sizeof(uint64_t) * e->h_bar.size(), e->stream));
        p.bar = e->d_bar;
    }
    if (r.loop.zero_ring()) return 1;
    AO_HIP(e, hipMemsetAsync(e->d_active, 0, G, e->stream));
    AO_HIP(e, hipMemsetAsync(e->d_early, 0, G, e->stream));
    AO_HIP(e, hipMemsetAsync(e->d_settled, 0, G, e->stream));
    AO_HIP(e, hipMemsetAsync(p.stats, 0, sizeof(unsigned) * 4 * G, e->stream));
    std::fill(e->active.begin(), e->active.end(), 0);
    r.open = true;
    std::vector<int32_t> games;
    for (int g = 0; g < G; ++g)
        if (act[g]) games.push_back(g);
    if (t.on ? roll_tactics_step(e, games, nullptr, false) : roll_begin_games(e, games, nullptr)) { roll_close(e); return 1; }
    p.live = r.loop.slot(0);
    ao::launch_select(p, e->stream);
    AO_HIP(e, hipGetLastError());
    AO_HIP(e, hipStreamSynchronize(e->stream));
    return 0;
}

int ao_roll_join(ao_engine* e, const ao_roll_opts* o) {
    RollState& r = e->roll;
    if (!r.open) return e->fail("ao_roll_join: no roll is open");
    if (!o) return e->fail("ao_roll_join: null argument");
    AO_HIP(e, hipSetDevice(e->cfg.device));
    std::vector<uint8_t> act;
    if (roll_listed(e, o->active, &act, "ao_roll_join")) return 1;
    if (roll_take_tables(e, o, act, false, "ao_roll_join")) return 1;
    std::vector<int32_t> games;
    for (int g = 0; g < e->G; ++g)
        if (act[g]) games.push_back(g);
    // (a joined game has LS_IDLE: the next launch's expansion half does nothing for it, its selection half starts simulation 0)
    if (e->roll.tac.on ? roll_tactics_step(e, games, nullptr, false) : roll_begin_games(e, games, nullptr)) return roll_fail(e, e->err);
    return 0;
}

int ao_roll_drain(ao_engine* e) {
    if (!e->roll.open) return e->fail("ao_roll_drain: no roll is open");
    e->roll.draining = true;
    return 0;
}

int ao_roll_run(ao_engine* e, int64_t max_launches, ao_roll_records* out) {
    RollState& r = e->roll;
    if (!r.open) return e->fail("ao_roll_run: no roll is open");
    if (!out || !out->game || !out->ply || !out->action || !out->win || !out->tau || !out->sims || !out->settled || !out->pi)
        return e->fail("ao_roll_run: null record array");
    if (max_launches < 0) return e->fail("ao_roll_run: max_launches must be >= 0");
    AO_HIP(e, hipSetDevice(e->cfg.device));
    out->count = 0;
    r.tac.rec_count = 0;
    int64_t launches = 0;
    if (ao::roll_run_returns(0, r.n_in_move, launches, max_launches)) return 0;
    for (;;) {
        switch (r.cad.next()) {
        case ao::ROLL_TURN:
            if (roll_turn(e, out)) return 1;
            if (ao::roll_run_returns(out->count, r.n_in_move, launches, max_launches)) return 0;
            break;
        case ao::ROLL_LOOK:
            if (roll_look(e)) return 1;
            break;
        case ao::ROLL_LAUNCH:
            if (roll_launch(e)) return 1;
            ++launches;
            if (!r.cad.turn_due() && ao::roll_run_returns(0, r.n_in_move, launches, max_launches)) return 0;
            break;
        }
    }
}

int ao_roll_end(ao_engine* e) {
    RollState& r = e->roll;
    if (!r.open) return e->fail("ao_roll_end: no roll is open");
    if (r.n_in_move > 0)
        return e->fail("ao_roll_end: " + std::to_string(r.n_in_move) + " game(s) are still in a move (ao_roll_drain, then ao_roll_run until nothing is)");
    AO_HIP(e, hipSetDevice(e->cfg.device));
    if (r.loop.harvest(r.loop.launch)) return 1;
    AO_HIP(e, hipStreamSynchronize(e->stream));
    roll_close(e);
    return 0;
}

int ao_roll_set_tactics(ao_engine* e, int32_t max_depth, int32_t max_nodes, int32_t solved_sims, int32_t want_allowed) {
    if (roll_refuses(e, "ao_roll_set_tactics")) return 1;
    RollTactics& t = e->roll.tac;
    if (max_depth == 0) {
        t.max_depth = t.max_nodes = t.solved_sims = 0;
        t.want_allowed = false;
        return 0;
    }
    const std::string bad_limits = ao::fw_limits_error("ao_roll_set_tactics", max_depth, max_nodes);
    if (!bad_limits.empty()) return e->fail(bad_limits);
    if (solved_sims < 0 || solved_sims > e->S)
        return e->fail("ao_roll_set_tactics: solved_sims must be in 0.." + std::to_string(e->S) + " (0: no cap)");
    t.max_depth = max_depth; t.max_nodes = max_nodes; t.solved_sims = solved_sims;
    t.want_allowed = want_allowed != 0;
    return 0;
}

int ao_roll_tactics_records(ao_engine* e, int32_t* verdict, int32_t* depth, int32_t* nodes, int32_t* unknown, uint8_t* allowed) {
    const RollTactics& t = e->roll.tac;
    if (allowed && t.rec_count > 0 && t.rec_allowed.size() < static_cast<size_t>(t.rec_count) * e->A)
        return e->fail("ao_roll_tactics_records: allowed rows need ao_roll_set_tactics(..., want_allowed = 1)");
    int32_t* out[4] = {verdict, depth, nodes, unknown};
    for (int b = 0; b < t.rec_count; ++b)
        for (int w = 0; w < 4; ++w)
            if (out[w]) out[w][b] = t.rec_words[4 * static_cast<size_t>(b) + w];
    if (allowed && t.rec_count > 0) std::memcpy(allowed, t.rec_allowed.data(), static_cast<size_t>(t.rec_count) * e->A);
    return 0;
}

int ao_roll_tactics_stats(ao_engine* e, int64_t* out) {
    if (!out) return e->fail("ao_roll_tactics_stats: null argument");
    std::copy(e->roll.tac.stats, e->roll.tac.stats + 6, out);
    return 0;
}

int ao_roll_stats(ao_engine* e, int64_t* turns, int64_t* games_turned, int64_t* bytes, int64_t* last_games, int64_t* last_bytes) {
    if (turns) *turns = e->roll.turns;
    if (games_turned) *games_turned = e->roll.games_turned;
    if (bytes) *bytes = e->roll.bytes;
    if (last_games) *last_games = e->roll.last_games;
    if (last_bytes) *last_bytes = e->roll.last_bytes;
    return 0;
}

}  // extern "C"
