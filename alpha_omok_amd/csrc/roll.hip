// roll.hip -- the device side of the rolling search (ao_roll_*, engine.hip): a TURN for a compact list of games while the
// others are mid-search in the same launch loop. Every kernel is one wavefront per LISTED game and touches that game's state
// only; what the host reads and writes per turn is O(listed games).
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
#include "host_handle.hpp"
#include "launchers.hpp"
#include "move_device.hpp"
#include "roll_schedule.hpp"

namespace ao {

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

void launch_roll_rootpos(const TreeParams& p, const int32_t* games, int n, Pos* rows, hipStream_t s) {
    hipLaunchKernelGGL(k_roll_rootpos, dim3(n), dim3(64), 0, s, p, games, rows);
}
void launch_roll_verdict(int32_t* items, const RollBatchView& b, int A, int solved_sims, uint64_t* bar, int32_t* game_words, uint8_t* game_allowed,
                         hipStream_t s) {
    hipLaunchKernelGGL(k_roll_verdict, dim3(b.n), dim3(64), 0, s, items, b, A, solved_sims, bar, game_words, game_allowed);
}
void launch_roll_words(const int32_t* games, int n, int A, const int32_t* game_words, const uint8_t* game_allowed, int32_t* out_words,
                       uint8_t* out_allowed, hipStream_t s) {
    hipLaunchKernelGGL(k_roll_words, dim3(n), dim3(64), 0, s, games, A, game_words, game_allowed, out_words, out_allowed);
}
void launch_roll_turn(const TreeParams& p, const int32_t* games, int n, uint8_t* active, const uint8_t* settled, int32_t* rec, double* rec_pi,
                      double* rec_visit, double* rec_policy, hipStream_t s) {
    AO_DISPATCH_NCH(nch_of_cells(p.A), hipLaunchKernelGGL(k_roll_turn<NCH>, dim3(n), dim3(64), 0, s, p, games, active, settled, rec, rec_pi,
                                                          rec_visit, rec_policy));
}
void launch_roll_gather(const TreeParams& p, const int32_t* games, int n, uint32_t* out_mt, int32_t* out_pos, hipStream_t s) {
    hipLaunchKernelGGL(k_roll_gather, dim3(n), dim3(64), 0, s, p, games, out_mt, out_pos);
}
void launch_roll_begin(const TreeParams& p, const int32_t* items, int n, const uint32_t* in_mt, const int32_t* in_pos, const double* in_noise,
                       int8_t* tau, uint8_t* active, uint8_t* settled, uint8_t* early, hipStream_t s) {
    AO_DISPATCH_NCH(nch_of_cells(p.A), hipLaunchKernelGGL(k_roll_begin<NCH>, dim3(n), dim3(64), 0, s, p, items, in_mt, in_pos, in_noise, tau,
                                                          active, settled, early));
}
void launch_roll_mask(const TreeParams& p, const uint8_t* early, uint8_t* out, hipStream_t s) {
    hipLaunchKernelGGL(k_roll_mask, dim3((p.G + 255) / 256), dim3(256), 0, s, p, early, out);
}

}  // namespace ao
