// root_tactics.hip -- the forced-win solver on an engine's own roots: the kernels, then ao_root_tactics. No reference
// counterpart; the definition is utils.root_tactics, which goes through utils.forced_win alone. The positions are the engine's
// TreeParams::rootpos, read on the device: no move list is staged. Three launches: the mover's search and the opponent's
// search after a pass (k_root_tactics_a), every reply's search for the games that stand under a proven threat with no win
// of their own (k_root_tactics_b), and one wavefront per game that puts the words together (k_root_tactics_rows). The
// search, its word and the search after a reply are those of the position batch (tactics_device.hpp).
#include <cstring>
#include <string>
#include <vector>

#include "engine.hpp"
#include "launchers.hpp"
#include "tactics_device.hpp"

namespace ao {

struct RootTacticsParams {
    const Pos* rootpos;     // [G]
    const uint8_t* active;  // [G] or null
    int G, B, A, win_mark, max_depth, max_nodes;
    RootTacticsBufs b;
};

// Two wavefronts per game: role 0 searches for the mover, role 1 for the opponent as if the mover had passed -- and role 0
// is that search with the sides exchanged: the opponent passes. Stones = popcount of the bitboards, the mover from the ply's
// parity (what replay_moves gives for the game's id). An inactive or a terminal game is not searched: both words 0.
template <int NCH>
__global__ __launch_bounds__(64 * kPosPerWG) void k_root_tactics_a(RootTacticsParams q) {
    __shared__ FwWave s_wave[kPosPerWG];
    const int wv = wg_wave();
    const int k = blockIdx.x * kPosPerWG + wv;
    const int g = k >> 1, role = k & 1;
    if (g >= q.G) return;
    const bool on = !q.active || __builtin_amdgcn_readfirstlane(static_cast<int>(q.active[g])) != 0;
    PosR s = pos_load(q.rootpos + g);
    const int stones = __builtin_amdgcn_readfirstlane(pos_stones(s));
    const int m = __builtin_amdgcn_readfirstlane(s.ply) & 1;

    FwResult r;
    int status;
    const uint32_t word = reply_search<NCH>(s, m ^ role ^ 1, stones, kPass, on, s_wave[wv], q.B, q.A, q.win_mark, q.max_depth, q.max_nodes,
                                            status, r);
    if (lane_id() == 0) {
        q.b.stage[2 * static_cast<size_t>(g) + role] = word;
        if (role == 0) {
#pragma unroll
            for (int w = 0; w < kBBWords; ++w) q.b.won[static_cast<size_t>(g) * kBBWords + w] = r.won[w];
        }
    }
}

// stage A left "the opponent's forced win is proven, the mover has none" for game g
__device__ __forceinline__ bool root_under_threat(const RootTacticsParams& q, int g) {
    const uint32_t own = q.b.stage[2 * static_cast<size_t>(g)], thr = q.b.stage[2 * static_cast<size_t>(g) + 1];
    return own != 0u && fw_word_result(own) != FW_WIN && fw_word_result(thr) == FW_WIN;
}

// One wavefront per (game, reply cell) pair, grid G x ceil(A / kPosPerWG). A wave returns at once unless its game is under a
// proven threat; otherwise it does what k_forced_defences does for a reply pair: the mover's stone on the cell, the
// opponent's search on what stands then. An occupied cell writes 0.
template <int NCH>
__global__ __launch_bounds__(64 * kPosPerWG) void k_root_tactics_b(RootTacticsParams q) {
    __shared__ FwWave s_wave[kPosPerWG];
    const int wv = wg_wave();
    const int g = blockIdx.x, j = blockIdx.y * kPosPerWG + wv;
    if (j >= q.A) return;
    if (!__builtin_amdgcn_readfirstlane(static_cast<int>(root_under_threat(q, g)))) return;
    PosR s = pos_load(q.rootpos + g);
    const int stones = __builtin_amdgcn_readfirstlane(pos_stones(s));
    const int m = __builtin_amdgcn_readfirstlane(s.ply) & 1;

    FwResult r;
    int status;
    const uint32_t word = reply_search<NCH>(s, m, stones, j, true, s_wave[wv], q.B, q.A, q.win_mark, q.max_depth, q.max_nodes, status, r);
    if (lane_id() == 0) q.b.pair[static_cast<size_t>(g) * q.A + j] = word;
}

// One wavefront per game: verdict, depth, nodes, unknown, allowed [A] and the bar of the move out of the words of its
// searches, by utils.root_tactics' rules. `nodes` and `unknown` count the searches the host definition runs: the mover's;
// the opponent's unless the mover wins; the replies' under a proven threat. Ballots and integer sums only: no result
// depends on an order. The bar (in: the caller's barred actions, or zeros) becomes the caller's plus the empty cells the
// verdict does not allow -- unless that left the game nothing to search: then it stays the caller's.
template <int NCH>
__global__ __launch_bounds__(64 * kPosPerWG) void k_root_tactics_rows(RootTacticsParams q) {
    const int g = wave_item();
    if (g >= q.G) return;
    const int lane = lane_id();
    const uint32_t own = q.b.stage[2 * static_cast<size_t>(g)], thr = q.b.stage[2 * static_cast<size_t>(g) + 1];
    const PosR s = pos_load(q.rootpos + g);
    const bool searched = own != 0u;
    const int own_res = fw_word_result(own), thr_res = fw_word_result(thr);
    const bool win = searched && own_res == FW_WIN;
    const bool threat = searched && !win && thr_res == FW_WIN;
    int verdict = win ? RT_WIN : RT_NONE;
    int depth = win ? fw_word_depth(own) : 0;
    int unknown = (searched && own_res == FW_UNKNOWN) ? 1 : 0;
    if (searched && !win && thr_res == FW_UNKNOWN) unknown |= 2;
    int nodes_l = 0;
    if (lane == 0 && searched) nodes_l = fw_word_nodes(own) + (win ? 0 : fw_word_nodes(thr));
    uint64_t em[NCH], ok[NCH];             // the empty cells; the cells the verdict allows
    int n_ok = 0;
    bool ran_out = false;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int cell = lane + 64 * c;
        const bool empty = cell < q.A && !(((s.bb[0][c] | s.bb[1][c]) >> lane) & 1ull);
        em[c] = __ballot(empty);
        const uint32_t w = (threat && cell < q.A) ? q.b.pair[static_cast<size_t>(g) * q.A + cell] : 0u;
        const int rep = fw_word_reply(w);
        nodes_l += fw_word_nodes(w);
        ran_out = ran_out || __ballot(rep == FD_UNKNOWN) != 0ull;
        const bool mine = (q.b.won[static_cast<size_t>(g) * kBBWords + c] >> lane) & 1ull;
        ok[c] = __ballot(threat ? (rep == FD_SAFE || rep == FD_UNKNOWN) : win ? mine : empty);
        n_ok += __popcll(ok[c]);
    }
    if (threat) {
        verdict = n_ok > 0 ? RT_DEFEND : RT_LOST;
        depth = fw_word_depth(thr);
        if (ran_out) unknown |= 4;
    }
    const bool open = !searched || verdict == RT_LOST;   // nothing proven that could restrict: every empty cell (zeros where nothing was searched)
    const int nodes = wave_sum_i(nodes_l);                // <= 227 * 65536
    if (lane == 0) {
        if (q.b.verdict) q.b.verdict[g] = verdict;
        if (q.b.depth) q.b.depth[g] = depth;
        if (q.b.nodes) q.b.nodes[g] = nodes;
        if (q.b.unknown) q.b.unknown[g] = unknown;
    }
    int n_left = 0;
    uint64_t allow[NCH], cb[NCH], nb[NCH];   // what the verdict allows; the caller's bar; the bar with the verdict's on top
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        allow[c] = open ? (searched ? em[c] : 0ull) : ok[c];
        cb[c] = q.b.bar ? uniform64(q.b.bar[static_cast<size_t>(g) * kBBWords + c]) & em[c] : 0ull;
        nb[c] = searched ? (cb[c] | (em[c] & ~allow[c])) : cb[c];
        n_left += __popcll(em[c] & ~nb[c]);
    }
    store_cell_mask<NCH>(q.b.allowed ? q.b.allowed + static_cast<size_t>(g) * q.A : nullptr, q.A, allow, true);
    if (q.b.bar && lane == 0) {
        uint64_t* out = q.b.bar + static_cast<size_t>(g) * kBBWords;
#pragma unroll
        for (int c = 0; c < NCH; ++c) out[c] = n_left > 0 ? nb[c] : cb[c];
#pragma unroll
        for (int c = NCH; c < kBBWords; ++c) out[c] = 0ull;
    }
}

// The kernels index everything by the position's number in q.rootpos, 0 .. q.G - 1. ao_root_tactics hands them the engine's [G]
// roots; the rolling search hands them n compact rows copied out of the roots (k_roll_rootpos) and a batch's own buffers: the
// LIST form is the same code with G = n, grids ceil(2n / kPosPerWG), n x ceil(A / kPosPerWG) and ceil(n / kPosPerWG).
static void launch_root_tactics_q(const RootTacticsParams& q, hipStream_t s) {
    const dim3 block(64 * kPosPerWG);
    const dim3 grid_a(static_cast<unsigned>((2 * q.G + kPosPerWG - 1) / kPosPerWG));
    const dim3 grid_b(static_cast<unsigned>(q.G), static_cast<unsigned>((q.A + kPosPerWG - 1) / kPosPerWG));
    const dim3 grid_r(static_cast<unsigned>((q.G + kPosPerWG - 1) / kPosPerWG));
    AO_DISPATCH_NCH(nch_of_cells(q.A), hipLaunchKernelGGL(k_root_tactics_a<NCH>, grid_a, block, 0, s, q);
                    hipLaunchKernelGGL(k_root_tactics_b<NCH>, grid_b, block, 0, s, q);
                    hipLaunchKernelGGL(k_root_tactics_rows<NCH>, grid_r, block, 0, s, q));
}

static void launch_root_tactics(const TreeParams& p, const uint8_t* active, int max_depth, int max_nodes, const RootTacticsBufs& b, hipStream_t s) {
    RootTacticsParams q{};
    q.rootpos = p.rootpos; q.active = active;
    q.G = p.G; q.B = p.B; q.A = p.A; q.win_mark = p.win_mark; q.max_depth = max_depth; q.max_nodes = max_nodes;
    q.b = b;
    launch_root_tactics_q(q, s);
}

void launch_root_tactics_rows(const Pos* rows, int n, int B, int A, int win_mark, int max_depth, int max_nodes, const RootTacticsBufs& b,
                              hipStream_t s) {
    RootTacticsParams q{};
    q.rootpos = rows; q.active = nullptr;
    q.G = n; q.B = B; q.A = A; q.win_mark = win_mark; q.max_depth = max_depth; q.max_nodes = max_nodes;
    q.b = b;
    launch_root_tactics_q(q, s);
}

}  // namespace ao

extern "C" {

// utils.root_tactics of every active game's root position, read where it lives (TreeParams::rootpos): no move list goes to
// the device. apply: the bar of the next move is left on the device -- the caller's pending masks (ao_set_root_bar)
// intersected with what the solver allows, game by game; a game whose intersection would be empty keeps the caller's.
int ao_root_tactics(ao_engine* e, const uint8_t* active, int32_t max_depth, int32_t max_nodes, int32_t apply, int32_t* verdict,
                    int32_t* depth, uint8_t* allowed, int32_t* nodes, int32_t* unknown) {
    if (roll_refuses(e, "ao_root_tactics")) return 1;
    if (e->in_move) return e->fail("ao_root_tactics inside a move (between ao_begin_move and ao_end_move)");
    const std::string bad_limits = ao::fw_limits_error("ao_root_tactics", max_depth, max_nodes);
    if (!bad_limits.empty()) return e->fail(bad_limits);
    if (e->tp.win_mark < 3 || e->tp.win_mark > 5 || e->tp.win_mark > e->cfg.board)
        return e->fail("ao_root_tactics: the solver needs win_mark in 3..5 and at most the board size");
    const size_t G = static_cast<size_t>(e->G), A = static_cast<size_t>(e->A);
    std::vector<uint8_t> act(G);
    for (size_t g = 0; g < G; ++g) act[g] = (active ? active[g] : 1) && !e->over[g];
    bool bar_any = false;
    if (apply && bar_build(e, act, &bar_any, "ao_root_tactics")) return 1;   // (before any device call)
    const size_t at_stage = G * ao::kBBWords * 8, at_pair = at_stage + G * 8, at_out = at_pair + G * A * 4;
    const size_t out_bytes = G * 16 + G * A, at_mask = at_out + out_bytes;
    if (readout_begin(e, "ao_root_tactics", at_mask + G)) return 1;
    ao::RootTacticsBufs b{};
    b.won = reinterpret_cast<uint64_t*>(e->d_ro.p);
    b.stage = reinterpret_cast<uint32_t*>(e->d_ro.p + at_stage);
    b.pair = reinterpret_cast<uint32_t*>(e->d_ro.p + at_pair);
    b.verdict = reinterpret_cast<int32_t*>(e->d_ro.p + at_out);
    b.depth = b.verdict + G; b.nodes = b.depth + G; b.unknown = b.nodes + G;
    b.allowed = e->d_ro.p + at_out + G * 16;
    uint8_t* d_act = e->d_ro.p + at_mask;
    AO_HIP(e, hipMemcpyAsync(d_act, act.data(), G, hipMemcpyHostToDevice, e->stream));
    if (apply) {
        AO_HIP(e, hipMemcpyAsync(e->d_bar, e->h_bar.data(), sizeof(uint64_t) * e->h_bar.size(), hipMemcpyHostToDevice, e->stream));
        b.bar = e->d_bar;
    }
    ao::launch_root_tactics(e->tp, d_act, max_depth, max_nodes, b, e->stream);
    AO_HIP(e, hipGetLastError());
    AO_HIP(e, hipMemcpyAsync(e->h_ro.data(), e->d_ro.p + at_out, out_bytes, hipMemcpyDeviceToHost, e->stream));
    AO_HIP(e, hipStreamSynchronize(e->stream));
    if (apply) e->bar_on_device = true;
    const int32_t* h = reinterpret_cast<const int32_t*>(e->h_ro.data());
    if (verdict) std::memcpy(verdict, h, 4 * G);
    if (depth) std::memcpy(depth, h + G, 4 * G);
    if (nodes) std::memcpy(nodes, h + 2 * G, 4 * G);
    if (unknown) std::memcpy(unknown, h + 3 * G, 4 * G);
    if (allowed) std::memcpy(allowed, e->h_ro.data() + G * 16, G * A);
    return 0;
}

}  // extern "C"
