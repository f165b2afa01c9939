// positions.hip -- the stateless, batched "position" layer beside the search: rule status, legal moves, input planes and the
// network's evaluation of positions the CALLER names, no tree and no game involved.
//
// One wavefront (64 lanes) owns one position, kPosPerWG positions per workgroup, nothing shared between them (no LDS but
// the search stack of k_forced_wins / k_forced_defences, one per wave).
//
// Reference map (paths relative to /root/reference/2_AlphaOmok/):
//   k_check_win_boards      utils.py:30-59 (check_win) on raw boards: the FULL window scan, row-major, black before white
//                           inside a window -- boards need not be reachable in play, so the scan order decides
//                           (check_win_board, tactics_device.hpp)
//   k_positions_from_moves  utils.py:171-179 (get_board) + utils.py:182-186 (get_turn) + utils.py:22-27 (legal_actions, as a
//                           mask: the CPython set ORDER is the tree kernels' business, legal_order) + utils.py:30-59
//                           (check_win of the final board, and of every prefix through the incremental win_after_move of
//                           the tree kernels) + utils.py:139-168 (get_state_pt, encode_planes of the tree kernels)
//   ao_positions_evaluate   agents.py:171-178 for n positions at once: planes on the device, then the ordinary forward
//   k_win_cells, k_audit_games  no counterpart: the cells that win at once and the per-ply tactical flags of game records,
//                           defined through utils.py:30-59 (check_win of the board with one more stone; winning_cells,
//                           tactics_device.hpp)
//   k_forced_wins           no counterpart: forced wins by continuous fours, a depth-first search per position over the same
//                           winning cells (fw_search, tactics_device.hpp; utils.forced_win of this package is the host
//                           definition)
//   k_forced_defences, k_defence_rows  no counterpart: which replies hold against the opponent's forced win -- the same
//                           search for every (position, reply) pair and for the pass, one wavefront each, then one
//                           wavefront per position that gathers its pairs (utils.forced_defences is the host definition)
// The solver on an engine's own roots (k_root_tactics_*) is root_tactics.hip.
//
// The bitboards, pos_place, pos_occupied, win_after_move and encode_planes are the tree kernels' own (tree_device.hpp): a
// position described here is the position the search would hold.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/omok_hip.h"
#include "host_handle.hpp"
#include "launchers.hpp"
#include "tactics_device.hpp"

namespace ao {

// per-position error codes (ao_positions_from_moves)
enum : int32_t { PE_OK = 0, PE_RANGE = 1, PE_OCCUPIED = 2, PE_LENGTH = 3 };

// boards int8 [n][A] (+1 black, -1 white, anything else empty) -> win int32 [n]
__global__ __launch_bounds__(64 * kPosPerWG) void k_check_win_boards(const int8_t* __restrict__ boards, int n, int B, int win_mark,
                                                                     int32_t* __restrict__ win) {
    const int i = wave_item();
    if (i >= n) return;
    const int lane = lane_id();
    const int A = B * B;
    uint64_t bb[2][kBBWords];
#pragma unroll
    for (int c = 0; c < kBBWords; ++c) {
        const int cell = lane + 64 * c;
        const int v = cell < A ? boards[static_cast<size_t>(i) * A + cell] : 0;
        bb[0][c] = __ballot(v == 1);
        bb[1][c] = __ballot(v == -1);
    }
    const int w = check_win_board(bb[0], bb[1], B, win_mark);
    if (lane == 0) win[i] = w;
}

// The position of the id (0, mv[0], ..., mv[nm - 1]) into `s`, wave-uniform (all 64 lanes call): the moves are placed in
// order, black first, moves past a win too. Returns the id's error code; `s` is then the empty board. end_ply: index of
// the first move after which check_win is non-zero, -1 if there is none. before_move(ply, move) is called with the position
// before a legal move in `s`, while no earlier prefix was terminal.
template <class F>
__device__ __forceinline__ int replay_moves(PosR& s, const int32_t* __restrict__ mv, int nm, int A, int B, int win_mark, int& end_ply,
                                            F&& before_move) {
    const int lane = lane_id();
    pos_clear(s);
    int err = (nm < 0 || nm > A) ? PE_LENGTH : PE_OK;
    end_ply = -1;
    // the moves 64 at a time, one per lane; each then comes out of a v_readlane (everything below is wave-uniform)
    for (int base = 0; err == PE_OK && base < nm; base += 64) {
        const int t_l = base + lane;
        const int m_l = t_l < nm ? mv[t_l] : 0;
        const int cnt = nm - base < 64 ? nm - base : 64;
        for (int j = 0; j < cnt; ++j) {
            const int m = read_lane(m_l, j);
            if (m < 0 || m >= A) { err = PE_RANGE; break; }
            if (pos_occupied(s, m)) { err = PE_OCCUPIED; break; }
            if (end_ply < 0) before_move(base + j, m);
            pos_place(s, m);
            // (every earlier position was not terminal, which is what the incremental test asks for)
            if (end_ply < 0 && win_after_move(s, m, B, win_mark) != 0) end_ply = base + j;
        }
    }
    if (err != PE_OK) pos_clear(s);
    return err;
}

// the ids of a launch, as every kernel below is given them
struct IdBatch {
    const int32_t* moves;   // [n][stride]: row i = root_id[1:] of position i
    const int32_t* nmoves;  // [n]
    int n, stride, B, A, win_mark;
};

// what a wave knows of its id once the moves are replayed: status = check_win of the position, turn = utils.get_turn, both 0
// where the id has an error (ok false; `s` is then the empty board)
struct IdPos {
    PosR s;
    int nm, err, end_ply, status, turn;
    bool ok;
};
// with_status false: status stays 0 (k_forced_defences takes it with the reply on the board)
template <class F>
__device__ __forceinline__ void id_position(IdPos& p, const IdBatch& q, int i, bool with_status, F&& before_move) {
    p.nm = __builtin_amdgcn_readfirstlane(q.nmoves[i]);
    p.err = replay_moves(p.s, q.moves + static_cast<size_t>(i) * q.stride, p.nm, q.A, q.B, q.win_mark, p.end_ply, before_move);
    p.ok = p.err == PE_OK;
    p.status = (with_status && p.ok) ? check_win_board(p.s.bb[0], p.s.bb[1], q.B, q.win_mark) : 0;
    p.turn = p.ok ? (p.nm & 1) : 0;
}
__device__ __forceinline__ void id_position(IdPos& p, const IdBatch& q, int i, bool with_status = true) {
    id_position(p, q, i, with_status, [](int, int) {});
}

struct PositionsParams {
    IdBatch ids;
    int C;
    int bad_as_empty;       // planes of a position with an error: 0 = zeros, 1 = the planes of the empty board (ao_positions_evaluate)
    // outputs, any may be null
    int32_t* status; int32_t* end_ply; int32_t* turn; int32_t* err;
    int8_t* board;          // [n][A]
    uint8_t* legal;         // [n][A]
    float* planes;          // [n][nsym][C][A]
    int nsym;               // 1, or 8: row 8 i + s of `planes` holds sym_planes(planes of position i, s) (symmetry.hpp)
};

template <int NCH>
__global__ __launch_bounds__(64 * kPosPerWG) void k_positions_from_moves(PositionsParams q) {
    const int i = wave_item();
    if (i >= q.ids.n) return;
    const int lane = lane_id();
    const int A = q.ids.A;
    IdPos p;
    id_position(p, q.ids, i);
    const PosR& s = p.s;
    if (lane == 0) {
        if (q.status) q.status[i] = p.status;
        if (q.end_ply) q.end_ply[i] = p.ok ? p.end_ply : 0;
        if (q.turn) q.turn[i] = p.turn;
        if (q.err) q.err[i] = p.err;
    }
    if (q.board) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int cell = lane + 64 * c;
            const int b0 = static_cast<int>((s.bb[0][c] >> lane) & 1ull), b1 = static_cast<int>((s.bb[1][c] >> lane) & 1ull);
            if (cell < A) q.board[static_cast<size_t>(i) * A + cell] = static_cast<int8_t>(b0 - b1);
        }
    }
    const uint64_t empty[kBBWords] = {~(s.bb[0][0] | s.bb[1][0]), ~(s.bb[0][1] | s.bb[1][1]), ~(s.bb[0][2] | s.bb[1][2]),
                                      ~(s.bb[0][3] | s.bb[1][3])};
    store_cell_mask<NCH>(q.legal ? q.legal + static_cast<size_t>(i) * A : nullptr, A, empty, p.ok);
    if (q.planes) {
        if (p.ok || q.bad_as_empty) {
            TreeParams tp{};   // the encoder's view of the batch: row i of a plain NCHW plane batch (no keys: the identity ...)
            tp.C = q.C;
            tp.A = A;
            tp.B = q.ids.B;
            tp.batch_nchw = q.planes;
            if (q.nsym == 1) encode_planes<NCH>(tp, i, s, i);
            else   // ... or all eight symmetries of the position, in rows of their own
                for (int sym = 0; sym < q.nsym; ++sym) encode_planes<NCH>(tp, q.nsym * i + sym, s, 0, nullptr, sym);
        } else {
            float* out = q.planes + static_cast<size_t>(i) * q.nsym * q.C * A;
            for (int idx = lane; idx < q.nsym * q.C * A; idx += 64) out[idx] = 0.f;
        }
    }
}

// The 8-fold mean of ao_positions_evaluate_sym: rows 8 i + s of policy_in / value_in are the network's answers on the eight
// symmetries of position i; each policy row is brought back into the board's own frame (cell c of symmetry s is read where c
// went, sym_cell_inv) and the eight are added in fp32 in the order ((p_0 + p_1) + p_2) + ... + p_7, then scaled by 1/8.
template <int NCH>
__global__ __launch_bounds__(64 * kPosPerWG) void k_sym_mean(const float* __restrict__ policy_in, const float* __restrict__ value_in, int n,
                                                             int B, float* __restrict__ policy, float* __restrict__ value) {
    const int i = wave_item();
    if (i >= n) return;
    const int lane = lane_id();
    const int A = B * B;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int cell = lane + 64 * c;
        if (cell >= A) continue;
        float acc = policy_in[static_cast<size_t>(8 * i) * A + cell];
        for (int sym = 1; sym < 8; ++sym)
            acc = __fadd_rn(acc, policy_in[static_cast<size_t>(8 * i + sym) * A + sym_cell_inv(sym, cell, B)]);
        policy[static_cast<size_t>(i) * A + cell] = __fmul_rn(0.125f, acc);
    }
    if (lane == 0) {
        float acc = value_in[8 * i];
        for (int sym = 1; sym < 8; ++sym) acc = __fadd_rn(acc, value_in[8 * i + sym]);
        value[i] = __fmul_rn(0.125f, acc);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// tactical cells: which empty cells win at once (winning_cells, tactics_device.hpp), asked of positions and of every ply of
// game records -- see ao_positions_win_cells and ao_positions_audit in omok_hip.h.
// ---------------------------------------------------------------------------------------------------------------------
// flag bits of one audited ply (ao_positions_audit)
enum : int { TF_WIN_AVAILABLE = 1, TF_WIN_TAKEN = 2, TF_THREAT = 4, TF_BLOCKED = 8, TF_LOST = 16 };

struct TacticsParams {
    IdBatch ids;
    // outputs, any may be null
    uint8_t* mine; uint8_t* theirs;                 // [n][A]   (k_win_cells)
    int32_t* status; int32_t* turn; int32_t* err;   // [n]      (err: both kernels)
    uint8_t* flags;                                 // [n][A]   (k_audit_games)
    int32_t* counts;                                // [n][8]
};

// the winning cells of the side to move and of its opponent in the position of id i
template <int NCH>
__global__ __launch_bounds__(64 * kPosPerWG) void k_win_cells(TacticsParams q) {
    const int i = wave_item();
    if (i >= q.ids.n) return;
    const int A = q.ids.A;
    IdPos p;
    id_position(p, q.ids, i);
    const bool open = p.ok && p.status == 0;      // a terminal position has no winning cells, for anyone
    uint64_t mine[kBBWords], theirs[kBBWords];
    winning_cells<NCH>(p.s, p.turn, q.ids.B, A, q.ids.win_mark, mine);
    winning_cells<NCH>(p.s, p.turn ^ 1, q.ids.B, A, q.ids.win_mark, theirs);
    if (lane_id() == 0) {
        if (q.status) q.status[i] = p.status;
        if (q.turn) q.turn[i] = p.turn;
        if (q.err) q.err[i] = p.err;
    }
    store_cell_mask<NCH>(q.mine ? q.mine + static_cast<size_t>(i) * A : nullptr, A, mine, open);
    store_cell_mask<NCH>(q.theirs ? q.theirs + static_cast<size_t>(i) * A : nullptr, A, theirs, open);
}

// the tactical audit of game record i: one flag byte per ply and eight counters
template <int NCH>
__global__ __launch_bounds__(64 * kPosPerWG) void k_audit_games(TacticsParams q) {
    const int i = wave_item();
    if (i >= q.ids.n) return;
    const int lane = lane_id();
    const int A = q.ids.A;
    int fl[kBBWords] = {0, 0, 0, 0};   // lane l of fl[c]: the flag byte of ply l + 64 c
    int n_win = 0, n_missed = 0, n_single = 0, n_unblocked = 0, n_lost = 0;
    IdPos p;
    id_position(p, q.ids, i, true, [&](int t, int m) {   // the position before move m of ply t is not terminal: audit the move
        uint64_t mine[kBBWords], theirs[kBBWords];
        winning_cells<NCH>(p.s, t & 1, q.ids.B, A, q.ids.win_mark, mine);
        winning_cells<NCH>(p.s, (t & 1) ^ 1, q.ids.B, A, q.ids.win_mark, theirs);
        const int n_mine = popcount4(mine), n_theirs = popcount4(theirs);
        const bool in_mine = has_cell(mine, m), in_theirs = has_cell(theirs, m);
        int f = 0;
        if (n_mine > 0) {
            f = TF_WIN_AVAILABLE | (in_mine ? TF_WIN_TAKEN : 0);
            n_win += 1;
            n_missed += in_mine ? 0 : 1;
        } else if (n_theirs > 0) {
            f = TF_THREAT | (in_theirs ? TF_BLOCKED : 0) | (n_theirs >= 2 ? TF_LOST : 0);
            n_single += n_theirs >= 2 ? 0 : 1;
            n_unblocked += (n_theirs >= 2 || in_theirs) ? 0 : 1;
            n_lost += n_theirs >= 2 ? 1 : 0;
        }
#pragma unroll
        for (int c = 0; c < kBBWords; ++c) fl[c] = (c == (t >> 6) && lane == (t & 63)) ? f : fl[c];
    });
    const bool ok = p.ok;
    if (lane == 0) {
        if (q.err) q.err[i] = p.err;
        if (q.counts) {
            int32_t* cn = q.counts + static_cast<size_t>(i) * 8;
            cn[0] = ok ? (p.end_ply >= 0 ? p.end_ply + 1 : p.nm) : 0;
            cn[1] = ok ? n_win : 0;
            cn[2] = ok ? n_missed : 0;
            cn[3] = ok ? n_single : 0;
            cn[4] = ok ? n_unblocked : 0;
            cn[5] = ok ? n_lost : 0;
            cn[6] = ok ? p.end_ply : 0;
            cn[7] = p.status;
        }
    }
    if (q.flags) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int t = lane + 64 * c;
            if (t < A) q.flags[static_cast<size_t>(i) * A + t] = static_cast<uint8_t>(ok ? fl[c] : 0);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// forced wins by continuous fours (VCF): fw_search of tactics_device.hpp on the position of an id -- see
// ao_positions_forced_wins in omok_hip.h for the text.
// ---------------------------------------------------------------------------------------------------------------------
struct ForcedParams {
    IdBatch ids;
    int max_depth, max_nodes, line_stride;
    // outputs, any may be null
    int32_t* result; int32_t* depth; int32_t* move; int32_t* line_len; int32_t* nodes;   // [n]
    int32_t* status; int32_t* turn; int32_t* err;                                        // [n]
    uint8_t* mask;          // [n][A]
    int16_t* line;          // [n][line_stride], line_stride = 2 max_depth - 1
};

// utils.forced_win of the position of id i, for its side to move
template <int NCH>
__global__ __launch_bounds__(64 * kPosPerWG) void k_forced_wins(ForcedParams q) {
    __shared__ FwWave s_wave[kPosPerWG];
    const int wv = wg_wave();
    const int i = blockIdx.x * kPosPerWG + wv;
    if (i >= q.ids.n) return;
    FwWave& W = s_wave[wv];
    const int lane = lane_id();
    IdPos p;
    id_position(p, q.ids, i);             // p.turn: the attacker

    FwResult r;
    fw_search<NCH>(p.s, p.turn, p.nm, p.status, W, q.ids.B, q.ids.A, q.ids.win_mark, p.ok, q.max_depth, q.max_nodes, r);
    wsync();
    const bool win = r.result == FW_WIN;
    const int len = win ? __builtin_amdgcn_readfirstlane(static_cast<int>(W.line[0][kFwLine - 1])) : 0;
    if (lane == 0) {
        if (q.result) q.result[i] = r.result;
        if (q.depth) q.depth[i] = r.depth;
        if (q.move) q.move[i] = win ? lowest_cell(r.won) : -1;
        if (q.line_len) q.line_len[i] = len;
        if (q.nodes) q.nodes[i] = r.nodes;
        if (q.status) q.status[i] = p.status;
        if (q.turn) q.turn[i] = p.turn;
        if (q.err) q.err[i] = p.err;
    }
    store_cell_mask<NCH>(q.mask ? q.mask + static_cast<size_t>(i) * q.ids.A : nullptr, q.ids.A, r.won, win);
    if (q.line && lane < q.line_stride)    // line_stride = 2 max_depth - 1 <= 31 < 64; len <= 2 depth - 1 <= line_stride
        q.line[static_cast<size_t>(i) * q.line_stride + lane] = lane < len ? W.line[0][lane] : static_cast<int16_t>(-1);
}

// ---------------------------------------------------------------------------------------------------------------------
// which replies hold against a forced win (VCF defence). The definition is utils.forced_defences: A + 1 searches of
// utils.forced_win per position -- see ao_positions_forced_defences in omok_hip.h for the text.
// ---------------------------------------------------------------------------------------------------------------------
// (the ids' fields stand here themselves: an embedded IdBatch ends on four bytes of padding, which moves max_depth and
// max_nodes in the kernel's arguments and with them the SGPR spill slots of all of k_forced_defences)
struct DefenceParams {
    const int32_t* moves;   // [n][stride]
    const int32_t* nmoves;  // [n]
    int n, stride, B, A, win_mark, max_depth, max_nodes;
    uint32_t* pair;         // k_forced_defences -> k_defence_rows: the word of each pair's search (fw_word), [n][A + 1]
    // outputs, any may be null
    uint8_t* threat_moves;                                  // [n][A]   (written by the pass's wave)
    int32_t* status; int32_t* turn; int32_t* err;           // [n]      (the same)
    int32_t* threat; int32_t* threat_depth; int32_t* nodes; // [n]      (k_defence_rows, as everything below)
    uint8_t* reply; uint8_t* depth;                         // [n][A]
    int32_t* counts;                                        // [n][4]
};

// One wavefront per pair (position i, candidate j): j < A is the mover's reply on cell j, j == A the pass; a workgroup
// holds kPosPerWG pairs of one position. The wave replays the id, puts the mover's stone on j and runs forced_win for the
// opponent on what stands then -- check_win of the board WITH the stone is the root's status (a stone that makes a line
// or fills the board leaves a terminal root: no, at one node per iteration), and the board holds one stone more than the
// id has moves. Pairs on an occupied cell, of a terminal position or of an id with an error write 0. i, j and all that
// follows from them are wave-uniform.
// This kernel keeps its own prologue, reply step, parameter struct and mask write: its device code is the one that was timed
// before id_position, reply_search, IdBatch and store_cell_mask existed, instruction for instruction at one to three mask
// words. On the shared pieces it came out 0.9 % slower on 9x9 (IdBatch alone renumbers its SGPR spill slots throughout;
// through reply_search it needs 129 / 144 VGPRs at two / three mask words against 104 / 119 and loses a wave per SIMD).
template <int NCH>
__global__ __launch_bounds__(64 * kPosPerWG) void k_forced_defences(DefenceParams q) {
    __shared__ FwWave s_wave[kPosPerWG];
    const int wv = wg_wave();
    const int i = blockIdx.x, j = blockIdx.y * kPosPerWG + wv;     // grid: n x ceil((A + 1) / kPosPerWG)
    if (j > q.A) return;
    const size_t pr = static_cast<size_t>(i) * (q.A + 1) + j;
    const bool pass = j == q.A;
    FwWave& W = s_wave[wv];
    const int lane = lane_id();
    const int nm = __builtin_amdgcn_readfirstlane(q.nmoves[i]);
    PosR s;
    int end_ply;
    const int err = replay_moves(s, q.moves + static_cast<size_t>(i) * q.stride, nm, q.A, q.B, q.win_mark, end_ply, [](int, int) {});
    const bool ok = err == PE_OK;
    const int m = ok ? (nm & 1) : 0;       // the mover; the attacker of every search is 1 - m
    // (a position that holds a line or is full has held one, or become full, after some move: end_ply)
    const bool searched = ok && end_ply < 0 && (pass || !pos_occupied(s, j));
    if (searched && !pass) pos_toggle(s, m, j);
    // check_win of what stands now: the root of a searched pair, and for the pass also the position's own status, which is
    // asked for even where nothing is searched (taken on every legal id, like k_forced_wins: a condition here costs registers)
    const int status = ok ? check_win_board(s.bb[0], s.bb[1], q.B, q.win_mark) : 0;

    FwResult r;
    fw_search<NCH>(s, m ^ 1, pass ? nm : nm + 1, status, W, q.B, q.A, q.win_mark, searched, q.max_depth, q.max_nodes, r);
    if (lane == 0) q.pair[pr] = searched ? fw_word(r) : 0u;
    if (!pass) return;
    if (lane == 0) {
        if (q.status) q.status[i] = status;
        if (q.turn) q.turn[i] = m;
        if (q.err) q.err[i] = err;
    }
    if (q.threat_moves) {
        const bool win = r.result == FW_WIN;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int cell = lane + 64 * c;
            if (cell < q.A) q.threat_moves[static_cast<size_t>(i) * q.A + cell] = static_cast<uint8_t>(win && ((r.won[c] >> lane) & 1ull));
        }
    }
}

// One wavefront per position: the words of its A + 1 pairs into reply / depth [A], counts [4], nodes and the threat.
// Ballots and integer sums only: the result does not depend on any order.
template <int NCH>
__global__ __launch_bounds__(64 * kPosPerWG) void k_defence_rows(DefenceParams q) {
    const int i = wave_item();
    if (i >= q.n) return;
    const int lane = lane_id();
    const int A = q.A;
    const uint32_t* pair = q.pair + static_cast<size_t>(i) * (A + 1);
    const uint32_t pw = pair[A];           // the pass
    int n_empty = 0, n_safe = 0, n_loses = 0, n_unknown = 0;
    int nodes_l = lane == 0 ? fw_word_nodes(pw) : 0;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int cell = lane + 64 * c;
        const uint32_t w = cell < A ? pair[cell] : 0u;
        const int rep = fw_word_reply(w);
        n_empty += __popcll(__ballot(rep != FD_NONE));
        n_safe += __popcll(__ballot(rep == FD_SAFE));
        n_loses += __popcll(__ballot(rep == FD_LOSES));
        n_unknown += __popcll(__ballot(rep == FD_UNKNOWN));
        nodes_l += fw_word_nodes(w);
        if (cell < A) {
            if (q.reply) q.reply[static_cast<size_t>(i) * A + cell] = static_cast<uint8_t>(rep);
            if (q.depth) q.depth[static_cast<size_t>(i) * A + cell] = static_cast<uint8_t>(fw_word_depth(w));
        }
    }
    const int nodes = wave_sum_i(nodes_l);   // <= 226 * 65536
    if (lane == 0) {
        if (q.threat) q.threat[i] = pw ? fw_word_result(pw) : 0;
        if (q.threat_depth) q.threat_depth[i] = fw_word_depth(pw);
        if (q.nodes) q.nodes[i] = nodes;
        if (q.counts) {
            int32_t* cn = q.counts + static_cast<size_t>(i) * 4;
            cn[0] = n_empty; cn[1] = n_safe; cn[2] = n_loses; cn[3] = n_unknown;
        }
    }
}

}  // namespace ao

struct ao_positions : ao::HandleBase {
    int B = 0, A = 0, C = 0, win_mark = 0, cap = 0, device = 0;
    hipStream_t stream = nullptr;
    ao::DevPool pool;
    int32_t* d_moves = nullptr;    // [cap][A]
    int32_t* d_n = nullptr;        // [cap]
    int32_t* d_i32 = nullptr;      // [4][cap]: status, end_ply, turn, err (d_status .. d_err below)
    uint8_t* d_cells0 = nullptr;   // [cap][A] bytes, two of them: whatever per-cell rows an entry point's kernels write
    uint8_t* d_cells1 = nullptr;   //          (d_cells0 also as int8 boards: d_board below)
    ao::DevBuf<float> d_planes{&pool};     // [cap][C][A]   -- the three below: allocated by the first ao_positions_evaluate
    ao::DevBuf<float> d_policy{&pool};     // [cap][A]
    ao::DevBuf<float> d_value{&pool};      // [cap]
    ao::DevBuf<float> d_mean{&pool};       // [cap / 8][A] policy, then [cap / 8] value -- allocated by the first ao_positions_evaluate_sym with nsym 8
    ao::DevBuf<int32_t> d_counts{&pool};   // [cap][8]      -- allocated by the first ao_positions_audit
    ao::DevBuf<int32_t> d_forced{&pool};   // [5][cap]: ForcedSlot -- these two: by the first ao_positions_forced_wins
    ao::DevBuf<int16_t> d_line{&pool};     // [cap][2 * 16 - 1]
    ao::DevBuf<uint32_t> d_pair{&pool};    // [cap][A + 1]  -- the three below: allocated by the first ao_positions_forced_defences
    ao::DevBuf<int32_t> d_defence{&pool};  // [3][cap]: DefenceSlot, then counts [cap][4]
    ao::DevBuf<uint8_t> d_depth{&pool};    // [cap][A]
    std::vector<int32_t> h_moves, h_n;
};

namespace {

// the staging buffers by what they hold: slot k of an int32 [..][cap] buffer
int32_t* slot(const ao_positions* p, int32_t* base, int k) { return base + static_cast<size_t>(k) * p->cap; }
int32_t* d_status(const ao_positions* p) { return slot(p, p->d_i32, 0); }
int32_t* d_end_ply(const ao_positions* p) { return slot(p, p->d_i32, 1); }
int32_t* d_turn(const ao_positions* p) { return slot(p, p->d_i32, 2); }
int32_t* d_err(const ao_positions* p) { return slot(p, p->d_i32, 3); }
int8_t* d_board(const ao_positions* p) { return reinterpret_cast<int8_t*>(p->d_cells0); }   // boards in (check_win), boards out (from_moves)
enum ForcedSlot { F_RESULT, F_DEPTH, F_MOVE, F_LINE_LEN, F_NODES, F_SLOTS };
int32_t* d_forced(const ao_positions* p, ForcedSlot k) { return slot(p, p->d_forced.p, k); }
enum DefenceSlot { D_THREAT, D_THREAT_DEPTH, D_NODES, D_COUNTS, D_SLOTS = D_COUNTS + 4 };   // (counts: four words per position)
int32_t* d_defence(const ao_positions* p, DefenceSlot k) { return slot(p, p->d_defence.p, k); }

ao::IdBatch staged_ids(const ao_positions* p, int m) { return ao::IdBatch{p->d_moves, p->d_n, m, p->A, p->B, p->A, p->win_mark}; }
dim3 wave_grid(int waves) { return dim3(static_cast<unsigned>((waves + ao::kPosPerWG - 1) / ao::kPosPerWG)); }
const dim3 kBlock(64 * ao::kPosPerWG);

// positions [first, first + m) of the caller's move lists -> d_moves [m][A] / d_n [m] (lists the kernel refuses by their
// length are uploaded empty: only the length is looked at)
int stage_moves(ao_positions* p, const char* who, const int32_t* host_moves, int32_t stride, const int32_t* host_n, int64_t first, int m) {
    const int A = p->A;
    p->h_moves.assign(static_cast<size_t>(m) * A, 0);
    p->h_n.resize(static_cast<size_t>(m));
    for (int k = 0; k < m; ++k) {
        const int32_t nm = host_n[first + k];
        p->h_n[static_cast<size_t>(k)] = nm;
        if (nm < 1 || nm > A) continue;
        if (nm > stride) return p->fail(std::string(who) + ": position " + std::to_string(first + k) + " has more moves than `stride`");
        std::memcpy(p->h_moves.data() + static_cast<size_t>(k) * A, host_moves + (first + k) * static_cast<int64_t>(stride), sizeof(int32_t) * nm);
    }
    AO_HIP(p, hipMemcpyAsync(p->d_moves, p->h_moves.data(), sizeof(int32_t) * m * A, hipMemcpyHostToDevice, p->stream));
    AO_HIP(p, hipMemcpyAsync(p->d_n, p->h_n.data(), sizeof(int32_t) * m, hipMemcpyHostToDevice, p->stream));
    return 0;
}

// what every id-batch entry point is called with
struct IdArgs { const char* who; const int32_t* moves; int32_t stride; const int32_t* n_moves; int32_t n;
                int32_t per_chunk = 0; };   // ids of one chunk; 0: the handle's capacity
// its first check; what is particular to an entry point (limits, the network) is checked by the entry point after this one
bool negative_ids(ao_positions* p, const IdArgs& c, const char* noun = "position") {
    return (c.n < 0 || c.stride < 0) && p->fail(std::string(c.who) + ": negative " + noun + " count or stride");
}
bool bad_limits(ao_positions* p, const char* who, int max_depth, int max_nodes) {
    const std::string bad = ao::fw_limits_error(who, max_depth, max_nodes);
    return !bad.empty() && p->fail(bad);
}
// one output of a chunk: `per` elements of `size` bytes per position from `dev` into the caller's whole array (null: not asked for)
struct Fetch { void* host; const void* dev; size_t per, size; };
template <class T>
Fetch fetch(T* host, const T* dev, size_t per = 1) { return Fetch{host, dev, per, sizeof(T)}; }

// Every id-batch entry point after its argument checks: n == 0 is a no-op, a null move buffer an error, then the caller's ids
// go through the device `cap` at a time. prepare() runs once on the handle's device before the first chunk (reserve,
// synchronise); chunk(first, m, out) launches on the m staged ids of positions [first, first + m) and names the outputs to
// fetch; after(first, m) runs once they have arrived. prepare and chunk return non-zero after p->fail.
template <class Prepare, class Chunk, class After>
int for_id_chunks(ao_positions* p, const IdArgs& c, Prepare&& prepare, Chunk&& chunk, After&& after) {
    if (c.n == 0) return 0;
    if (!c.n_moves || (!c.moves && c.stride > 0)) return p->fail(std::string(c.who) + ": null move buffer");
    AO_HIP(p, hipSetDevice(p->device));
    if (prepare()) return 1;
    std::vector<Fetch> out;
    const int per_chunk = c.per_chunk > 0 ? c.per_chunk : p->cap;
    for (int64_t first = 0; first < c.n; first += per_chunk) {
        const int m = static_cast<int>(std::min<int64_t>(per_chunk, c.n - first));
        if (stage_moves(p, c.who, c.moves, c.stride, c.n_moves, first, m)) return 1;
        out.clear();
        if (chunk(first, m, out)) return 1;
        AO_HIP(p, hipGetLastError());
        for (const Fetch& f : out)
            if (f.host)
                AO_HIP(p, hipMemcpyAsync(static_cast<char*>(f.host) + static_cast<size_t>(first) * f.per * f.size, f.dev,
                                         static_cast<size_t>(m) * f.per * f.size, hipMemcpyDeviceToHost, p->stream));
        // the staging buffers are reused by the next chunk, and what a kernel wrote into the caller's device memory (planes) is
        // complete for any stream
        AO_HIP(p, hipStreamSynchronize(p->stream));
        after(first, m);
    }
    return 0;
}
template <class Prepare, class Chunk>
int for_id_chunks(ao_positions* p, const IdArgs& c, Prepare&& prepare, Chunk&& chunk) {
    return for_id_chunks(p, c, prepare, chunk, [](int64_t, int) {});
}
const auto kNothing = [] { return 0; };

// k_positions_from_moves on the m staged ids: the outputs asked for land in d_i32, d_board, d_cells1 (legal) and `planes`
int launch_from_moves(ao_positions* p, int m, bool status, bool end_ply, bool turn, bool board, bool legal, float* planes, bool err,
                      bool bad_as_empty, int nsym = 1) {
    ao::PositionsParams q{};
    q.nsym = nsym;
    q.ids = staged_ids(p, m);
    q.C = p->C;
    q.bad_as_empty = bad_as_empty ? 1 : 0;
    q.status = status ? d_status(p) : nullptr;
    q.end_ply = end_ply ? d_end_ply(p) : nullptr;
    q.turn = turn ? d_turn(p) : nullptr;
    q.err = err ? d_err(p) : nullptr;
    q.board = board ? d_board(p) : nullptr;
    q.legal = legal ? p->d_cells1 : nullptr;
    q.planes = planes;
    AO_DISPATCH_NCH(ao::nch_of_cells(p->A), hipLaunchKernelGGL(ao::k_positions_from_moves<NCH>, wave_grid(m), kBlock, 0, p->stream, q));
    AO_HIP(p, hipGetLastError());
    return 0;
}

}  // namespace

static int positions_create_impl(ao_positions* p, int board, int inplanes, int win_mark, int capacity, int device) {
    p->device = device;
    if (board < 3 || board > ao::kMaxBoard) return p->fail("board must be in 3..15");
    if (inplanes < 1 || inplanes > ao::kMaxPlanes) return p->fail("inplanes must be in 1..9 (the plane encoder keeps eight plies of history)");
    if (win_mark < 3 || win_mark > 5 || win_mark > board) return p->fail("win_mark must be in 3..5 and at most the board size");
    if (capacity < 1) return p->fail("capacity must be >= 1");
    p->B = board; p->A = board * board; p->C = inplanes; p->win_mark = win_mark; p->cap = capacity;
    const size_t cap = static_cast<size_t>(capacity), A = static_cast<size_t>(p->A);
    AO_HIP(p, hipSetDevice(device));
    AO_HIP(p, hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
    return p->pool.alloc(p, &p->d_moves, cap * A) || p->pool.alloc(p, &p->d_n, cap) || p->pool.alloc(p, &p->d_i32, 4 * cap) ||
           p->pool.alloc(p, &p->d_cells0, cap * A) || p->pool.alloc(p, &p->d_cells1, cap * A);
}

extern "C" {

void ao_positions_destroy(ao_positions* p) {
    if (!p) return;
    hipSetDevice(p->device);
    if (p->stream) hipStreamSynchronize(p->stream);
    p->pool.free_all();
    if (p->stream) hipStreamDestroy(p->stream);
    delete p;
}

int ao_positions_create(int board, int inplanes, int win_mark, int capacity, int device, ao_positions** out) {
    ao_positions* p = new ao_positions;
    return ao::finish_create(p, positions_create_impl(p, board, inplanes, win_mark, capacity, device), out, ao_positions_destroy,
                             "ao_positions_create: ");
}

const char* ao_positions_last_error(const ao_positions* p) { return p ? p->err.c_str() : ao::create_error<ao_positions>().c_str(); }

// (boards are staged, not ids: a chunk loop of its own)
int ao_positions_check_win(ao_positions* p, const int8_t* host_boards, int32_t n, int32_t* host_win) {
    if (n < 0) return p->fail("ao_positions_check_win: negative position count");
    if (n == 0) return 0;
    if (!host_boards || !host_win) return p->fail("ao_positions_check_win: null buffer");
    AO_HIP(p, hipSetDevice(p->device));
    const size_t A = static_cast<size_t>(p->A);
    for (int64_t first = 0; first < n; first += p->cap) {
        const int m = static_cast<int>(std::min<int64_t>(p->cap, n - first));
        AO_HIP(p, hipMemcpyAsync(d_board(p), host_boards + first * A, static_cast<size_t>(m) * A, hipMemcpyHostToDevice, p->stream));
        hipLaunchKernelGGL(ao::k_check_win_boards, wave_grid(m), kBlock, 0, p->stream, d_board(p), m, p->B, p->win_mark, d_status(p));
        AO_HIP(p, hipGetLastError());
        AO_HIP(p, hipMemcpyAsync(host_win + first, d_status(p), sizeof(int32_t) * m, hipMemcpyDeviceToHost, p->stream));
        AO_HIP(p, hipStreamSynchronize(p->stream));   // the staging buffers are reused by the next chunk
    }
    return 0;
}

int ao_positions_from_moves(ao_positions* p, const int32_t* host_moves, int32_t stride, const int32_t* host_n, int32_t n,
                            int32_t* host_status, int32_t* host_end_ply, int32_t* host_turn, int8_t* host_board,
                            uint8_t* host_legal, float* dev_planes_nchw, int32_t* host_err) {
    const size_t A = static_cast<size_t>(p->A);
    const IdArgs call{"ao_positions_from_moves", host_moves, stride, host_n, n};
    if (negative_ids(p, call)) return 1;
    return for_id_chunks(
        p, call,
        [&] {
            // the caller's plane buffer may be memory that work queued on another stream still uses (a caching allocator hands such out)
            if (dev_planes_nchw) AO_HIP(p, hipDeviceSynchronize());
            return 0;
        },
        [&](int64_t first, int m, std::vector<Fetch>& out) {
            float* planes = dev_planes_nchw ? dev_planes_nchw + static_cast<size_t>(first) * p->C * A : nullptr;
            if (launch_from_moves(p, m, host_status, host_end_ply, host_turn, host_board, host_legal, planes, host_err, false)) return 1;
            out = {fetch(host_status, d_status(p)), fetch(host_end_ply, d_end_ply(p)), fetch(host_turn, d_turn(p)),
                   fetch(host_err, d_err(p)), fetch(host_board, d_board(p), A), fetch(host_legal, p->d_cells1, A)};
            return 0;
        });
}

int ao_positions_win_cells(ao_positions* p, const int32_t* host_moves, int32_t stride, const int32_t* host_n, int32_t n,
                           uint8_t* host_mine, uint8_t* host_theirs, int32_t* host_status, int32_t* host_turn, int32_t* host_err) {
    const size_t A = static_cast<size_t>(p->A);
    const IdArgs call{"ao_positions_win_cells", host_moves, stride, host_n, n};
    if (negative_ids(p, call)) return 1;
    return for_id_chunks(p, call, kNothing,
                         [&](int64_t, int m, std::vector<Fetch>& out) {
                             ao::TacticsParams q{};
                             q.ids = staged_ids(p, m);
                             q.mine = p->d_cells0; q.theirs = p->d_cells1;
                             q.status = d_status(p); q.turn = d_turn(p); q.err = d_err(p);
                             AO_DISPATCH_NCH(ao::nch_of_cells(p->A), hipLaunchKernelGGL(ao::k_win_cells<NCH>, wave_grid(m), kBlock, 0, p->stream, q));
                             out = {fetch(host_mine, q.mine, A), fetch(host_theirs, q.theirs, A), fetch(host_status, q.status),
                                    fetch(host_turn, q.turn), fetch(host_err, q.err)};
                             return 0;
                         });
}

int ao_positions_audit(ao_positions* p, const int32_t* host_moves, int32_t stride, const int32_t* host_n, int32_t n,
                       uint8_t* host_flags, int32_t* host_counts, int32_t* host_err) {
    const size_t A = static_cast<size_t>(p->A), cap = static_cast<size_t>(p->cap);
    const IdArgs call{"ao_positions_audit", host_moves, stride, host_n, n};
    if (negative_ids(p, call, "record")) return 1;
    return for_id_chunks(p, call, [&] { return p->d_counts.reserve(p, cap * 8); },
                         [&](int64_t, int m, std::vector<Fetch>& out) {
                             ao::TacticsParams q{};
                             q.ids = staged_ids(p, m);
                             q.flags = p->d_cells1; q.counts = p->d_counts.p; q.err = d_err(p);
                             AO_DISPATCH_NCH(ao::nch_of_cells(p->A), hipLaunchKernelGGL(ao::k_audit_games<NCH>, wave_grid(m), kBlock, 0, p->stream, q));
                             out = {fetch(host_flags, q.flags, A), fetch(host_counts, q.counts, 8), fetch(host_err, q.err)};
                             return 0;
                         });
}

int ao_positions_forced_wins(ao_positions* p, const int32_t* host_moves, int32_t stride, const int32_t* host_n, int32_t n,
                             int32_t max_depth, int32_t max_nodes, int32_t* host_result, int32_t* host_depth, int32_t* host_move,
                             uint8_t* host_moves_mask, int16_t* host_line, int32_t* host_line_len, int32_t* host_nodes,
                             int32_t* host_status, int32_t* host_turn, int32_t* host_err) {
    const size_t A = static_cast<size_t>(p->A), cap = static_cast<size_t>(p->cap);
    const IdArgs call{"ao_positions_forced_wins", host_moves, stride, host_n, n};
    if (negative_ids(p, call) || bad_limits(p, call.who, max_depth, max_nodes)) return 1;
    return for_id_chunks(
        p, call, [&] { return p->d_forced.reserve(p, F_SLOTS * cap) || p->d_line.reserve(p, cap * (2 * ao::kFwMaxDepth - 1)); },
        [&](int64_t, int m, std::vector<Fetch>& out) {
            ao::ForcedParams q{};
            q.ids = staged_ids(p, m);
            q.max_depth = max_depth; q.max_nodes = max_nodes; q.line_stride = 2 * max_depth - 1;
            q.result = d_forced(p, F_RESULT); q.depth = d_forced(p, F_DEPTH); q.move = d_forced(p, F_MOVE);
            q.line_len = d_forced(p, F_LINE_LEN); q.nodes = d_forced(p, F_NODES);
            q.status = d_status(p); q.turn = d_turn(p); q.err = d_err(p);
            q.mask = p->d_cells0;
            q.line = p->d_line.p;
            AO_DISPATCH_NCH(ao::nch_of_cells(p->A), hipLaunchKernelGGL(ao::k_forced_wins<NCH>, wave_grid(m), kBlock, 0, p->stream, q));
            out = {fetch(host_result, q.result), fetch(host_depth, q.depth), fetch(host_move, q.move), fetch(host_line_len, q.line_len),
                   fetch(host_nodes, q.nodes), fetch(host_moves_mask, q.mask, A), fetch(host_line, q.line, static_cast<size_t>(q.line_stride)),
                   fetch(host_status, q.status), fetch(host_turn, q.turn), fetch(host_err, q.err)};
            return 0;
        });
}

int ao_positions_forced_defences(ao_positions* p, const int32_t* host_moves, int32_t stride, const int32_t* host_n, int32_t n,
                                 int32_t max_depth, int32_t max_nodes, int32_t* host_threat, int32_t* host_threat_depth,
                                 uint8_t* host_threat_moves, uint8_t* host_reply, uint8_t* host_depth, int32_t* host_counts,
                                 int32_t* host_nodes, int32_t* host_status, int32_t* host_turn, int32_t* host_err) {
    const size_t A = static_cast<size_t>(p->A), cap = static_cast<size_t>(p->cap);
    const IdArgs call{"ao_positions_forced_defences", host_moves, stride, host_n, n};
    if (negative_ids(p, call) || bad_limits(p, call.who, max_depth, max_nodes)) return 1;
    return for_id_chunks(
        p, call, [&] { return p->d_pair.reserve(p, cap * (A + 1)) || p->d_defence.reserve(p, D_SLOTS * cap) || p->d_depth.reserve(p, cap * A); },
        [&](int64_t, int m, std::vector<Fetch>& out) {
            // k_forced_defences on the (A + 1) pairs of each of the m staged ids, then k_defence_rows on the ids
            ao::DefenceParams q{};
            q.moves = p->d_moves; q.nmoves = p->d_n;
            q.n = m; q.stride = p->A; q.B = p->B; q.A = p->A; q.win_mark = p->win_mark;
            q.max_depth = max_depth; q.max_nodes = max_nodes;
            q.pair = p->d_pair.p;
            q.threat_moves = p->d_cells0;
            q.status = d_status(p); q.turn = d_turn(p); q.err = d_err(p);
            q.threat = d_defence(p, D_THREAT); q.threat_depth = d_defence(p, D_THREAT_DEPTH); q.nodes = d_defence(p, D_NODES);
            q.counts = d_defence(p, D_COUNTS);
            q.reply = p->d_cells1; q.depth = p->d_depth.p;
            const dim3 pair_grid(static_cast<unsigned>(m), wave_grid(p->A + 1).x);
            AO_DISPATCH_NCH(ao::nch_of_cells(p->A), hipLaunchKernelGGL(ao::k_forced_defences<NCH>, pair_grid, kBlock, 0, p->stream, q);
                            hipLaunchKernelGGL(ao::k_defence_rows<NCH>, wave_grid(m), kBlock, 0, p->stream, q));
            out = {fetch(host_threat, q.threat), fetch(host_threat_depth, q.threat_depth), fetch(host_nodes, q.nodes),
                   fetch(host_counts, q.counts, 4), fetch(host_threat_moves, q.threat_moves, A), fetch(host_reply, q.reply, A),
                   fetch(host_depth, q.depth, A), fetch(host_status, q.status), fetch(host_turn, q.turn), fetch(host_err, q.err)};
            return 0;
        });
}

}  // extern "C"

// nsym 1: the network's answer on each position as it stands. nsym 8: the mean over the eight symmetries -- eight rows per
// position through ONE forward (so a chunk holds capacity / 8 positions), brought back and added up by k_sym_mean.
static int evaluate_impl(ao_positions* p, const char* who, ao_net* net, const int32_t* host_moves, int32_t stride, const int32_t* host_n,
                         int32_t n, int nsym, float* host_policy, float* host_value, int32_t* host_status, int32_t* host_err) {
    const size_t A = static_cast<size_t>(p->A), cap = static_cast<size_t>(p->cap);
    const std::string w(who);
    if (nsym != 1 && nsym != 8) return p->fail(w + ": nsym must be 1 or 8");
    if (nsym == 8 && p->cap < 8) return p->fail(w + ": eight rows per position need a capacity of at least 8");
    const IdArgs call{who, host_moves, stride, host_n, n, nsym == 8 ? p->cap / 8 : 0};
    if (negative_ids(p, call)) return 1;
    if (!net) return p->fail(w + ": null network");
    std::string why;
    if (ao::net_check(net, p->B, p->C, p->device, &why)) return p->fail(w + ": " + why);
    if (n == 0) return 0;
    if (!host_n || (!host_moves && stride > 0) || !host_policy || !host_value) return p->fail(w + ": null buffer");
    std::vector<int32_t> own_err(host_err ? 0 : static_cast<size_t>(n));
    int32_t* err = host_err ? host_err : own_err.data();
    const size_t cap8 = cap / 8;
    return for_id_chunks(
        p, call,
        [&]() -> int {
            AO_HIP(p, hipDeviceSynchronize());   // the network's workspace may still serve a forward queued on another stream
            return p->d_planes.reserve(p, cap * p->C * A) || p->d_policy.reserve(p, cap * A) || p->d_value.reserve(p, cap) ||
                   (nsym == 8 && p->d_mean.reserve(p, cap8 * (A + 1)));
        },
        [&](int64_t, int m, std::vector<Fetch>& out) {
            // a position with an error is fed as the empty board: its row must not disturb the rest of the chunk
            if (launch_from_moves(p, m, true, false, false, false, false, p->d_planes.p, true, true, nsym)) return 1;
            if (ao_net_forward(net, p->d_planes.p, m * nsym, p->d_policy.p, p->d_value.p, p->stream))
                return p->fail(w + ": " + ao_net_last_error(net));
            const float* policy = p->d_policy.p;
            const float* value = p->d_value.p;
            if (nsym == 8) {
                float* mp = p->d_mean.p;
                float* mv = p->d_mean.p + cap8 * A;
                AO_DISPATCH_NCH(ao::nch_of_cells(p->A), hipLaunchKernelGGL(ao::k_sym_mean<NCH>, wave_grid(m), kBlock, 0, p->stream, policy, value,
                                                                           m, p->B, mp, mv));
                policy = mp;
                value = mv;
            }
            out = {fetch(host_policy, policy, A), fetch(host_value, value), fetch(host_status, d_status(p)), fetch(err, d_err(p))};
            return 0;
        },
        [&](int64_t first, int m) {
            for (int64_t k = first; k < first + m; ++k) {
                if (err[k] == 0) continue;
                std::fill_n(host_policy + k * A, A, 0.f);
                host_value[k] = 0.f;
            }
        });
}

extern "C" {

int ao_positions_evaluate(ao_positions* p, ao_net* net, const int32_t* host_moves, int32_t stride, const int32_t* host_n,
                          int32_t n, float* host_policy, float* host_value, int32_t* host_status, int32_t* host_err) {
    return evaluate_impl(p, "ao_positions_evaluate", net, host_moves, stride, host_n, n, 1, host_policy, host_value, host_status, host_err);
}

int ao_positions_evaluate_sym(ao_positions* p, ao_net* net, const int32_t* host_moves, int32_t stride, const int32_t* host_n,
                              int32_t n, int32_t nsym, float* host_policy, float* host_value, int32_t* host_status, int32_t* host_err) {
    return evaluate_impl(p, "ao_positions_evaluate_sym", net, host_moves, stride, host_n, n, nsym, host_policy, host_value, host_status,
                         host_err);
}

}  // extern "C"
