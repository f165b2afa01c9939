// positions.hip -- the stateless, batched "position" layer beside the search: rule status, legal moves, input planes and the
// network's evaluation of positions the CALLER names, no tree and no game involved.
//
// One wavefront (64 lanes) owns one position, kPosPerWG positions per workgroup, nothing shared between them (no LDS but
// the search stack of k_forced_wins / k_forced_defences, one per wave).
//
// Reference map (paths relative to /root/reference/2_AlphaOmok/):
//   k_check_win_boards      utils.py:30-59 (check_win) on raw boards: the FULL window scan, row-major, black before white
//                           inside a window -- boards need not be reachable in play, so the scan order decides
//   k_positions_from_moves  utils.py:171-179 (get_board) + utils.py:182-186 (get_turn) + utils.py:22-27 (legal_actions, as a
//                           mask: the CPython set ORDER is the tree kernels' business, legal_order) + utils.py:30-59
//                           (check_win of the final board, and of every prefix through the incremental win_after_move of
//                           the tree kernels) + utils.py:139-168 (get_state_pt, encode_planes of the tree kernels)
//   ao_positions_evaluate   agents.py:171-178 for n positions at once: planes on the device, then the ordinary forward
//   k_win_cells, k_audit_games  no counterpart: the cells that win at once and the per-ply tactical flags of game records,
//                           defined through utils.py:30-59 (check_win of the board with one more stone)
//   k_forced_wins           no counterpart: forced wins by continuous fours, a depth-first search per position over the same
//                           winning cells (utils.forced_win of this package is the host definition)
//   k_forced_defences, k_defence_rows  no counterpart: which replies hold against the opponent's forced win -- the same
//                           search (fw_search) for every (position, reply) pair and for the pass, one wavefront each, then
//                           one wavefront per position that gathers its pairs (utils.forced_defences is the host definition)
//
// The bitboards, pos_place, pos_occupied, win_after_move and encode_planes are the tree kernels' own (tree_device.hpp): a
// position described here is the position the search would hold.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/omok_hip.h"
#include "host_handle.hpp"
#include "tree_device.hpp"

namespace ao {

int net_check(const ao_net* n, int board, int inplanes, int device, std::string* why);   // net.hip

constexpr int kPosPerWG = 4;
constexpr int kMaxWinMark = 5;   // ao_positions_create: win_mark 3..5

// per-position error codes (ao_positions_from_moves)
enum : int32_t { PE_OK = 0, PE_RANGE = 1, PE_OCCUPIED = 2, PE_LENGTH = 3 };

// `len` (1..5) bits of a bitboard from bit `off` on (off + len <= 256); no dynamically indexed access (see pick4)
__device__ __forceinline__ unsigned bb_bits(const uint64_t (&bb)[kBBWords], int off, int len) {
    const int w = off >> 6, sh = off & 63;
    const uint64_t lo = pick4(bb[0], bb[1], bb[2], bb[3], w);
    const uint64_t hi = (w < kBBWords - 1) ? pick4(bb[0], bb[1], bb[2], bb[3], w + 1) : 0ull;
    uint64_t v = lo >> sh;
    v |= sh ? (hi << (64 - sh)) : 0ull;
    return static_cast<unsigned>(v) & ((1u << len) - 1u);
}

// any complete row, column or diagonal in a k x k window given as k*k bits (bit r*k + c)
__device__ __forceinline__ bool window_has_line(unsigned m, int k) {
    const unsigned rowm = (1u << k) - 1u;
    unsigned colm = 0u, d1 = 0u, d2 = 0u;
    for (int r = 0; r < k; ++r) {
        colm |= 1u << (r * k);
        d1 |= 1u << (r * k + r);
        d2 |= 1u << (r * k + (k - 1 - r));
    }
    bool any = ((m & d1) == d1) || ((m & d2) == d2);
    for (int i = 0; i < k; ++i) {
        const unsigned rm = rowm << (i * k), cm = colm << i;
        any = any || ((m & rm) == rm) || ((m & cm) == cm);
    }
    return any;
}

// utils.check_win (utils.py:30-59) of a whole board, wave-uniform (all 64 lanes call): lane = window, 64 windows per pass
// in row-major order; the first window holding a line decides, black before white inside it. Overlines count: they
// contain a window's line. No line anywhere: 3 on a full board, else 0.
__device__ __forceinline__ int check_win_board(const uint64_t (&black)[kBBWords], const uint64_t (&white)[kBBWords], int B, int k) {
    const int lane = lane_id();
    const int W = B - k + 1;
    const int nw = W > 0 ? W * W : 0;
    for (int base = 0; base < nw; base += 64) {
        const int wi = base + lane;
        const bool in = wi < nw;
        const int wr = in ? wi / W : 0, wc = in ? wi % W : 0;
        unsigned mb = 0u, mw = 0u;
        for (int r = 0; r < k; ++r) {
            const int off = (wr + r) * B + wc;
            mb |= bb_bits(black, off, k) << (r * k);
            mw |= bb_bits(white, off, k) << (r * k);
        }
        const bool hb = in && window_has_line(mb, k);
        const bool hw = in && window_has_line(mw, k);
        const uint64_t hit = __ballot(hb || hw), hitb = __ballot(hb);
        if (hit) {
            const int first = __ffsll(static_cast<long long>(hit)) - 1;
            return ((hitb >> first) & 1ull) ? 1 : 2;
        }
    }
    int stones = 0;
#pragma unroll
    for (int i = 0; i < kBBWords; ++i) stones += __popcll(black[i]) + __popcll(white[i]);
    return stones == B * B ? 3 : 0;
}

// boards int8 [n][A] (+1 black, -1 white, anything else empty) -> win int32 [n]
__global__ __launch_bounds__(64 * kPosPerWG) void k_check_win_boards(const int8_t* __restrict__ boards, int n, int B, int win_mark,
                                                                     int32_t* __restrict__ win) {
    const int i = blockIdx.x * kPosPerWG + __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
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
// the first move after which check_win is non-zero, -1 if there is none.
__device__ __forceinline__ int replay_moves(PosR& s, const int32_t* __restrict__ mv, int nm, int A, int B, int win_mark, int& end_ply) {
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
            pos_place(s, m);
            // (every earlier position was not terminal, which is what the incremental test asks for)
            if (end_ply < 0 && win_after_move(s, m, B, win_mark) != 0) end_ply = base + j;
        }
    }
    if (err != PE_OK) pos_clear(s);
    return err;
}

struct PositionsParams {
    const int32_t* moves;   // [n][stride]: row i = root_id[1:] of position i
    const int32_t* nmoves;  // [n]
    int n, stride, B, A, C, win_mark;
    int bad_as_empty;       // planes of a position with an error: 0 = zeros, 1 = the planes of the empty board (ao_positions_evaluate)
    // outputs, any may be null
    int32_t* status; int32_t* end_ply; int32_t* turn; int32_t* err;
    int8_t* board;          // [n][A]
    uint8_t* legal;         // [n][A]
    float* planes;          // [n][C][A]
};

template <int NCH>
__global__ __launch_bounds__(64 * kPosPerWG) void k_positions_from_moves(PositionsParams q) {
    const int i = blockIdx.x * kPosPerWG + __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
    if (i >= q.n) return;
    const int lane = lane_id();
    const int nm = __builtin_amdgcn_readfirstlane(q.nmoves[i]);
    PosR s;
    int end_ply;
    const int err = replay_moves(s, q.moves + static_cast<size_t>(i) * q.stride, nm, q.A, q.B, q.win_mark, end_ply);
    const bool ok = err == PE_OK;
    const int status = ok ? check_win_board(s.bb[0], s.bb[1], q.B, q.win_mark) : 0;
    if (lane == 0) {
        if (q.status) q.status[i] = status;
        if (q.end_ply) q.end_ply[i] = ok ? end_ply : 0;
        if (q.turn) q.turn[i] = ok ? (nm & 1) : 0;
        if (q.err) q.err[i] = err;
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int cell = lane + 64 * c;
        if (cell >= q.A) continue;
        const int b0 = static_cast<int>((s.bb[0][c] >> lane) & 1ull), b1 = static_cast<int>((s.bb[1][c] >> lane) & 1ull);
        if (q.board) q.board[static_cast<size_t>(i) * q.A + cell] = static_cast<int8_t>(b0 - b1);
        if (q.legal) q.legal[static_cast<size_t>(i) * q.A + cell] = static_cast<uint8_t>(ok && !(b0 | b1));
    }
    if (q.planes) {
        if (ok || q.bad_as_empty) {
            TreeParams tp{};   // the encoder's view of the batch: row i of a plain NCHW plane batch
            tp.C = q.C;
            tp.A = q.A;
            tp.batch_nchw = q.planes;
            encode_planes<NCH>(tp, i, s, i);
        } else {
            float* out = q.planes + static_cast<size_t>(i) * q.C * q.A;
            for (int idx = lane; idx < q.C * q.A; idx += 64) out[idx] = 0.f;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// tactical cells: which empty cells win at once. No reference counterpart; the definition is utils.check_win
// (utils.py:30-59) of the board with one more stone -- see ao_positions_win_cells in omok_hip.h.
// ---------------------------------------------------------------------------------------------------------------------
// flag bits of one audited ply (ao_positions_audit)
enum : int { TF_WIN_AVAILABLE = 1, TF_WIN_TAKEN = 2, TF_THREAT = 4, TF_BLOCKED = 8, TF_LOST = 16 };

// The empty cells on which a stone of `colour` (0 black / 1 white) completes a line of win_mark or more, as 64-cell mask
// words (wave-uniform; all 64 lanes call). Lane = cell, NCH passes. In each direction the lane counts the colour's
// contiguous stones on either side of its cell, up to win_mark - 1 a side, every probed cell checked by ROW and COLUMN (a
// run that reaches column B-1 does not go on at column 0 of the next row); 1 + left + right >= win_mark wins, overlines
// included. On a position without a line that is check_win == colour + 1 after the stone: only a line through the new
// stone can be new, and it is the colour's. The ballot of the predicate is the mask word.
template <int NCH>
__device__ __forceinline__ void winning_cells(const PosR& s, int colour, int B, int A, int win_mark, uint64_t (&out)[kBBWords]) {
    const int lane = lane_id();
    // the colour's stones by a mask blend and by value (see win_after_move_by and pick4)
    const uint64_t mk = 0ull - static_cast<uint64_t>(colour & 1);
    const uint64_t a0 = (s.bb[0][0] & ~mk) | (s.bb[1][0] & mk), a1 = (s.bb[0][1] & ~mk) | (s.bb[1][1] & mk);
    const uint64_t a2 = (s.bb[0][2] & ~mk) | (s.bb[1][2] & mk), a3 = (s.bb[0][3] & ~mk) | (s.bb[1][3] & mk);
#pragma unroll
    for (int c = 0; c < kBBWords; ++c) {
        if (c >= NCH) { out[c] = 0ull; continue; }
        const int cell = lane + 64 * c;
        const bool empty = cell < A && !(((s.bb[0][c] | s.bb[1][c]) >> lane) & 1ull);
        const int r = cell / B, col = cell % B;
        bool win = false;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const int dr = (d == 0) ? 0 : 1;
            const int dc = (d == 0) ? 1 : (d == 1) ? 0 : (d == 2) ? 1 : -1;
            int run = 1;
#pragma unroll
            for (int side = -1; side <= 1; side += 2) {
                bool on = empty;
#pragma unroll
                for (int t = 1; t < kMaxWinMark; ++t) {
                    const int rr = r + side * t * dr, cc = col + side * t * dc;
                    const bool in = t < win_mark && rr >= 0 && rr < B && cc >= 0 && cc < B;
                    const int cl = in ? rr * B + cc : 0;                       // 0 .. A-1 < 64 * kBBWords
                    on = on && in && ((pick4(a0, a1, a2, a3, cl >> 6) >> (cl & 63)) & 1ull);
                    run += on ? 1 : 0;
                }
            }
            win = win || run >= win_mark;
        }
        out[c] = __ballot(empty && win);
    }
}

__device__ __forceinline__ int popcount4(const uint64_t (&m)[kBBWords]) {
    return __popcll(m[0]) + __popcll(m[1]) + __popcll(m[2]) + __popcll(m[3]);
}

struct TacticsParams {
    const int32_t* moves;   // [n][stride]
    const int32_t* nmoves;  // [n]
    int n, stride, B, A, win_mark;
    // outputs, any may be null
    uint8_t* mine; uint8_t* theirs;                 // [n][A]   (k_win_cells)
    int32_t* status; int32_t* turn; int32_t* err;   // [n]      (err: both kernels)
    uint8_t* flags;                                 // [n][A]   (k_audit_games)
    int32_t* counts;                                // [n][8]
};

// the winning cells of the side to move and of its opponent in the position of id i
template <int NCH>
__global__ __launch_bounds__(64 * kPosPerWG) void k_win_cells(TacticsParams q) {
    const int i = blockIdx.x * kPosPerWG + __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
    if (i >= q.n) return;
    const int lane = lane_id();
    const int nm = __builtin_amdgcn_readfirstlane(q.nmoves[i]);
    PosR s;
    int end_ply;
    const int err = replay_moves(s, q.moves + static_cast<size_t>(i) * q.stride, nm, q.A, q.B, q.win_mark, end_ply);
    const bool ok = err == PE_OK;
    const int status = ok ? check_win_board(s.bb[0], s.bb[1], q.B, q.win_mark) : 0;
    const bool open = ok && status == 0;          // a terminal position has no winning cells, for anyone
    const int turn = ok ? (nm & 1) : 0;
    uint64_t mine[kBBWords], theirs[kBBWords];
    winning_cells<NCH>(s, turn, q.B, q.A, q.win_mark, mine);
    winning_cells<NCH>(s, turn ^ 1, q.B, q.A, q.win_mark, theirs);
    if (lane == 0) {
        if (q.status) q.status[i] = status;
        if (q.turn) q.turn[i] = turn;
        if (q.err) q.err[i] = err;
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int cell = lane + 64 * c;
        if (cell >= q.A) continue;
        if (q.mine) q.mine[static_cast<size_t>(i) * q.A + cell] = static_cast<uint8_t>(open && ((mine[c] >> lane) & 1ull));
        if (q.theirs) q.theirs[static_cast<size_t>(i) * q.A + cell] = static_cast<uint8_t>(open && ((theirs[c] >> lane) & 1ull));
    }
}

// the tactical audit of game record i: one flag byte per ply and eight counters
template <int NCH>
__global__ __launch_bounds__(64 * kPosPerWG) void k_audit_games(TacticsParams q) {
    const int i = blockIdx.x * kPosPerWG + __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
    if (i >= q.n) return;
    const int lane = lane_id();
    const int nm = __builtin_amdgcn_readfirstlane(q.nmoves[i]);
    const int32_t* mv = q.moves + static_cast<size_t>(i) * q.stride;
    PosR s;
    pos_clear(s);
    int err = (nm < 0 || nm > q.A) ? PE_LENGTH : PE_OK;
    int end_ply = -1;
    int fl[kBBWords] = {0, 0, 0, 0};   // lane l of fl[c]: the flag byte of ply l + 64 c
    int n_win = 0, n_missed = 0, n_single = 0, n_unblocked = 0, n_lost = 0;
    for (int base = 0; err == PE_OK && base < nm; base += 64) {
        const int t_l = base + lane;
        const int m_l = t_l < nm ? mv[t_l] : 0;
        const int cnt = nm - base < 64 ? nm - base : 64;
        for (int j = 0; j < cnt; ++j) {
            const int m = read_lane(m_l, j);
            if (m < 0 || m >= q.A) { err = PE_RANGE; break; }
            if (pos_occupied(s, m)) { err = PE_OCCUPIED; break; }
            if (end_ply < 0) {             // the position before this move is not terminal: audit the move
                const int t = base + j;
                uint64_t mine[kBBWords], theirs[kBBWords];
                winning_cells<NCH>(s, t & 1, q.B, q.A, q.win_mark, mine);
                winning_cells<NCH>(s, (t & 1) ^ 1, q.B, q.A, q.win_mark, theirs);
                const int n_mine = popcount4(mine), n_theirs = popcount4(theirs);
                const bool in_mine = (pick4(mine[0], mine[1], mine[2], mine[3], m >> 6) >> (m & 63)) & 1ull;
                const bool in_theirs = (pick4(theirs[0], theirs[1], theirs[2], theirs[3], m >> 6) >> (m & 63)) & 1ull;
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
            }
            pos_place(s, m);
            if (end_ply < 0 && win_after_move(s, m, q.B, q.win_mark) != 0) end_ply = base + j;
        }
    }
    if (err != PE_OK) pos_clear(s);
    const bool ok = err == PE_OK;
    const int status = ok ? check_win_board(s.bb[0], s.bb[1], q.B, q.win_mark) : 0;
    if (lane == 0) {
        if (q.err) q.err[i] = err;
        if (q.counts) {
            int32_t* cn = q.counts + static_cast<size_t>(i) * 8;
            cn[0] = ok ? (end_ply >= 0 ? end_ply + 1 : nm) : 0;
            cn[1] = ok ? n_win : 0;
            cn[2] = ok ? n_missed : 0;
            cn[3] = ok ? n_single : 0;
            cn[4] = ok ? n_unblocked : 0;
            cn[5] = ok ? n_lost : 0;
            cn[6] = ok ? end_ply : 0;
            cn[7] = status;
        }
    }
    if (q.flags) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int t = lane + 64 * c;
            if (t < q.A) q.flags[static_cast<size_t>(i) * q.A + t] = static_cast<uint8_t>(ok ? fl[c] : 0);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// forced wins by continuous fours (VCF). No reference counterpart; the definition is utils.forced_win, which asks
// utils.check_win (utils.py:30-59) and nothing else -- see ao_positions_forced_wins in omok_hip.h for the text.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kFwMaxDepth = 16;            // ao_positions_forced_wins: max_depth 1..16
constexpr int kFwMaxNodes = 65536;         //                           max_nodes 1..65536
constexpr int kFwLine = 2 * kFwMaxDepth;   // a line has at most 2 * 16 - 1 stones; the last slot holds its length
enum : int32_t { FW_NONE = 0, FW_WIN = 1, FW_UNKNOWN = 2 };

// one level of the search stack = one attacker node and the four being tried there
struct FwLevel {
    uint64_t cand[kBBWords];   // candidates not tried yet
    uint64_t rep[kBBWords];    // forced replies to the four on `c` not tried yet
    int32_t c, b;              // the attacker's stone and the defender's reply on the board below this level's child
    int32_t b0;                // min(replies): the reply the line follows
    int32_t pad_;
};
struct FwWave {
    FwLevel lv[kFwMaxDepth];               // 16 x 80 B
    int16_t line[kFwMaxDepth][kFwLine];    // line[L]: the line from the node of level L on, [kFwLine - 1] = its length; 1 KB
};

__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(v));
    const unsigned hi = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(v >> 32));
    return lo | (static_cast<uint64_t>(hi) << 32);
}

// a stone of `colour` on `cell` comes or goes (wave-uniform cell; selects, no dynamically indexed access: see pick4)
__device__ __forceinline__ void pos_toggle(PosR& s, int colour, int cell) {
    const int w = cell >> 6;
    const uint64_t bit = 1ull << (cell & 63);
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int i = 0; i < kBBWords; ++i) s.bb[c][i] ^= (c == colour && i == w) ? bit : 0ull;
}

// lowest set cell of a 256-cell mask that is not empty, and the mask without it
__device__ __forceinline__ int pop_lowest(uint64_t (&m)[kBBWords]) {
    int cell = -1;
#pragma unroll
    for (int i = 0; i < kBBWords; ++i) {
        const bool here = cell < 0 && m[i] != 0ull;
        cell = here ? 64 * i + __ffsll(static_cast<long long>(m[i])) - 1 : cell;
        m[i] = here ? m[i] & (m[i] - 1ull) : m[i];
    }
    return cell;
}
__device__ __forceinline__ int lowest_cell(const uint64_t (&m)[kBBWords]) {
    uint64_t t[kBBWords] = {m[0], m[1], m[2], m[3]};
    return pop_lowest(t);
}
__device__ __forceinline__ void mask_add(uint64_t (&m)[kBBWords], int cell) {
#pragma unroll
    for (int i = 0; i < kBBWords; ++i) m[i] |= (i == (cell >> 6)) ? 1ull << (cell & 63) : 0ull;
}

// The empty cells on which a stone of `colour` makes a four: afterwards the colour has a winning cell that goes through the
// new stone (wave-uniform; all 64 lanes call). Lane = cell, NCH passes. Some win_mark-window through the cell holds
// win_mark - 2 stones of the colour, the cell, no stone of the other colour and nothing off the board -- so exactly one more
// empty cell, which then wins. Where the colour has NO winning cell before the stone this is "winning_cells after the stone
// is not empty": a winning cell e after the stone on c lies with c on one line of >= win_mark; were they win_mark or more
// apart on it, the win_mark-window from e towards c would hold e and stones only, and e would have won before. Probed cells
// are checked by row and column like winning_cells'.
template <int NCH>
__device__ __forceinline__ void four_cells(const PosR& s, int colour, int B, int A, int win_mark, uint64_t (&out)[kBBWords]) {
    const int lane = lane_id();
    const uint64_t mk = 0ull - static_cast<uint64_t>(colour & 1);
    const uint64_t a0 = (s.bb[0][0] & ~mk) | (s.bb[1][0] & mk), a1 = (s.bb[0][1] & ~mk) | (s.bb[1][1] & mk);
    const uint64_t a2 = (s.bb[0][2] & ~mk) | (s.bb[1][2] & mk), a3 = (s.bb[0][3] & ~mk) | (s.bb[1][3] & mk);
    const uint64_t d0 = (s.bb[1][0] & ~mk) | (s.bb[0][0] & mk), d1 = (s.bb[1][1] & ~mk) | (s.bb[0][1] & mk);
    const uint64_t d2 = (s.bb[1][2] & ~mk) | (s.bb[0][2] & mk), d3 = (s.bb[1][3] & ~mk) | (s.bb[0][3] & mk);
    constexpr int R = kMaxWinMark - 1;     // offsets -R..R along a line, bit t + R of the two masks below
    const unsigned wm = (1u << win_mark) - 1u;
#pragma unroll
    for (int c = 0; c < kBBWords; ++c) {
        if (c >= NCH) { out[c] = 0ull; continue; }
        const int cell = lane + 64 * c;
        const bool empty = cell < A && !(((s.bb[0][c] | s.bb[1][c]) >> lane) & 1ull);
        const int r = cell / B, col = cell % B;
        bool four = false;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const int dr = (d == 0) ? 0 : 1;
            const int dc = (d == 0) ? 1 : (d == 1) ? 0 : (d == 2) ? 1 : -1;
            unsigned own = 0u, shut = 0u;  // the colour's stones / cells no line of the colour can use
#pragma unroll
            for (int t = -R; t <= R; ++t) {
                if (t == 0) continue;
                const int rr = r + t * dr, cc = col + t * dc;
                const bool in = rr >= 0 && rr < B && cc >= 0 && cc < B;
                const int cl = in ? rr * B + cc : 0;                           // 0 .. A-1 < 64 * kBBWords
                const bool mine = in && ((pick4(a0, a1, a2, a3, cl >> 6) >> (cl & 63)) & 1ull);
                const bool his = in && ((pick4(d0, d1, d2, d3, cl >> 6) >> (cl & 63)) & 1ull);
                own |= mine ? 1u << (t + R) : 0u;
                shut |= (!in || his) ? 1u << (t + R) : 0u;
            }
#pragma unroll
            for (int st = 0; st < kMaxWinMark; ++st) {                         // the window of offsets -st .. -st + win_mark - 1
                const unsigned w = wm << (R - st);
                const bool ok = st < win_mark && (shut & w) == 0u && __popc(own & w) == win_mark - 2;
                four = four || ok;
            }
        }
        out[c] = __ballot(empty && four);
    }
}

struct ForcedParams {
    const int32_t* moves;   // [n][stride]
    const int32_t* nmoves;  // [n]
    int n, stride, B, A, win_mark, max_depth, max_nodes, line_stride;
    // outputs, any may be null
    int32_t* result; int32_t* depth; int32_t* move; int32_t* line_len; int32_t* nodes;   // [n]
    int32_t* status; int32_t* turn; int32_t* err;                                        // [n]
    uint8_t* mask;          // [n][A]
    int16_t* line;          // [n][line_stride], line_stride = 2 max_depth - 1
};

// what a search leaves behind (the principal line stays in the wave's FwWave: line[0], its length in the last slot)
struct FwResult {
    int result, depth, nodes;
    uint64_t won[kBBWords];    // the root's collection: every first move that wins within depth
};

// utils.forced_win of the position `s` for the attacker `a`: iterative deepening over a depth-first search that the wave
// walks as ONE thread of control -- every value that steers it is wave-uniform (ballots, counters, words read back from the
// wave's own LDS stack), the 64 lanes only share the work inside winning_cells / four_cells / check_win_board. No
// recursion: the states below are the call and return points of wins_within / four of the definition. The board is one
// PosR; stones are toggled on the way down and up, `s` is afterwards what it was. `stones`: the stones on the board (two
// more per level: a full board is terminal), `status`: check_win of `s`. Nothing depends on whose turn the stone count
// says it is: the attacker moves first, whoever it is (all 64 lanes call, with wave-uniform arguments).
template <int NCH>
__device__ __forceinline__ void fw_search(PosR& s, int a, int stones, int status, FwWave& W, int B_in, int A, int win_mark, bool run,
                                          int max_depth, int max_nodes, FwResult& r) {
    const int lane = lane_id();
    r.result = FW_NONE;
    r.depth = 0;
    r.nodes = 0;
#pragma unroll
    for (int w = 0; w < kBBWords; ++w) r.won[w] = 0ull;
    enum { ENTER, NEXT_C, NEXT_B, RETURN };

    for (int D = 1; run && r.result == FW_NONE && D <= max_depth; ++D) {
        int L = 0, state = ENTER;
        bool yes = false;                  // what the node that RETURNs answers
        for (;;) {
            // The lanes' geometry inside winning_cells / four_cells (the cells a lane probes, and whether they are on the
            // board) depends on B alone. Hoisted out of the search it would have to live in registers throughout -- some
            // 300 VGPRs at four mask words, spilling to scratch; behind a B the compiler cannot see through it is worked
            // out again at each call.
            int B = B_in;
            asm volatile("" : "+s"(B));
            if (state == ENTER) {          // wins_within(P, D - L); the node's level is L <= D - 1 <= 15
                if (r.nodes >= max_nodes) { r.result = FW_UNKNOWN; break; }
                r.nodes += 1;
                yes = false;
                state = RETURN;
                // below the root a position cannot hold a line (the attacker's stone was no winning cell, the defender
                // had none), it can only be full
                const bool terminal = L == 0 ? status != 0 : stones + 2 * L >= A;
                if (!terminal) {
                    uint64_t mine[kBBWords], theirs[kBBWords];
                    winning_cells<NCH>(s, a, B, A, win_mark, mine);
                    winning_cells<NCH>(s, a ^ 1, B, A, win_mark, theirs);
                    const int n_theirs = popcount4(theirs);
                    if (popcount4(mine) > 0) {
                        yes = true;
                        if (lane == 0) {
                            W.line[L][0] = static_cast<int16_t>(lowest_cell(mine));
                            W.line[L][kFwLine - 1] = 1;
                        }
                        if (L == 0) {
#pragma unroll
                            for (int w = 0; w < kBBWords; ++w) r.won[w] = mine[w];
                        }
                    } else if (D - L > 1 && n_theirs < 2) {
                        uint64_t cand[kBBWords];
                        four_cells<NCH>(s, a, B, A, win_mark, cand);
                        if (lane == 0) {
#pragma unroll
                            for (int w = 0; w < kBBWords; ++w) W.lv[L].cand[w] = n_theirs ? cand[w] & theirs[w] : cand[w];
                        }
                        state = NEXT_C;
                    }
                }
                wsync();
            } else if (state == NEXT_C) {  // the next candidate of level L, or the end of its loop
                uint64_t cand[kBBWords];
#pragma unroll
                for (int w = 0; w < kBBWords; ++w) cand[w] = uniform64(W.lv[L].cand[w]);
                const int c = pop_lowest(cand);
                if (c < 0) {               // (the root's answer is `won`)
                    yes = false;
                    state = RETURN;
                    continue;
                }
                // four(P, c, D - L): the defender has no winning cell after it -- before it he had at most one, and then c is
                // that cell -- so the four stands or falls with its forced replies
                pos_toggle(s, a, c);
                uint64_t rep[kBBWords];
                winning_cells<NCH>(s, a, B, A, win_mark, rep);
                wsync();                   // the reads of cand above are done before lane 0 overwrites it
                if (lane == 0) {
#pragma unroll
                    for (int w = 0; w < kBBWords; ++w) { W.lv[L].cand[w] = cand[w]; W.lv[L].rep[w] = rep[w]; }
                    W.lv[L].c = c;
                    W.lv[L].b0 = lowest_cell(rep);
                }
                wsync();
                if (popcount4(rep) == 0) pos_toggle(s, a, c);     // (four_cells says this cannot happen)
                else state = NEXT_B;
            } else if (state == NEXT_B) {  // the next forced reply to the four of level L, or the four has held
                uint64_t rep[kBBWords];
#pragma unroll
                for (int w = 0; w < kBBWords; ++w) rep[w] = uniform64(W.lv[L].rep[w]);
                const int c = __builtin_amdgcn_readfirstlane(W.lv[L].c);
                const int b = pop_lowest(rep);
                if (b < 0) {               // every reply loses: c succeeds
                    pos_toggle(s, a, c);
                    if (L == 0) {          // the root collects and goes on
                        mask_add(r.won, c);
                        state = NEXT_C;
                    } else {
                        yes = true;
                        state = RETURN;
                    }
                    continue;
                }
                wsync();
                if (lane == 0) {
#pragma unroll
                    for (int w = 0; w < kBBWords; ++w) W.lv[L].rep[w] = rep[w];
                    W.lv[L].b = b;
                }
                wsync();
                pos_toggle(s, a ^ 1, b);
                L += 1;
                state = ENTER;
            } else {                       // RETURN: the node of level L answers `yes` to the four of level L - 1
                if (L == 0) break;
                L -= 1;
                const int c = __builtin_amdgcn_readfirstlane(W.lv[L].c);
                const int b = __builtin_amdgcn_readfirstlane(W.lv[L].b);
                const int b0 = __builtin_amdgcn_readfirstlane(W.lv[L].b0);
                pos_toggle(s, a ^ 1, b);
                if (yes) {
                    // the line follows the first reply; the root keeps the line of its first success (min(moves))
                    if (b == b0 && (L > 0 || popcount4(r.won) == 0)) {
                        const int len = __builtin_amdgcn_readfirstlane(static_cast<int>(W.line[L + 1][kFwLine - 1]));   // <= 2 (D - L - 1) - 1
                        const int16_t v = lane < len ? W.line[L + 1][lane] : static_cast<int16_t>(0);
                        wsync();
                        if (lane < len) W.line[L][lane + 2] = v;               // lane + 2 <= len + 1 <= 2 (D - L) - 2 <= 30
                        if (lane == 0) {
                            W.line[L][0] = static_cast<int16_t>(c);
                            W.line[L][1] = static_cast<int16_t>(b);
                            W.line[L][kFwLine - 1] = static_cast<int16_t>(len + 2);
                        }
                        wsync();
                    }
                    state = NEXT_B;
                } else {
                    pos_toggle(s, a, c);
                    state = NEXT_C;
                }
            }
        }
        if (r.result == FW_NONE && popcount4(r.won) > 0) {
            r.result = FW_WIN;
            r.depth = D;
        }
    }
}

// utils.forced_win of the position of id i, for its side to move
template <int NCH>
__global__ __launch_bounds__(64 * kPosPerWG) void k_forced_wins(ForcedParams q) {
    __shared__ FwWave s_wave[kPosPerWG];
    const int wv = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
    const int i = blockIdx.x * kPosPerWG + wv;
    if (i >= q.n) return;
    FwWave& W = s_wave[wv];
    const int lane = lane_id();
    const int nm = __builtin_amdgcn_readfirstlane(q.nmoves[i]);
    PosR s;
    int end_ply;
    const int err = replay_moves(s, q.moves + static_cast<size_t>(i) * q.stride, nm, q.A, q.B, q.win_mark, end_ply);
    const bool ok = err == PE_OK;
    const int status = ok ? check_win_board(s.bb[0], s.bb[1], q.B, q.win_mark) : 0;
    const int a = ok ? (nm & 1) : 0;       // the attacker

    FwResult r;
    fw_search<NCH>(s, a, nm, status, W, q.B, q.A, q.win_mark, ok, q.max_depth, q.max_nodes, r);
    const int result = r.result, depth = r.depth, nodes = r.nodes;
    const uint64_t (&won)[kBBWords] = r.won;
    wsync();
    const bool win = result == FW_WIN;
    const int len = win ? __builtin_amdgcn_readfirstlane(static_cast<int>(W.line[0][kFwLine - 1])) : 0;
    if (lane == 0) {
        if (q.result) q.result[i] = result;
        if (q.depth) q.depth[i] = depth;
        if (q.move) q.move[i] = win ? lowest_cell(won) : -1;
        if (q.line_len) q.line_len[i] = len;
        if (q.nodes) q.nodes[i] = nodes;
        if (q.status) q.status[i] = status;
        if (q.turn) q.turn[i] = a;
        if (q.err) q.err[i] = err;
    }
    if (q.mask) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int cell = lane + 64 * c;
            if (cell < q.A) q.mask[static_cast<size_t>(i) * q.A + cell] = static_cast<uint8_t>(win && ((won[c] >> lane) & 1ull));
        }
    }
    if (q.line && lane < q.line_stride)    // line_stride = 2 max_depth - 1 <= 31 < 64; len <= 2 depth - 1 <= line_stride
        q.line[static_cast<size_t>(i) * q.line_stride + lane] = lane < len ? W.line[0][lane] : static_cast<int16_t>(-1);
}

// ---------------------------------------------------------------------------------------------------------------------
// which replies hold against a forced win (VCF defence). No reference counterpart; the definition is
// utils.forced_defences: A + 1 searches of utils.forced_win per position, which asks utils.check_win (utils.py:30-59) and
// nothing else -- see ao_positions_forced_defences in omok_hip.h for the text.
// ---------------------------------------------------------------------------------------------------------------------
enum : int { FD_NONE = 0, FD_SAFE = 1, FD_LOSES = 2, FD_UNKNOWN = 3 };

struct DefenceParams {
    const int32_t* moves;   // [n][stride]
    const int32_t* nmoves;  // [n]
    int n, stride, B, A, win_mark, max_depth, max_nodes;
    // k_forced_defences -> k_defence_rows: one word per pair, [n][A + 1]; 0 for a pair without a search, else
    // (1 + result) | depth << 2 | nodes << 8 (depth <= 16, nodes <= 65536: 25 bits)
    uint32_t* pair;
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
template <int NCH>
__global__ __launch_bounds__(64 * kPosPerWG) void k_forced_defences(DefenceParams q) {
    __shared__ FwWave s_wave[kPosPerWG];
    const int wv = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
    const int i = blockIdx.x, j = blockIdx.y * kPosPerWG + wv;     // grid: n x ceil((A + 1) / kPosPerWG)
    if (j > q.A) return;
    const size_t pr = static_cast<size_t>(i) * (q.A + 1) + j;
    const bool pass = j == q.A;
    FwWave& W = s_wave[wv];
    const int lane = lane_id();
    const int nm = __builtin_amdgcn_readfirstlane(q.nmoves[i]);
    PosR s;
    int end_ply;
    const int err = replay_moves(s, q.moves + static_cast<size_t>(i) * q.stride, nm, q.A, q.B, q.win_mark, end_ply);
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
    if (lane == 0)
        q.pair[pr] = searched ? static_cast<uint32_t>(1 + r.result) | static_cast<uint32_t>(r.depth) << 2 | static_cast<uint32_t>(r.nodes) << 8 : 0u;
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
    const int i = blockIdx.x * kPosPerWG + __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
    if (i >= q.n) return;
    const int lane = lane_id();
    const uint32_t* pair = q.pair + static_cast<size_t>(i) * (q.A + 1);
    const uint32_t pw = pair[q.A];         // the pass
    int n_empty = 0, n_safe = 0, n_loses = 0, n_unknown = 0;
    int nodes_l = lane == 0 ? static_cast<int>(pw >> 8) : 0;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int cell = lane + 64 * c;
        const uint32_t w = cell < q.A ? pair[cell] : 0u;
        const int rep = static_cast<int>(w & 3u);
        n_empty += __popcll(__ballot(rep != FD_NONE));
        n_safe += __popcll(__ballot(rep == FD_SAFE));
        n_loses += __popcll(__ballot(rep == FD_LOSES));
        n_unknown += __popcll(__ballot(rep == FD_UNKNOWN));
        nodes_l += static_cast<int>(w >> 8);
        if (cell < q.A) {
            if (q.reply) q.reply[static_cast<size_t>(i) * q.A + cell] = static_cast<uint8_t>(rep);
            if (q.depth) q.depth[static_cast<size_t>(i) * q.A + cell] = static_cast<uint8_t>((w >> 2) & 31u);
        }
    }
    const int nodes = wave_sum_i(nodes_l);   // <= 226 * 65536
    if (lane == 0) {
        if (q.threat) q.threat[i] = pw ? static_cast<int>(pw & 3u) - 1 : 0;
        if (q.threat_depth) q.threat_depth[i] = static_cast<int>((pw >> 2) & 31u);
        if (q.nodes) q.nodes[i] = nodes;
        if (q.counts) {
            int32_t* cn = q.counts + static_cast<size_t>(i) * 4;
            cn[0] = n_empty; cn[1] = n_safe; cn[2] = n_loses; cn[3] = n_unknown;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// the solver on an engine's own roots (ao_root_tactics, engine.hip). No reference counterpart; the definition is
// utils.root_tactics, which goes through utils.forced_win alone. The positions are the engine's TreeParams::rootpos, read
// on the device: no move list is staged. Three launches: the mover's search and the opponent's search after a pass
// (k_root_tactics_a), every reply's search for the games that stand under a proven threat with no win of their own
// (k_root_tactics_b), and one wavefront per game that puts the words together (k_root_tactics_rows). A search's word is
// the one of k_forced_defences: 0 without a search, else (1 + result) | depth << 2 | nodes << 8.
// ---------------------------------------------------------------------------------------------------------------------
struct RootTacticsParams {
    const Pos* rootpos;     // [G]
    const uint8_t* active;  // [G] or null
    int G, B, A, win_mark, max_depth, max_nodes;
    RootTacticsBufs b;
};

__device__ __forceinline__ uint32_t fw_word(const FwResult& r) {
    return static_cast<uint32_t>(1 + r.result) | static_cast<uint32_t>(r.depth) << 2 | static_cast<uint32_t>(r.nodes) << 8;
}
__device__ __forceinline__ int pos_stones(const PosR& s) { return popcount4(s.bb[0]) + popcount4(s.bb[1]); }

// Two wavefronts per game: role 0 searches for the mover, role 1 for the opponent as if the mover had passed. Stones =
// popcount of the bitboards, the mover from the ply's parity (what replay_moves gives for the game's id), status =
// check_win_board. An inactive or a terminal game is not searched: both words 0.
template <int NCH>
__global__ __launch_bounds__(64 * kPosPerWG) void k_root_tactics_a(RootTacticsParams q) {
    __shared__ FwWave s_wave[kPosPerWG];
    const int wv = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
    const int k = blockIdx.x * kPosPerWG + wv;
    const int g = k >> 1, role = k & 1;
    if (g >= q.G) return;
    FwWave& W = s_wave[wv];
    const int lane = lane_id();
    const bool on = !q.active || __builtin_amdgcn_readfirstlane(static_cast<int>(q.active[g])) != 0;
    PosR s = pos_load(q.rootpos + g);
    const int stones = __builtin_amdgcn_readfirstlane(pos_stones(s));
    const int m = __builtin_amdgcn_readfirstlane(s.ply) & 1;
    const int status = check_win_board(s.bb[0], s.bb[1], q.B, q.win_mark);
    const bool searched = on && status == 0;

    FwResult r;
    fw_search<NCH>(s, m ^ role, stones, status, W, q.B, q.A, q.win_mark, searched, q.max_depth, q.max_nodes, r);
    if (lane == 0) {
        q.b.stage[2 * static_cast<size_t>(g) + role] = searched ? fw_word(r) : 0u;
        if (role == 0) {
#pragma unroll
            for (int w = 0; w < kBBWords; ++w) q.b.won[static_cast<size_t>(g) * kBBWords + w] = r.won[w];
        }
    }
}

// stage A left "the opponent's forced win is proven, the mover has none" for game g
__device__ __forceinline__ bool root_under_threat(const RootTacticsParams& q, int g) {
    const uint32_t own = q.b.stage[2 * static_cast<size_t>(g)], thr = q.b.stage[2 * static_cast<size_t>(g) + 1];
    return own != 0u && static_cast<int>(own & 3u) - 1 != FW_WIN && static_cast<int>(thr & 3u) - 1 == FW_WIN;
}

// One wavefront per (game, reply cell) pair, grid G x ceil(A / kPosPerWG). A wave returns at once unless its game is under a
// proven threat; otherwise it does what k_forced_defences does for a reply pair: the mover's stone on the cell, the
// opponent's search on what stands then. An occupied cell writes 0.
template <int NCH>
__global__ __launch_bounds__(64 * kPosPerWG) void k_root_tactics_b(RootTacticsParams q) {
    __shared__ FwWave s_wave[kPosPerWG];
    const int wv = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
    const int g = blockIdx.x, j = blockIdx.y * kPosPerWG + wv;
    if (j >= q.A) return;
    if (!__builtin_amdgcn_readfirstlane(static_cast<int>(root_under_threat(q, g)))) return;
    FwWave& W = s_wave[wv];
    const int lane = lane_id();
    PosR s = pos_load(q.rootpos + g);
    const int stones = __builtin_amdgcn_readfirstlane(pos_stones(s));
    const int m = __builtin_amdgcn_readfirstlane(s.ply) & 1;
    const bool searched = !pos_occupied(s, j);
    if (searched) pos_toggle(s, m, j);
    const int status = check_win_board(s.bb[0], s.bb[1], q.B, q.win_mark);

    FwResult r;
    fw_search<NCH>(s, m ^ 1, stones + 1, status, W, q.B, q.A, q.win_mark, searched, q.max_depth, q.max_nodes, r);
    if (lane == 0) q.b.pair[static_cast<size_t>(g) * q.A + j] = searched ? fw_word(r) : 0u;
}

// One wavefront per game: verdict, depth, nodes, unknown, allowed [A] and the bar of the move out of the words of its
// searches, by utils.root_tactics' rules. `nodes` and `unknown` count the searches the host definition runs: the mover's;
// the opponent's unless the mover wins; the replies' under a proven threat. Ballots and integer sums only: no result
// depends on an order. The bar (in: the caller's barred actions, or zeros) becomes the caller's plus the empty cells the
// verdict does not allow -- unless that left the game nothing to search: then it stays the caller's.
template <int NCH>
__global__ __launch_bounds__(64 * kPosPerWG) void k_root_tactics_rows(RootTacticsParams q) {
    const int g = blockIdx.x * kPosPerWG + __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
    if (g >= q.G) return;
    const int lane = lane_id();
    const uint32_t own = q.b.stage[2 * static_cast<size_t>(g)], thr = q.b.stage[2 * static_cast<size_t>(g) + 1];
    const PosR s = pos_load(q.rootpos + g);
    const bool searched = own != 0u;
    const int own_res = static_cast<int>(own & 3u) - 1, thr_res = static_cast<int>(thr & 3u) - 1;
    const bool win = searched && own_res == FW_WIN;
    const bool threat = searched && !win && thr_res == FW_WIN;
    int verdict = win ? RT_WIN : RT_NONE;
    int depth = win ? static_cast<int>((own >> 2) & 31u) : 0;
    int unknown = (searched && own_res == FW_UNKNOWN) ? 1 : 0;
    if (searched && !win && thr_res == FW_UNKNOWN) unknown |= 2;
    int nodes_l = 0;
    if (lane == 0 && searched) nodes_l = static_cast<int>(own >> 8) + (win ? 0 : static_cast<int>(thr >> 8));
    uint64_t em[NCH], ok[NCH];             // the empty cells; the cells the verdict allows
    int n_ok = 0;
    bool ran_out = false;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int cell = lane + 64 * c;
        const bool empty = cell < q.A && !(((s.bb[0][c] | s.bb[1][c]) >> lane) & 1ull);
        em[c] = __ballot(empty);
        const uint32_t w = (threat && cell < q.A) ? q.b.pair[static_cast<size_t>(g) * q.A + cell] : 0u;
        const int rep = static_cast<int>(w & 3u);
        nodes_l += static_cast<int>(w >> 8);
        ran_out = ran_out || __ballot(rep == FD_UNKNOWN) != 0ull;
        const bool mine = (q.b.won[static_cast<size_t>(g) * kBBWords + c] >> lane) & 1ull;
        ok[c] = __ballot(threat ? (rep == FD_SAFE || rep == FD_UNKNOWN) : win ? mine : empty);
        n_ok += __popcll(ok[c]);
    }
    if (threat) {
        verdict = n_ok > 0 ? RT_DEFEND : RT_LOST;
        depth = static_cast<int>((thr >> 2) & 31u);
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
    uint64_t cb[NCH], nb[NCH];             // the caller's bar; the bar with the verdict's on top
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int cell = lane + 64 * c;
        const uint64_t allow = open ? (searched ? em[c] : 0ull) : ok[c];
        if (q.b.allowed && cell < q.A) q.b.allowed[static_cast<size_t>(g) * q.A + cell] = static_cast<uint8_t>((allow >> lane) & 1ull);
        cb[c] = q.b.bar ? uniform64(q.b.bar[static_cast<size_t>(g) * kBBWords + c]) & em[c] : 0ull;
        nb[c] = searched ? (cb[c] | (em[c] & ~allow)) : cb[c];
        n_left += __popcll(em[c] & ~nb[c]);
    }
    if (q.b.bar && lane == 0) {
        uint64_t* out = q.b.bar + static_cast<size_t>(g) * kBBWords;
#pragma unroll
        for (int c = 0; c < NCH; ++c) out[c] = n_left > 0 ? nb[c] : cb[c];
#pragma unroll
        for (int c = NCH; c < kBBWords; ++c) out[c] = 0ull;
    }
}

void launch_root_tactics(const TreeParams& p, const uint8_t* active, int max_depth, int max_nodes, const RootTacticsBufs& b, hipStream_t s) {
    RootTacticsParams q{};
    q.rootpos = p.rootpos; q.active = active;
    q.G = p.G; q.B = p.B; q.A = p.A; q.win_mark = p.win_mark; q.max_depth = max_depth; q.max_nodes = max_nodes;
    q.b = b;
    const dim3 block(64 * kPosPerWG);
    const dim3 grid_a(static_cast<unsigned>((2 * p.G + kPosPerWG - 1) / kPosPerWG));
    const dim3 grid_b(static_cast<unsigned>(p.G), static_cast<unsigned>((p.A + kPosPerWG - 1) / kPosPerWG));
    const dim3 grid_r(static_cast<unsigned>((p.G + kPosPerWG - 1) / kPosPerWG));
    AO_DISPATCH_NCH(nch_of_cells(p.A), hipLaunchKernelGGL(k_root_tactics_a<NCH>, grid_a, block, 0, s, q);
                    hipLaunchKernelGGL(k_root_tactics_b<NCH>, grid_b, block, 0, s, q);
                    hipLaunchKernelGGL(k_root_tactics_rows<NCH>, grid_r, block, 0, s, q));
}

}  // namespace ao

struct ao_positions : ao::HandleBase {
    int B = 0, A = 0, C = 0, win_mark = 0, cap = 0, device = 0;
    hipStream_t stream = nullptr;
    ao::DevPool pool;
    int32_t* d_moves = nullptr;    // [cap][A]
    int32_t* d_n = nullptr;        // [cap]
    int32_t* d_i32 = nullptr;      // [4][cap]: status, end_ply, turn, err
    int8_t* d_board = nullptr;     // [cap][A] (boards in for check_win, boards out for from_moves)
    uint8_t* d_legal = nullptr;    // [cap][A]
    ao::DevBuf<float> d_planes{&pool};     // [cap][C][A]   -- the three below: allocated by the first ao_positions_evaluate
    ao::DevBuf<float> d_policy{&pool};     // [cap][A]
    ao::DevBuf<float> d_value{&pool};      // [cap]
    ao::DevBuf<int32_t> d_counts{&pool};   // [cap][8]      -- allocated by the first ao_positions_audit
    ao::DevBuf<int32_t> d_forced{&pool};   // [5][cap]: result, depth, move, line_len, nodes -- these two: by the first ao_positions_forced_wins
    ao::DevBuf<int16_t> d_line{&pool};     // [cap][2 * 16 - 1]
    ao::DevBuf<uint32_t> d_pair{&pool};    // [cap][A + 1]  -- the three below: allocated by the first ao_positions_forced_defences
    ao::DevBuf<int32_t> d_defence{&pool};  // [3][cap]: threat, threat_depth, nodes, then counts [cap][4]
    ao::DevBuf<uint8_t> d_depth{&pool};    // [cap][A]
    std::vector<int32_t> h_moves, h_n;
};

namespace {

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

int launch_from_moves(ao_positions* p, int m, bool status, bool end_ply, bool turn, bool board, bool legal, float* planes, bool err,
                      bool bad_as_empty) {
    ao::PositionsParams q{};
    q.moves = p->d_moves; q.nmoves = p->d_n;
    q.n = m; q.stride = p->A; q.B = p->B; q.A = p->A; q.C = p->C; q.win_mark = p->win_mark;
    q.bad_as_empty = bad_as_empty ? 1 : 0;
    q.status = status ? p->d_i32 : nullptr;
    q.end_ply = end_ply ? p->d_i32 + p->cap : nullptr;
    q.turn = turn ? p->d_i32 + 2 * static_cast<size_t>(p->cap) : nullptr;
    q.err = err ? p->d_i32 + 3 * static_cast<size_t>(p->cap) : nullptr;
    q.board = board ? p->d_board : nullptr;
    q.legal = legal ? p->d_legal : nullptr;
    q.planes = planes;
    const dim3 grid(static_cast<unsigned>((m + ao::kPosPerWG - 1) / ao::kPosPerWG)), block(64 * ao::kPosPerWG);
    AO_DISPATCH_NCH(ao::nch_of_cells(p->A), hipLaunchKernelGGL(ao::k_positions_from_moves<NCH>, grid, block, 0, p->stream, q));
    AO_HIP(p, hipGetLastError());
    return 0;
}

// k_win_cells (audit false) or k_audit_games on the m staged ids; the kernel's outputs land in the staging buffers
int launch_tactics(ao_positions* p, int m, bool audit) {
    ao::TacticsParams q{};
    q.moves = p->d_moves; q.nmoves = p->d_n;
    q.n = m; q.stride = p->A; q.B = p->B; q.A = p->A; q.win_mark = p->win_mark;
    q.err = p->d_i32 + 3 * static_cast<size_t>(p->cap);
    if (audit) {
        q.flags = p->d_legal;
        q.counts = p->d_counts.p;
    } else {
        q.mine = reinterpret_cast<uint8_t*>(p->d_board);
        q.theirs = p->d_legal;
        q.status = p->d_i32;
        q.turn = p->d_i32 + 2 * static_cast<size_t>(p->cap);
    }
    const dim3 grid(static_cast<unsigned>((m + ao::kPosPerWG - 1) / ao::kPosPerWG)), block(64 * ao::kPosPerWG);
    AO_DISPATCH_NCH(ao::nch_of_cells(p->A),
                    if (audit) hipLaunchKernelGGL(ao::k_audit_games<NCH>, grid, block, 0, p->stream, q);
                    else hipLaunchKernelGGL(ao::k_win_cells<NCH>, grid, block, 0, p->stream, q));
    AO_HIP(p, hipGetLastError());
    return 0;
}

// k_forced_wins on the m staged ids; the outputs land in d_forced, d_line, d_board (the mask) and d_i32
int launch_forced(ao_positions* p, int m, int max_depth, int max_nodes) {
    ao::ForcedParams q{};
    const size_t cap = static_cast<size_t>(p->cap);
    q.moves = p->d_moves; q.nmoves = p->d_n;
    q.n = m; q.stride = p->A; q.B = p->B; q.A = p->A; q.win_mark = p->win_mark;
    q.max_depth = max_depth; q.max_nodes = max_nodes; q.line_stride = 2 * max_depth - 1;
    int32_t* forced = p->d_forced.p;
    q.result = forced; q.depth = forced + cap; q.move = forced + 2 * cap;
    q.line_len = forced + 3 * cap; q.nodes = forced + 4 * cap;
    q.status = p->d_i32; q.turn = p->d_i32 + 2 * cap; q.err = p->d_i32 + 3 * cap;
    q.mask = reinterpret_cast<uint8_t*>(p->d_board);
    q.line = p->d_line.p;
    const dim3 grid(static_cast<unsigned>((m + ao::kPosPerWG - 1) / ao::kPosPerWG)), block(64 * ao::kPosPerWG);
    AO_DISPATCH_NCH(ao::nch_of_cells(p->A), hipLaunchKernelGGL(ao::k_forced_wins<NCH>, grid, block, 0, p->stream, q));
    AO_HIP(p, hipGetLastError());
    return 0;
}

// k_forced_defences on the (A + 1) pairs of each of the m staged ids, then k_defence_rows on the ids; the outputs land in
// d_defence, d_board (threat_moves), d_legal (reply), d_depth and d_i32
int launch_defences(ao_positions* p, int m, int max_depth, int max_nodes) {
    ao::DefenceParams q{};
    const size_t cap = static_cast<size_t>(p->cap);
    q.moves = p->d_moves; q.nmoves = p->d_n;
    q.n = m; q.stride = p->A; q.B = p->B; q.A = p->A; q.win_mark = p->win_mark;
    q.max_depth = max_depth; q.max_nodes = max_nodes;
    q.pair = p->d_pair.p;
    q.threat_moves = reinterpret_cast<uint8_t*>(p->d_board);
    q.status = p->d_i32; q.turn = p->d_i32 + 2 * cap; q.err = p->d_i32 + 3 * cap;
    int32_t* def = p->d_defence.p;
    q.threat = def; q.threat_depth = def + cap; q.nodes = def + 2 * cap; q.counts = def + 3 * cap;
    q.reply = p->d_legal; q.depth = p->d_depth.p;
    const dim3 pair_grid(static_cast<unsigned>(m), static_cast<unsigned>((p->A + 1 + ao::kPosPerWG - 1) / ao::kPosPerWG));
    const dim3 grid(static_cast<unsigned>((m + ao::kPosPerWG - 1) / ao::kPosPerWG)), block(64 * ao::kPosPerWG);
    AO_DISPATCH_NCH(ao::nch_of_cells(p->A), hipLaunchKernelGGL(ao::k_forced_defences<NCH>, pair_grid, block, 0, p->stream, q);
                    hipLaunchKernelGGL(ao::k_defence_rows<NCH>, grid, block, 0, p->stream, q));
    AO_HIP(p, hipGetLastError());
    return 0;
}

template <class T>
int download(ao_positions* p, T* host, const T* dev, size_t count) {
    if (host) AO_HIP(p, hipMemcpyAsync(host, dev, sizeof(T) * count, hipMemcpyDeviceToHost, p->stream));
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
           p->pool.alloc(p, &p->d_board, cap * A) || p->pool.alloc(p, &p->d_legal, cap * A);
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

int ao_positions_check_win(ao_positions* p, const int8_t* host_boards, int32_t n, int32_t* host_win) {
    if (n < 0) return p->fail("ao_positions_check_win: negative position count");
    if (n == 0) return 0;
    if (!host_boards || !host_win) return p->fail("ao_positions_check_win: null buffer");
    AO_HIP(p, hipSetDevice(p->device));
    const size_t A = static_cast<size_t>(p->A);
    for (int64_t first = 0; first < n; first += p->cap) {
        const int m = static_cast<int>(std::min<int64_t>(p->cap, n - first));
        AO_HIP(p, hipMemcpyAsync(p->d_board, host_boards + first * A, static_cast<size_t>(m) * A, hipMemcpyHostToDevice, p->stream));
        hipLaunchKernelGGL(ao::k_check_win_boards, dim3(static_cast<unsigned>((m + ao::kPosPerWG - 1) / ao::kPosPerWG)),
                           dim3(64 * ao::kPosPerWG), 0, p->stream, p->d_board, m, p->B, p->win_mark, p->d_i32);
        AO_HIP(p, hipGetLastError());
        AO_HIP(p, hipMemcpyAsync(host_win + first, p->d_i32, sizeof(int32_t) * m, hipMemcpyDeviceToHost, p->stream));
        AO_HIP(p, hipStreamSynchronize(p->stream));   // the staging buffers are reused by the next chunk
    }
    return 0;
}

int ao_positions_from_moves(ao_positions* p, const int32_t* host_moves, int32_t stride, const int32_t* host_n, int32_t n,
                            int32_t* host_status, int32_t* host_end_ply, int32_t* host_turn, int8_t* host_board,
                            uint8_t* host_legal, float* dev_planes_nchw, int32_t* host_err) {
    if (n < 0 || stride < 0) return p->fail("ao_positions_from_moves: negative position count or stride");
    if (n == 0) return 0;
    if (!host_n || (!host_moves && stride > 0)) return p->fail("ao_positions_from_moves: null move buffer");
    AO_HIP(p, hipSetDevice(p->device));
    // the caller's plane buffer may be memory that work queued on another stream still uses (a caching allocator hands such out)
    if (dev_planes_nchw) AO_HIP(p, hipDeviceSynchronize());
    const size_t A = static_cast<size_t>(p->A), cap = static_cast<size_t>(p->cap);
    for (int64_t first = 0; first < n; first += p->cap) {
        const int m = static_cast<int>(std::min<int64_t>(p->cap, n - first));
        if (stage_moves(p, "ao_positions_from_moves", host_moves, stride, host_n, first, m)) return 1;
        float* planes = dev_planes_nchw ? dev_planes_nchw + static_cast<size_t>(first) * p->C * A : nullptr;
        if (launch_from_moves(p, m, host_status, host_end_ply, host_turn, host_board, host_legal, planes, host_err, false)) return 1;
        if (download(p, host_status ? host_status + first : nullptr, p->d_i32, m) ||
            download(p, host_end_ply ? host_end_ply + first : nullptr, p->d_i32 + cap, m) ||
            download(p, host_turn ? host_turn + first : nullptr, p->d_i32 + 2 * cap, m) ||
            download(p, host_err ? host_err + first : nullptr, p->d_i32 + 3 * cap, m) ||
            download(p, host_board ? host_board + first * A : nullptr, p->d_board, m * A) ||
            download(p, host_legal ? host_legal + first * A : nullptr, p->d_legal, m * A))
            return 1;
        AO_HIP(p, hipStreamSynchronize(p->stream));   // the planes are complete for any stream; the staging buffers are reused
    }
    return 0;
}

int ao_positions_win_cells(ao_positions* p, const int32_t* host_moves, int32_t stride, const int32_t* host_n, int32_t n,
                           uint8_t* host_mine, uint8_t* host_theirs, int32_t* host_status, int32_t* host_turn, int32_t* host_err) {
    if (n < 0 || stride < 0) return p->fail("ao_positions_win_cells: negative position count or stride");
    if (n == 0) return 0;
    if (!host_n || (!host_moves && stride > 0)) return p->fail("ao_positions_win_cells: null move buffer");
    AO_HIP(p, hipSetDevice(p->device));
    const size_t A = static_cast<size_t>(p->A), cap = static_cast<size_t>(p->cap);
    for (int64_t first = 0; first < n; first += p->cap) {
        const int m = static_cast<int>(std::min<int64_t>(p->cap, n - first));
        if (stage_moves(p, "ao_positions_win_cells", host_moves, stride, host_n, first, m)) return 1;
        if (launch_tactics(p, m, false)) return 1;
        if (download(p, host_mine ? host_mine + first * A : nullptr, reinterpret_cast<const uint8_t*>(p->d_board), m * A) ||
            download(p, host_theirs ? host_theirs + first * A : nullptr, p->d_legal, m * A) ||
            download(p, host_status ? host_status + first : nullptr, p->d_i32, m) ||
            download(p, host_turn ? host_turn + first : nullptr, p->d_i32 + 2 * cap, m) ||
            download(p, host_err ? host_err + first : nullptr, p->d_i32 + 3 * cap, m))
            return 1;
        AO_HIP(p, hipStreamSynchronize(p->stream));   // the staging buffers are reused by the next chunk
    }
    return 0;
}

int ao_positions_audit(ao_positions* p, const int32_t* host_moves, int32_t stride, const int32_t* host_n, int32_t n,
                       uint8_t* host_flags, int32_t* host_counts, int32_t* host_err) {
    if (n < 0 || stride < 0) return p->fail("ao_positions_audit: negative record count or stride");
    if (n == 0) return 0;
    if (!host_n || (!host_moves && stride > 0)) return p->fail("ao_positions_audit: null move buffer");
    AO_HIP(p, hipSetDevice(p->device));
    const size_t A = static_cast<size_t>(p->A), cap = static_cast<size_t>(p->cap);
    if (p->d_counts.reserve(p, cap * 8)) return 1;
    for (int64_t first = 0; first < n; first += p->cap) {
        const int m = static_cast<int>(std::min<int64_t>(p->cap, n - first));
        if (stage_moves(p, "ao_positions_audit", host_moves, stride, host_n, first, m)) return 1;
        if (launch_tactics(p, m, true)) return 1;
        if (download(p, host_flags ? host_flags + first * A : nullptr, p->d_legal, m * A) ||
            download(p, host_counts ? host_counts + first * 8 : nullptr, p->d_counts.p, static_cast<size_t>(m) * 8) ||
            download(p, host_err ? host_err + first : nullptr, p->d_i32 + 3 * cap, m))
            return 1;
        AO_HIP(p, hipStreamSynchronize(p->stream));   // the staging buffers are reused by the next chunk
    }
    return 0;
}

int ao_positions_forced_wins(ao_positions* p, const int32_t* host_moves, int32_t stride, const int32_t* host_n, int32_t n,
                             int32_t max_depth, int32_t max_nodes, int32_t* host_result, int32_t* host_depth, int32_t* host_move,
                             uint8_t* host_moves_mask, int16_t* host_line, int32_t* host_line_len, int32_t* host_nodes,
                             int32_t* host_status, int32_t* host_turn, int32_t* host_err) {
    if (n < 0 || stride < 0) return p->fail("ao_positions_forced_wins: negative position count or stride");
    if (max_depth < 1 || max_depth > ao::kFwMaxDepth) return p->fail("ao_positions_forced_wins: max_depth must be in 1..16");
    if (max_nodes < 1 || max_nodes > ao::kFwMaxNodes) return p->fail("ao_positions_forced_wins: max_nodes must be in 1..65536");
    if (n == 0) return 0;
    if (!host_n || (!host_moves && stride > 0)) return p->fail("ao_positions_forced_wins: null move buffer");
    AO_HIP(p, hipSetDevice(p->device));
    const size_t A = static_cast<size_t>(p->A), cap = static_cast<size_t>(p->cap);
    const size_t lw = static_cast<size_t>(2 * max_depth - 1);
    if (p->d_forced.reserve(p, 5 * cap) || p->d_line.reserve(p, cap * (2 * ao::kFwMaxDepth - 1))) return 1;
    for (int64_t first = 0; first < n; first += p->cap) {
        const int m = static_cast<int>(std::min<int64_t>(p->cap, n - first));
        if (stage_moves(p, "ao_positions_forced_wins", host_moves, stride, host_n, first, m)) return 1;
        if (launch_forced(p, m, max_depth, max_nodes)) return 1;
        if (download(p, host_result ? host_result + first : nullptr, p->d_forced.p, m) ||
            download(p, host_depth ? host_depth + first : nullptr, p->d_forced.p + cap, m) ||
            download(p, host_move ? host_move + first : nullptr, p->d_forced.p + 2 * cap, m) ||
            download(p, host_line_len ? host_line_len + first : nullptr, p->d_forced.p + 3 * cap, m) ||
            download(p, host_nodes ? host_nodes + first : nullptr, p->d_forced.p + 4 * cap, m) ||
            download(p, host_moves_mask ? host_moves_mask + first * A : nullptr, reinterpret_cast<const uint8_t*>(p->d_board), m * A) ||
            download(p, host_line ? host_line + first * lw : nullptr, p->d_line.p, m * lw) ||
            download(p, host_status ? host_status + first : nullptr, p->d_i32, m) ||
            download(p, host_turn ? host_turn + first : nullptr, p->d_i32 + 2 * cap, m) ||
            download(p, host_err ? host_err + first : nullptr, p->d_i32 + 3 * cap, m))
            return 1;
        AO_HIP(p, hipStreamSynchronize(p->stream));   // the staging buffers are reused by the next chunk
    }
    return 0;
}

int ao_positions_forced_defences(ao_positions* p, const int32_t* host_moves, int32_t stride, const int32_t* host_n, int32_t n,
                                 int32_t max_depth, int32_t max_nodes, int32_t* host_threat, int32_t* host_threat_depth,
                                 uint8_t* host_threat_moves, uint8_t* host_reply, uint8_t* host_depth, int32_t* host_counts,
                                 int32_t* host_nodes, int32_t* host_status, int32_t* host_turn, int32_t* host_err) {
    if (n < 0 || stride < 0) return p->fail("ao_positions_forced_defences: negative position count or stride");
    if (max_depth < 1 || max_depth > ao::kFwMaxDepth) return p->fail("ao_positions_forced_defences: max_depth must be in 1..16");
    if (max_nodes < 1 || max_nodes > ao::kFwMaxNodes) return p->fail("ao_positions_forced_defences: max_nodes must be in 1..65536");
    if (n == 0) return 0;
    if (!host_n || (!host_moves && stride > 0)) return p->fail("ao_positions_forced_defences: null move buffer");
    const size_t A = static_cast<size_t>(p->A), cap = static_cast<size_t>(p->cap);
    AO_HIP(p, hipSetDevice(p->device));
    if (p->d_pair.reserve(p, cap * (A + 1)) || p->d_defence.reserve(p, 7 * cap) || p->d_depth.reserve(p, cap * A)) return 1;
    for (int64_t first = 0; first < n; first += p->cap) {
        const int m = static_cast<int>(std::min<int64_t>(p->cap, n - first));
        if (stage_moves(p, "ao_positions_forced_defences", host_moves, stride, host_n, first, m)) return 1;
        if (launch_defences(p, m, max_depth, max_nodes)) return 1;
        if (download(p, host_threat ? host_threat + first : nullptr, p->d_defence.p, m) ||
            download(p, host_threat_depth ? host_threat_depth + first : nullptr, p->d_defence.p + cap, m) ||
            download(p, host_nodes ? host_nodes + first : nullptr, p->d_defence.p + 2 * cap, m) ||
            download(p, host_counts ? host_counts + first * 4 : nullptr, p->d_defence.p + 3 * cap, static_cast<size_t>(m) * 4) ||
            download(p, host_threat_moves ? host_threat_moves + first * A : nullptr, reinterpret_cast<const uint8_t*>(p->d_board), m * A) ||
            download(p, host_reply ? host_reply + first * A : nullptr, p->d_legal, m * A) ||
            download(p, host_depth ? host_depth + first * A : nullptr, p->d_depth.p, m * A) ||
            download(p, host_status ? host_status + first : nullptr, p->d_i32, m) ||
            download(p, host_turn ? host_turn + first : nullptr, p->d_i32 + 2 * cap, m) ||
            download(p, host_err ? host_err + first : nullptr, p->d_i32 + 3 * cap, m))
            return 1;
        AO_HIP(p, hipStreamSynchronize(p->stream));   // the staging buffers are reused by the next chunk
    }
    return 0;
}

int ao_positions_evaluate(ao_positions* p, ao_net* net, const int32_t* host_moves, int32_t stride, const int32_t* host_n,
                          int32_t n, float* host_policy, float* host_value, int32_t* host_status, int32_t* host_err) {
    if (n < 0 || stride < 0) return p->fail("ao_positions_evaluate: negative position count or stride");
    if (!net) return p->fail("ao_positions_evaluate: null network");
    std::string why;
    if (ao::net_check(net, p->B, p->C, p->device, &why)) return p->fail("ao_positions_evaluate: " + why);
    if (n == 0) return 0;
    if (!host_n || (!host_moves && stride > 0) || !host_policy || !host_value) return p->fail("ao_positions_evaluate: null buffer");
    AO_HIP(p, hipSetDevice(p->device));
    AO_HIP(p, hipDeviceSynchronize());   // the network's workspace may still serve a forward queued on another stream
    const size_t A = static_cast<size_t>(p->A), cap = static_cast<size_t>(p->cap);
    if (p->d_planes.reserve(p, cap * p->C * A) || p->d_policy.reserve(p, cap * A) || p->d_value.reserve(p, cap)) return 1;
    std::vector<int32_t> err_chunk;
    for (int64_t first = 0; first < n; first += p->cap) {
        const int m = static_cast<int>(std::min<int64_t>(p->cap, n - first));
        if (stage_moves(p, "ao_positions_evaluate", host_moves, stride, host_n, first, m)) return 1;
        // a position with an error is fed as the empty board: its row must not disturb the rest of the chunk
        if (launch_from_moves(p, m, true, false, false, false, false, p->d_planes.p, true, true)) return 1;
        if (ao_net_forward(net, p->d_planes.p, m, p->d_policy.p, p->d_value.p, p->stream))
            return p->fail(std::string("ao_positions_evaluate: ") + ao_net_last_error(net));
        err_chunk.resize(static_cast<size_t>(m));
        if (download(p, host_policy + first * A, p->d_policy.p, m * A) || download(p, host_value + first, p->d_value.p, m) ||
            download(p, host_status ? host_status + first : nullptr, p->d_i32, m) || download(p, err_chunk.data(), p->d_i32 + 3 * cap, m))
            return 1;
        AO_HIP(p, hipStreamSynchronize(p->stream));
        for (int k = 0; k < m; ++k) {
            if (err_chunk[static_cast<size_t>(k)] == 0) continue;
            std::fill_n(host_policy + (first + k) * A, A, 0.f);
            host_value[first + k] = 0.f;
        }
        if (host_err) std::memcpy(host_err + first, err_chunk.data(), sizeof(int32_t) * m);
    }
    return 0;
}

}  // extern "C"
