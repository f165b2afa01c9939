// tactics_device.hpp -- what the kernels that ask tactical questions of a position share: the rule status of a whole board, the
// cells that win at once and the cells that make a four, the forced-win search by continuous fours (VCF) with its one-word
// result, and the search after a reply. Included by positions.hip (the positions a caller names: k_win_cells, k_audit_games,
// k_forced_wins, k_forced_defences, k_defence_rows) and root_tactics.hip (an engine's own roots: k_root_tactics_a, _b, _rows);
// the solver's limits are tactics_limits.hpp.
//
// One wavefront (64 lanes) owns one position, kPosPerWG of them per workgroup, nothing shared between them (no LDS but the
// search stack, one FwWave per wave). No reference counterpart beyond utils.check_win (utils.py:30-59 of the reference, see
// the map in positions.hip): utils.forced_win / utils.forced_defences / utils.root_tactics of this package are the host
// definitions. The bitboards, pos_occupied and pick4 are the tree kernels' own (tree_device.hpp).
#pragma once
#include "tactics_limits.hpp"
#include "tree_device.hpp"

namespace ao {

constexpr int kPosPerWG = 4;
constexpr int kMaxWinMark = 5;   // ao_positions_create: win_mark 3..5

constexpr int kFwLine = 2 * kFwMaxDepth;   // a line has at most 2 * 16 - 1 stones; the last slot holds its length
enum : int32_t { FW_NONE = 0, FW_WIN = 1, FW_UNKNOWN = 2 };
enum : int { FD_NONE = 0, FD_SAFE = 1, FD_LOSES = 2, FD_UNKNOWN = 3 };

// the wave's index in its workgroup, and the item (position, game) of a kernel that gives each wave one: both wave-uniform
__device__ __forceinline__ int wg_wave() { return __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6); }
__device__ __forceinline__ int wave_item() { return blockIdx.x * kPosPerWG + wg_wave(); }

// ---------------------------------------------------------------------------------------------------------------------
// 256-cell masks as four 64-cell words, and single stones on a PosR
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int popcount4(const uint64_t (&m)[kBBWords]) {
    return __popcll(m[0]) + __popcll(m[1]) + __popcll(m[2]) + __popcll(m[3]);
}
__device__ __forceinline__ int pos_stones(const PosR& s) { return popcount4(s.bb[0]) + popcount4(s.bb[1]); }

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

// bit `lane` of word c of `mask` -> row[lane + 64 c] of a uint8 [A] row, 0 where `gate` is false; a null row is not written
// (all 64 lanes call; NW >= NCH words)
template <int NCH, int NW>
__device__ __forceinline__ void store_cell_mask(uint8_t* __restrict__ row, int A, const uint64_t (&mask)[NW], bool gate) {
    static_assert(NW >= NCH, "a mask word for every pass");
    if (!row) return;
    const int lane = lane_id();
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int cell = lane + 64 * c;
        if (cell < A) row[cell] = static_cast<uint8_t>(gate && ((mask[c] >> lane) & 1ull));
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// utils.check_win of a whole board
// ---------------------------------------------------------------------------------------------------------------------
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

// ---------------------------------------------------------------------------------------------------------------------
// tactical cells: which empty cells win at once, which make a four. The definition is utils.check_win (utils.py:30-59)
// of the board with one more stone -- see ao_positions_win_cells in omok_hip.h.
// ---------------------------------------------------------------------------------------------------------------------
// the stones of `colour` (0 black / 1 white) and of the other colour, by a mask blend and by value (see win_after_move_by
// and pick4)
struct ColourWords { uint64_t own[kBBWords], other[kBBWords]; };
__device__ __forceinline__ ColourWords colour_words(const PosR& s, int colour) {
    const uint64_t mk = 0ull - static_cast<uint64_t>(colour & 1);
    ColourWords w;
#pragma unroll
    for (int i = 0; i < kBBWords; ++i) {
        w.own[i] = (s.bb[0][i] & ~mk) | (s.bb[1][i] & mk);
        w.other[i] = (s.bb[1][i] & ~mk) | (s.bb[0][i] & mk);
    }
    return w;
}
// (winning_cells / four_cells spell this test out: through the helper the search kernels get another register allocation,
// fewer VGPRs and half as many SGPR spills again, and the root tactics measured 3 % slower)
__device__ __forceinline__ bool has_cell(const uint64_t (&m)[kBBWords], int cell) {
    return (pick4(m[0], m[1], m[2], m[3], cell >> 6) >> (cell & 63)) & 1ull;
}
// the step of line direction d = 0..3: along the row, down the column, the two diagonals
__device__ __forceinline__ void line_step(int d, int& dr, int& dc) {
    dr = (d == 0) ? 0 : 1;
    dc = (d == 0) ? 1 : (d == 1) ? 0 : (d == 2) ? 1 : -1;
}

// The empty cells on which a stone of `colour` (0 black / 1 white) completes a line of win_mark or more, as 64-cell mask
// words (wave-uniform; all 64 lanes call). Lane = cell, NCH passes. In each direction the lane counts the colour's
// contiguous stones on either side of its cell, up to win_mark - 1 a side, every probed cell checked by ROW and COLUMN (a
// run that reaches column B-1 does not go on at column 0 of the next row); 1 + left + right >= win_mark wins, overlines
// included. On a position without a line that is check_win == colour + 1 after the stone: only a line through the new
// stone can be new, and it is the colour's. The ballot of the predicate is the mask word.
template <int NCH>
__device__ __forceinline__ void winning_cells(const PosR& s, int colour, int B, int A, int win_mark, uint64_t (&out)[kBBWords]) {
    const int lane = lane_id();
    const ColourWords w = colour_words(s, colour);
#pragma unroll
    for (int c = 0; c < kBBWords; ++c) {
        if (c >= NCH) { out[c] = 0ull; continue; }
        const int cell = lane + 64 * c;
        const bool empty = cell < A && !(((s.bb[0][c] | s.bb[1][c]) >> lane) & 1ull);
        const int r = cell / B, col = cell % B;
        bool win = false;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            int dr, dc;
            line_step(d, dr, dc);
            int run = 1;
#pragma unroll
            for (int side = -1; side <= 1; side += 2) {
                bool on = empty;
#pragma unroll
                for (int t = 1; t < kMaxWinMark; ++t) {
                    const int rr = r + side * t * dr, cc = col + side * t * dc;
                    const bool in = t < win_mark && rr >= 0 && rr < B && cc >= 0 && cc < B;
                    const int cl = in ? rr * B + cc : 0;                       // 0 .. A-1 < 64 * kBBWords
                    on = on && in && ((pick4(w.own[0], w.own[1], w.own[2], w.own[3], cl >> 6) >> (cl & 63)) & 1ull);
                    run += on ? 1 : 0;
                }
            }
            win = win || run >= win_mark;
        }
        out[c] = __ballot(empty && win);
    }
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
    const ColourWords w = colour_words(s, colour);
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
            int dr, dc;
            line_step(d, dr, dc);
            unsigned own = 0u, shut = 0u;  // the colour's stones / cells no line of the colour can use
#pragma unroll
            for (int t = -R; t <= R; ++t) {
                if (t == 0) continue;
                const int rr = r + t * dr, cc = col + t * dc;
                const bool in = rr >= 0 && rr < B && cc >= 0 && cc < B;
                const int cl = in ? rr * B + cc : 0;                           // 0 .. A-1 < 64 * kBBWords
                const bool mine = in && ((pick4(w.own[0], w.own[1], w.own[2], w.own[3], cl >> 6) >> (cl & 63)) & 1ull);
                const bool his = in && ((pick4(w.other[0], w.other[1], w.other[2], w.other[3], cl >> 6) >> (cl & 63)) & 1ull);
                own |= mine ? 1u << (t + R) : 0u;
                shut |= (!in || his) ? 1u << (t + R) : 0u;
            }
#pragma unroll
            for (int st = 0; st < kMaxWinMark; ++st) {                         // the window of offsets -st .. -st + win_mark - 1
                const unsigned wd = wm << (R - st);
                const bool ok = st < win_mark && (shut & wd) == 0u && __popc(own & wd) == win_mark - 2;
                four = four || ok;
            }
        }
        out[c] = __ballot(empty && four);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// forced wins by continuous fours (VCF). The definition is utils.forced_win, which asks utils.check_win (utils.py:30-59)
// and nothing else -- see ao_positions_forced_wins in omok_hip.h for the text.
// ---------------------------------------------------------------------------------------------------------------------
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

// what a search leaves behind (the principal line stays in the wave's FwWave: line[0], its length in the last slot)
struct FwResult {
    int result, depth, nodes;
    uint64_t won[kBBWords];    // the root's collection: every first move that wins within depth
};

// A search as one word, the form in which the kernels hand searches to each other: 0 = no search, else
// (1 + result) | depth << 2 | nodes << 8 (depth <= 16, nodes <= 65536: 25 bits). The word's low two bits are the FD_* value
// of the reply the search answers: FD_NONE no search, FD_SAFE = 1 + FW_NONE, FD_LOSES = 1 + FW_WIN, FD_UNKNOWN = 1 + FW_UNKNOWN.
__device__ __forceinline__ uint32_t fw_word(const FwResult& r) {
    return static_cast<uint32_t>(1 + r.result) | static_cast<uint32_t>(r.depth) << 2 | static_cast<uint32_t>(r.nodes) << 8;
}
__device__ __forceinline__ int fw_word_reply(uint32_t w) { return static_cast<int>(w & 3u); }              // FD_*
__device__ __forceinline__ int fw_word_result(uint32_t w) { return fw_word_reply(w) - 1; }                  // FW_*, -1 without a search
__device__ __forceinline__ int fw_word_depth(uint32_t w) { return static_cast<int>((w >> 2) & 31u); }
__device__ __forceinline__ int fw_word_nodes(uint32_t w) { return static_cast<int>(w >> 8); }

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

// The opponent's search after the mover's reply, the step both search stages of the root tactics take (k_forced_defences
// keeps the same step written out, for its registers' and its speed's sake: see there): the stone of the
// mover `m` goes on cell j if that is empty (j == kPass: no stone, the mover passes), `status` becomes check_win of what
// stands then -- the root of the search: a stone that makes a line or fills the board leaves a terminal root, which answers
// no at one node per iteration -- and forced_win runs for the opponent. `allowed`: the caller's own condition for searching
// at all. Not searched, whatever the caller allows: a reply on an occupied cell, and a pass in a position that is over.
// `stones`: the stones on the board before the reply. Returns the search's word, 0 where nothing was searched; r.won of the
// search is the caller's to use. The stone stays on `s` (all 64 lanes call, with wave-uniform arguments).
constexpr int kPass = -1;
template <int NCH>
__device__ __forceinline__ uint32_t reply_search(PosR& s, int m, int stones, int j, bool allowed, FwWave& W, int B, int A, int win_mark,
                                                 int max_depth, int max_nodes, int& status, FwResult& r) {
    const bool pass = j == kPass;
    const bool placed = allowed && !pass && !pos_occupied(s, j);
    if (placed) pos_toggle(s, m, j);
    status = check_win_board(s.bb[0], s.bb[1], B, win_mark);
    const bool searched = pass ? allowed && status == 0 : placed;
    fw_search<NCH>(s, m ^ 1, pass ? stones : stones + 1, status, W, B, A, win_mark, searched, max_depth, max_nodes, r);
    return searched ? fw_word(r) : 0u;
}

}  // namespace ao
