// search_schedule.hpp -- the host arithmetic of the launch schedule (engine.hip). For ao_search's MoveSearch: how wide the
// sit-out window of an over-subscribed move is, how many launches it plans beyond its simulations, when the catch-up rounds go
// on and when they give up. For the LaunchLoop under both MoveSearch and the rolling search: which words of the row-counter ring
// a harvest reads and how the harvested counters add up to ao_row_stats. No HIP, no engine: plain C++17, tested on the host
// (tests/host/search_schedule_main.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

namespace ao {

// Over-subscription (`rows` active games of G on cap_rows < rows rows per simulation). Every launch a window of the game indices
// sits out, sized so that the games that do descend ask for about cap_rows rows -- a share ask_frac of them does (the rest ends
// at terminal leaves), measured over the previous move of the engine, less 2.5 standard deviations of that binomial; the window
// moves on by its own length per launch (tree_device.hpp, select_game).
// row_target: rows the controller steers a launch's demand to; sit_idx: the window at the move's average demand (the host's
// estimate); sit0: the window the move STARTS with
struct SitWindow { unsigned row_target, sit_idx, sit0; };
inline SitWindow sit_window(int rows, int G, int cap_rows, double ask_frac) {
    SitWindow w;
    const double f = std::min(1.0, std::max(0.5, ask_frac));
    const double slack = 2.5 * std::sqrt(static_cast<double>(cap_rows) * (1.0 - f)) + 4.0;
    w.row_target = static_cast<unsigned>(std::max(1.0, cap_rows - slack));
    const double askers = std::min<double>(rows, std::floor(w.row_target / f));
    w.sit_idx = static_cast<unsigned>(std::lround((rows - askers) * G / static_cast<double>(rows)));
    if (w.sit_idx >= static_cast<unsigned>(G)) w.sit_idx = static_cast<unsigned>(G) - 1u;
    // the move STARTS with the window that is safe for any demand -- as many games descend as there are rows -- and the
    // controller opens it within a handful of launches: the first descents of a move ask for more rows than its average
    // (measured: 4741 - 4957 asked of 4096 at the average's window, ~2000 leaves per move sent waiting), and a leaf that
    // waits costs its game a launch at the END of the move, when the batch is nearly empty
    const double askers0 = std::min<double>(rows, w.row_target);
    w.sit0 = static_cast<unsigned>(std::lround((rows - askers0) * G / static_cast<double>(rows)));
    if (w.sit0 >= static_cast<unsigned>(G)) w.sit0 = static_cast<unsigned>(G) - 1u;
    return w;
}

// a game sits out sit_idx / G of the launches: that many more launches before anyone can be done (a few short: the catch-up
// rounds find out exactly). <= 0: none.
inline int planned_extra_launches(int sims, int G, unsigned sit_idx) {
    return static_cast<int>(std::ceil(static_cast<double>(sims) * G / (G - sit_idx))) - sims - 8;
}

// The catch-up rounds of a move whose games may be short of their simulations after the nominal number of launches. The
// counters say by how much; max(largest deficit, all deficits / rows per launch) is a lower bound of the launches still needed
// -- run them, look again. A round without progress is not a stall yet -- a leaf that waited takes its row in one launch and is
// expanded by the next, and a game may have sat out the only launch of the round -- so the sit-out window is switched OFF first
// (nobody sits out, and every round runs two launches at least); two more rounds without progress after that are a real stall.
struct CatchUp {
    int cap_rows;
    int max_rounds;        // 4 (S + 2), or the override (AO_CATCHUP_ROUNDS) if that is >= 0
    bool window_off;       // nobody sits out any more
    int round = 0, stalled = 0;
    int64_t last_sum = -1;
    CatchUp(int cap_rows_, int S, int rounds_override, bool window_off_)
        : cap_rows(cap_rows_), max_rounds(rounds_override >= 0 ? rounds_override : 4 * (S + 2)), window_off(window_off_) {}
    bool open() const { return round < max_rounds; }   // may another round look at the counters?
    // One round, from the deficits target - done of the active games that are short: their sum, the largest, whether any game
    // has an error word set, whether descents run under a level budget. Returns the launches to run, 0 = the loop ends.
    int next(int64_t sum, int mx, bool bad, bool level_budget) {
        ++round;
        if (mx == 0 || bad) return 0;                   // done / a per-game error (reported by ao_end_move)
        if (sum == last_sum && !level_budget) {         // (with a level budget a round may pass without a finished simulation)
            if (!window_off) window_off = true;
            else if (++stalled >= 2) return 0;          // a real stall: ao_end_move names the games
        } else {
            stalled = 0;
        }
        last_sum = sum;
        int extra = static_cast<int>(std::max<int64_t>(mx, (sum + cap_rows - 1) / cap_rows));
        if (window_off) extra = std::max(extra, 2);
        return extra;
    }
};

// ao_row_stats: what the harvested row counters of the selection launches add up to
struct RowLedger {
    int64_t launches = 0, rows_live = 0, rows_launched = 0, waits = 0;
    void add(int64_t want, int cap_rows) {   // one launch whose leaves asked for `want` rows
        rows_live += std::min<int64_t>(want, cap_rows);
        waits += std::max<int64_t>(want - cap_rows, 0);
        rows_launched += cap_rows;
        ++launches;
    }
};

// The row counters live in a ring of `ring` device words: launch i counts in word i % ring. What has to be read to sum up the
// launches [harvested, upto): the words [first, first + head) and, where the range runs past the ring's end, [0, tail) -- at
// most `ring` words (the launch loop harvests wherever the ring wraps, so a range never holds more launches than that).
struct RingSpans { int first, head, tail; };
inline RingSpans ring_spans(int64_t harvested, int64_t upto, int ring) {
    if (upto <= harvested) return {0, 0, 0};
    const int count = static_cast<int>(std::min<int64_t>(upto - harvested, ring)), first = static_cast<int>(harvested % ring);
    const int head = std::min(count, ring - first);
    return {first, head, count - head};
}

}  // namespace ao
