// Drives alpha_omok_amd/csrc/search_schedule.hpp from stdin, one case per line, one answer line per case
// (tests/test_search_schedule_host.py writes the cases and restates the formulas):
//   W rows G cap_rows ask_frac                     -> W row_target sit_idx sit0
//   P sims G sit_idx                               -> P planned_extra_launches
//   C cap_rows S override window_off level_budget n  sum mx bad  (n times)
//                                                  -> C then per round "<launches>:<window_off>", "stop" (the rule ended the
//                                                     loop) or "closed" (the round bound did), then rounds=<rounds looked at>
//   L cap_rows n  want (n times)                   -> L launches rows_live rows_launched waits
//   R harvested upto ring                          -> R first head tail
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "search_schedule.hpp"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind;
        if (!(in >> kind)) continue;
        if (kind == "W") {
            int rows, G, cap;
            std::string frac;   // (hex float: exact)
            in >> rows >> G >> cap >> frac;
            const ao::SitWindow w = ao::sit_window(rows, G, cap, std::stod(frac));
            std::printf("W %u %u %u\n", w.row_target, w.sit_idx, w.sit0);
        } else if (kind == "P") {
            int sims, G;
            unsigned sit_idx;
            in >> sims >> G >> sit_idx;
            std::printf("P %d\n", ao::planned_extra_launches(sims, G, sit_idx));
        } else if (kind == "C") {
            int cap, S, override_, window_off, level_budget, n;
            in >> cap >> S >> override_ >> window_off >> level_budget >> n;
            ao::CatchUp cu(cap, S, override_, window_off != 0);
            std::printf("C");
            bool ended = false;
            for (int k = 0; k < n && !ended; ++k) {
                long long sum;
                int mx, bad;
                in >> sum >> mx >> bad;
                if (!cu.open()) {
                    std::printf(" closed");
                    ended = true;
                    break;
                }
                const int launches = cu.next(sum, mx, bad != 0, level_budget != 0);
                if (launches == 0) {
                    std::printf(" stop");
                    ended = true;
                } else {
                    std::printf(" %d:%d", launches, cu.window_off ? 1 : 0);
                }
            }
            if (!ended && !cu.open()) std::printf(" closed");
            std::printf(" rounds=%d\n", cu.round);
        } else if (kind == "L") {
            int cap, n;
            in >> cap >> n;
            ao::RowLedger led;
            for (int k = 0; k < n; ++k) {
                long long want;
                in >> want;
                led.add(want, cap);
            }
            std::printf("L %lld %lld %lld %lld\n", static_cast<long long>(led.launches), static_cast<long long>(led.rows_live),
                        static_cast<long long>(led.rows_launched), static_cast<long long>(led.waits));
        } else if (kind == "R") {
            long long harvested, upto;
            int ring;
            in >> harvested >> upto >> ring;
            const ao::RingSpans s = ao::ring_spans(harvested, upto, ring);
            std::printf("R %d %d %d\n", s.first, s.head, s.tail);
        } else {
            std::fprintf(stderr, "unknown case: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
