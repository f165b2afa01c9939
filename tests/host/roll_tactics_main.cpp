// Drives the rules of the solver beside the rolling loop (alpha_omok_amd/csrc/roll_schedule.hpp) from stdin, one case per line,
// one answer line per case (tests/test_roll_tactics_host.py writes the cases and restates the rules):
//   S budget verdict solved_sims                          -> S budget of the move
//   T state done target leaf_idle                         -> T 0|1     (state: 0 out of a move, 1 searching, 2 waiting)
//   G event_done age hold blocked                         -> G 0|1     (the batch's games begin their move)
//   K busy_slots slots starts_batch searching pending     -> K 0|1     (the host waits for the oldest batch)
//   N                                                     -> N slots of the ring
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "roll_schedule.hpp"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind;
        if (!(in >> kind)) continue;
        if (kind == "S") {
            int budget, verdict, solved;
            in >> budget >> verdict >> solved;
            std::printf("S %d\n", ao::roll_solved_budget(budget, verdict, solved));
        } else if (kind == "T") {
            int state, done, target, idle;
            in >> state >> done >> target >> idle;
            std::printf("T %d\n", ao::roll_game_turns(state, done, target, idle != 0) ? 1 : 0);
        } else if (kind == "G") {
            int done, age, hold, blocked;
            in >> done >> age >> hold >> blocked;
            std::printf("G %d\n", ao::roll_batch_begins(done != 0, age, hold, blocked != 0) ? 1 : 0);
        } else if (kind == "K") {
            int busy, slots, starts, searching, pending;
            in >> busy >> slots >> starts >> searching >> pending;
            std::printf("K %d\n", ao::roll_must_block(busy, slots, starts != 0, searching, pending) ? 1 : 0);
        } else if (kind == "N") {
            std::printf("N %d\n", ao::kRollBatchSlots);
        } else {
            std::fprintf(stderr, "unknown case: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
