// Drives alpha_omok_amd/csrc/roll_schedule.hpp from stdin, one case per line, one answer line per case
// (tests/test_roll_schedule_host.py writes the cases and restates the rules):
//   M ply tau_plies engine_noise S root_status  ns sims (ns times)  nn noise (nn times)     (ns / nn 0: no table)
//                                                  -> M tau budget target gflags draw refuse
//   T in_move done target leaf_idle                -> T 0|1
//   B win draining                                 -> B 0|1
//   R records in_move launches max_launches        -> R 0|1
//   C turn_every early steps                       -> C then one letter per step: L launch, K look, T turn
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "roll_schedule.hpp"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind;
        if (!(in >> kind)) continue;
        if (kind == "M") {
            int ply, tau_plies, engine_noise, S, status, ns, nn;
            in >> ply >> tau_plies >> engine_noise >> S >> status >> ns;
            std::vector<int32_t> sims(ns);
            for (int& v : sims) in >> v;
            in >> nn;
            std::vector<uint8_t> noise(nn);
            for (uint8_t& v : noise) { int x; in >> x; v = static_cast<uint8_t>(x); }
            const ao::RollMove m = ao::roll_next_move(ply, tau_plies, ns ? sims.data() : nullptr, ns, nn ? noise.data() : nullptr, nn,
                                                      engine_noise != 0, S, status);
            std::printf("M %d %d %d %d %d %d\n", m.tau, m.budget, m.target, m.gflags, m.draw, m.refuse);
        } else if (kind == "T") {
            int in_move, done, target, idle;
            in >> in_move >> done >> target >> idle;
            std::printf("T %d\n", ao::roll_turns(in_move != 0, done, target, idle != 0) ? 1 : 0);
        } else if (kind == "B") {
            int win, draining;
            in >> win >> draining;
            std::printf("B %d\n", ao::roll_begins_next(win, draining != 0) ? 1 : 0);
        } else if (kind == "R") {
            int records, in_move;
            long long launches, max_launches;
            in >> records >> in_move >> launches >> max_launches;
            std::printf("R %d\n", ao::roll_run_returns(records, in_move, launches, max_launches) ? 1 : 0);
        } else if (kind == "C") {
            int turn_every, early, steps;
            in >> turn_every >> early >> steps;
            ao::RollCadence cad;
            cad.turn_every = turn_every;
            cad.early = early != 0;
            std::string out;
            for (int k = 0; k < steps; ++k) {
                const ao::RollStep s = cad.next();
                out += s == ao::ROLL_LAUNCH ? 'L' : (s == ao::ROLL_LOOK ? 'K' : 'T');
            }
            std::printf("C %s\n", out.c_str());
        } else {
            std::fprintf(stderr, "unknown case: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
