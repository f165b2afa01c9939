// tactics_limits.hpp -- the limits of the forced-win solver (fw_search, tactics_device.hpp) and their one check, host code: every
// entry point that takes max_depth / max_nodes (ao_positions_forced_wins, ao_positions_forced_defences, ao_root_tactics) asks here.
#pragma once
#include <string>

namespace ao {

constexpr int kFwMaxDepth = 16;            // ao_positions_forced_wins: max_depth 1..16
constexpr int kFwMaxNodes = 65536;         //                           max_nodes 1..65536

// ao_set_leaf_tactics: the solver runs once per simulation of every game, so its budget is far smaller -- the cap bounds one
// launch at about 1024 x the per-node time of DESIGN.md section 4
constexpr int kLeafMaxNodes = 1024;        // ao_set_leaf_tactics:      max_nodes 1..1024

// the text an entry point `who` fails with for search limits outside 1..kFwMaxDepth / 1..node_cap, empty if they are fine
inline std::string fw_limits_error(const char* who, int max_depth, int max_nodes, int node_cap = kFwMaxNodes) {
    if (max_depth < 1 || max_depth > kFwMaxDepth) return std::string(who) + ": max_depth must be in 1.." + std::to_string(kFwMaxDepth);
    if (max_nodes < 1 || max_nodes > node_cap) return std::string(who) + ": max_nodes must be in 1.." + std::to_string(node_cap);
    return std::string();
}

}  // namespace ao
