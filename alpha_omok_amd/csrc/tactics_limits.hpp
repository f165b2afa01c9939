// tactics_limits.hpp -- the limits of the forced-win solver (fw_search, tactics_device.hpp) and their one check, host code: every
// entry point that takes max_depth / max_nodes (ao_positions_forced_wins, ao_positions_forced_defences, ao_root_tactics) asks here.
#pragma once
#include <string>

namespace ao {

constexpr int kFwMaxDepth = 16;            // ao_positions_forced_wins: max_depth 1..16
constexpr int kFwMaxNodes = 65536;         //                           max_nodes 1..65536

// the text an entry point `who` fails with for search limits outside 1..kFwMaxDepth / 1..kFwMaxNodes, empty if they are fine
inline std::string fw_limits_error(const char* who, int max_depth, int max_nodes) {
    if (max_depth < 1 || max_depth > kFwMaxDepth) return std::string(who) + ": max_depth must be in 1.." + std::to_string(kFwMaxDepth);
    if (max_nodes < 1 || max_nodes > kFwMaxNodes) return std::string(who) + ": max_nodes must be in 1.." + std::to_string(kFwMaxNodes);
    return std::string();
}

}  // namespace ao
