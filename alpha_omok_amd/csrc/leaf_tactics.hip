// leaf_tactics.hip -- the forced-win solver on the leaves a search is about to expand (ao_set_leaf_tactics, engine.hip). No
// reference counterpart; the definition is utils.leaf_tactics_value, which goes through utils.forced_win alone: the value of a
// leaf whose mover has a proven forced win by continuous fours is +1 (the value is the leaf mover's own, agents.py:223-239),
// every other leaf keeps what the network said. The positions are the engine's TreeParams::leaf_pos, read on the device. Two
// launches between a network launch and the tree launch behind it: the search (k_leaf_tactics: one byte per game) and the
// override (k_leaf_values: one float per proven leaf, in the row expand_backup_game reads). No tree kernel and no network kernel
// knows of either. The search is the position batch's and the root tactics' (tactics_device.hpp).
#include "host_handle.hpp"
#include "launchers.hpp"
#include "tactics_device.hpp"

namespace ao {

// One wavefront per game. A wave returns unless its game is active and its leaf is one that the tree launch behind it expands
// (LS_EXPAND, LS_EXPAND_ROOT): a waiting leaf is searched in the launch that gives it its row, paused descents, idle games and
// terminal leaves never. Role 0 of k_root_tactics_a on the leaf: the opponent passes, the mover searches; stones = popcount of
// the bitboards, the mover from the ply's parity. Everything that steers the wave is wave-uniform. Lane 0 writes the game's byte
// (1: proven; 0 for every game that was not searched, so that no byte of an earlier launch is read) and adds to the game's four
// counters -- searched, proven, out of nodes, nodes; one wave owns a game's row: plain integer adds.
template <int NCH>
__global__ __launch_bounds__(64 * kPosPerWG) void k_leaf_tactics(LeafTacticsParams q) {
    __shared__ FwWave s_wave[kPosPerWG];
    const int wv = wg_wave();
    const int g = wave_item();
    if (g >= q.G) return;
    const int on = !q.active || __builtin_amdgcn_readfirstlane(static_cast<int>(q.active[g])) != 0;
    const int st = __builtin_amdgcn_readfirstlane(q.leaf_status[g]);
    if (!on || (st != LS_EXPAND && st != LS_EXPAND_ROOT)) {
        if (lane_id() == 0) q.proven[g] = 0;
        return;
    }
    PosR s = pos_load(q.leaf_pos + g);
    const int stones = __builtin_amdgcn_readfirstlane(pos_stones(s));
    const int m = __builtin_amdgcn_readfirstlane(s.ply) & 1;

    FwResult r;
    int status;
    const uint32_t word = reply_search<NCH>(s, m ^ 1, stones, kPass, true, s_wave[wv], q.B, q.A, q.win_mark, q.max_depth, q.max_nodes, status, r);
    if (lane_id() == 0) {
        const int res = fw_word_result(word);    // -1: the position is over (the selection marks those LS_TERMINAL: not reached)
        q.proven[g] = res == FW_WIN ? 1 : 0;
        if (word != 0u) {
            int32_t* c = q.counts + static_cast<size_t>(g) * 4;
            c[0] += 1;
            c[1] += res == FW_WIN ? 1 : 0;
            c[2] += res == FW_UNKNOWN ? 1 : 0;
            c[3] += fw_word_nodes(word);
        }
    }
}

// One thread per game: the proven leaf's value becomes +1 in the row the tree launch reads (all three row regimes: packed per
// move, handed out per simulation, the step-wise protocol's row g).
__global__ __launch_bounds__(256) void k_leaf_values(const uint8_t* proven, const int32_t* row_of_game, float* value, int G) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G || !proven[g]) return;
    value[row_of_game ? row_of_game[g] : g] = 1.0f;
}

void launch_leaf_tactics(const LeafTacticsParams& q, hipStream_t s) {
    const dim3 block(64 * kPosPerWG);
    const dim3 grid(static_cast<unsigned>((q.G + kPosPerWG - 1) / kPosPerWG));
    AO_DISPATCH_NCH(nch_of_cells(q.A), hipLaunchKernelGGL(k_leaf_tactics<NCH>, grid, block, 0, s, q));
}

void launch_leaf_values(const uint8_t* proven, const int32_t* row_of_game, float* value, int G, hipStream_t s) {
    hipLaunchKernelGGL(k_leaf_values, dim3(static_cast<unsigned>((G + 255) / 256)), dim3(256), 0, s, proven, row_of_game, value, G);
}

}  // namespace ao
