// launchers.hpp -- the host entry points that one translation unit defines and another calls: the launchers of the tree and step
// kernels, the few of the proof, root-tactics and leaf-tactics kernels that a second file uses, and the network's internal
// interface. Included by the callers AND by every file that defines one of them, so that a changed signature is a compile error
// where it changes and never a second overload. A launcher whose only caller stands in its own file (roll.hip, tree_readout.hip,
// tree_snapshot.hip, ao_root_tactics') is static there and has no entry here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/omok_hip.h"
#include "engine_types.hpp"

namespace ao {
// tree_kernels.hip
void launch_select(const TreeParams& p, hipStream_t s);
void launch_expand_backup(const TreeParams& p, hipStream_t s);
void launch_expand_select(const TreeParams& p, hipStream_t s);
void launch_begin_move(const TreeParams& p, hipStream_t s);
void launch_order(const TreeParams& p, int32_t* order, hipStream_t s);
void launch_end_move(const TreeParams& p, hipStream_t s);
// launch_play, launch_walk, launch_reroot: non-zero = refused by walk_lds_bytes (tree_walk.hpp), nothing launched
int launch_play(const TreeParams& p, hipStream_t s);
int launch_walk(const TreeParams& p, int count, const int32_t* games, const int32_t* extra, int stride, const int32_t* m,
                const int32_t* prev_known, int32_t* status_out, hipStream_t s);
int launch_reroot(const TreeParams& p, int count, const int32_t* games, hipStream_t s);   // k_reroot for the listed games (null: all p.G)
bool reroot_fits(const TreeParams& p);   // false: launch_reroot / launch_play / launch_walk would refuse (the queue of a p.cap arena does not fit the LDS)
void launch_reset(const TreeParams& p, const uint8_t* mask, hipStream_t s);
void launch_settle(const TreeParams& p, const uint8_t* mask, int stop_now, int leaf_open, uint8_t* settled, int32_t* out, hipStream_t s);
void launch_eval_log(const int32_t* games, int n, const int32_t* row_of_game, const float* policy, const float* value, int A,
                     float* out, const int32_t* sims_done, const int32_t* leaf_status, int what, hipStream_t s);
// tree_proofs.hip, both for ao_end_move under ao_set_proof_moves as well: exact minimax over what the roots reach (ws: int32 [G][cap]
// workspace; non-zero = refused, as launch_play), and utils.proof_pi on TreeParams::out_pi in place
int launch_tree_proofs(const TreeParams& p, const uint8_t* mask, int32_t* ws, int max_len, int32_t* root_out, int8_t* child_status,
                       int16_t* child_plies, int32_t* line, int32_t* line_len, hipStream_t s);
void launch_proof_pi(const TreeParams& p, const int8_t* child_status, const int16_t* child_plies, int32_t* verdict, hipStream_t s);
// root_tactics.hip: the solver's three kernels on n compact position rows, every buffer of b indexed by the row (a batch of the
// rolling search, roll.hip)
void launch_root_tactics_rows(const Pos* rows, int n, int B, int A, int win_mark, int max_depth, int max_nodes, const RootTacticsBufs& b,
                              hipStream_t s);
// leaf_tactics.hip: the forced-win solver on the leaves of the simulation under way (k_leaf_tactics), and +1 into the value row
// of every proven leaf (k_leaf_values; row_of_game null: row g)
void launch_leaf_tactics(const LeafTacticsParams& q, hipStream_t s);
void launch_leaf_values(const uint8_t* proven, const int32_t* row_of_game, float* value, int G, hipStream_t s);
// step_kernels.hip
void launch_step_board(const TreeParams& p, const StepNet& f, int rows, const int32_t* game_of_row, hipStream_t s);
// net.hip
int net_forward_il(ao_net* n, const float* in_il, int boards, float* policy, float* value,
                   hipStream_t s, int in_kind, int parts, const unsigned* live, unsigned row_cap);
int net_step_params(ao_net* n, int boards, float* policy, float* value, StepNet* out);
void net_fp16_fallback_begin(ao_net* n);
int net_fp16_fallback_end(ao_net* n);
void net_plan(const ao_net* n, int boards, int* group, int* nchq, int* kind);
int net_check(const ao_net* n, int board, int inplanes, int device, std::string* why);
}  // namespace ao
