// move_device.hpp -- what the begin and the end of ONE game's move do on the device, as functions of the game: the bodies of
// k_begin_move, k_end_move and k_play (tree_kernels.hip: every game of the engine, one wave each) and of the rolling search's
// turn (roll.hip: the listed games only, end of move and play in one wave). One copy of the arithmetic and of the order of the
// stream draws, so the two callers cannot differ by a bit. Reference map: tree_kernels.hip.
#pragma once
#include "tree_walk.hpp"

namespace ao {

// k_begin_move for game g: the simulation counter, and the re-noise (renoise: bit 0 of the game's gflags) / the bar of an
// inherited, expanded root (agents.py:93-103). Lane l reads the entries l, l + 64, ... of the game's noise row.
template <int NCH>
__device__ __forceinline__ void begin_move_game(const TreeParams& p, const int g, const bool renoise) {
    const int lane = lane_id();
    if (lane == 0) { p.sims_done[g] = 0; p.leaf_status[g] = LS_IDLE; }   // (no leaf of an aborted move is left waiting for a row)
    const int node = p.root_node[g];
    if ((!renoise && !p.bar) || node < 0) return;
    const size_t slot = node_slot(p, p.cur[g], g, node);
    const int L = nodePos(p, slot)->nchild;
    const uint64_t* bar = p.bar ? p.bar + static_cast<size_t>(g) * kBBWords : nullptr;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int i = lane + 64 * c;
        if (i < L) {
            if (renoise) {
                const double t1 = __dmul_rn(0.75, rowP(p, slot)[i]);
                const double t2 = __dmul_rn(0.25, p.noise_buf[static_cast<size_t>(g) * p.Ap + i]);
                rowP(p, slot)[i] = __dadd_rn(t1, t2);
            }
            // The bar on an inherited root (a fresh root gets it where it is expanded, expand_backup_game). A barred child
            // forgets its statistics and its subtree: N = W = 0, Q = kBarQ, and CH_UNVISITED leaves what hung below it
            // unreachable until the next re-rooting drops it. A child that carries the sentinel of an earlier search of
            // this root and is allowed now is an unvisited child again.
            if (bar) {
                const int a = rowACT(p, slot)[i];
                if ((bar[a >> 6] >> (a & 63)) & 1ull) {
                    rowN(p, slot)[i] = 0;
                    rowW(p, slot)[i] = 0.f;
                    rowQ(p, slot)[i] = kBarQ;
                    rowCH(p, slot)[i] = CH_UNVISITED;
                } else if (rowQ(p, slot)[i] == kBarQ) {
                    rowQ(p, slot)[i] = 0.f;
                }
            }
        }
    }
}

// k_end_move for game g: visit / policy / pi of get_pi (agents.py:64-80), argmax_onehot for tau == 0. One wave in a workgroup of
// its own (the function meets at workgroup barriers). out_pi [A] is written; out_visit / out_policy [A] where not null; pi_lds
// [256], where not null, gets a copy of pi that the same wave may read behind a barrier. mt: the game's stream if the caller has
// it open (the turn draws the tie-break and the action from one open stream), else null -- it is then opened and closed here, for
// tau == 0 only. Returns false, with nothing but the error word written, for a game that is short of its simulations.
template <int NCH>
__device__ __forceinline__ bool end_move_game(const TreeParams& p, const int g, const int tau, MtDev* mt_open, uint32_t* s_mt /*[624]*/,
                                              int* s_vis /*[256]*/, double* s_pol /*[256]*/, double* out_pi, double* out_visit,
                                              double* out_policy, double* pi_lds) {
    const int lane = lane_id();
    // The reference's search always runs its num_mcts simulations (agents.py:105-132): a game that is short of them -- a caller that
    // ends the move early, an over-subscribed search that left its catch-up loop -- gets an error word instead of a pi, and its
    // stream is not touched.
    if (p.sims_done[g] != p.sims_target[g]) {
        if (lane == 0) atomicOr(&p.err[g], ERR_SHORT);
        return false;
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int a = lane + 64 * c;
        if (a < p.A) { s_vis[a] = 0; s_pol[a] = 0.0; }
    }
    __syncthreads();
    const int node = p.root_node[g];
    int tot = 0;
    if (node >= 0) {
        const size_t slot = node_slot(p, p.cur[g], g, node);
        const int L = nodePos(p, slot)->nchild;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int i = lane + 64 * c;
            if (i < L) {
                const int a = rowACT(p, slot)[i];
                const int n = rowN(p, slot)[i];
                s_vis[a] = n;
                s_pol[a] = rowP(p, slot)[i];
                tot += n;
            }
        }
    }
    tot = wave_sum_i(tot);
    __syncthreads();
    const double total = static_cast<double>(tot);
    double pi[NCH];
    int vmax = -1;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int a = lane + 64 * c;
        pi[c] = 0.0;
        if (a < p.A) {
            pi[c] = __ddiv_rn(static_cast<double>(s_vis[a]), total);  // visit / visit.sum()
            vmax = s_vis[a] > vmax ? s_vis[a] : vmax;
            if (out_visit) out_visit[a] = static_cast<double>(s_vis[a]);
            if (out_policy) out_policy[a] = s_pol[a];
        }
    }
    if (tau == 0) {
        // utils.argmax_onehot: np.argwhere(pi == pi.max()) in ascending action order.
        // Equal pi <=> equal visit count (same divisor), so compare the exact integers.
        vmax = wave_max_i(vmax);
        MtDev own;
        MtDev& mt = mt_open ? *mt_open : own;
        if (!mt_open) mt.open(p.mt + static_cast<size_t>(g) * 624, p.mtpos + g, s_mt);
        uint64_t tm[NCH];
        int k = 0;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int a = lane + 64 * c;
            tm[c] = __ballot(a < p.A && s_vis[a] == vmax);
            k += __popcll(tm[c]);
        }
        int r = mt.below(k);
        int pick = -1;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int cnt = __popcll(tm[c]);
            if (pick < 0) {
                if (r < cnt) pick = 64 * c + nth_set_bit(tm[c], r);
                else r -= cnt;
            }
        }
        if (!mt_open) mt.close();
#pragma unroll
        for (int c = 0; c < NCH; ++c) pi[c] = (lane + 64 * c == pick) ? 1.0 : 0.0;
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int a = lane + 64 * c;
        if (a < p.A) {
            out_pi[a] = pi[c];
            if (pi_lds) pi_lds[a] = pi[c];
        }
    }
    return true;
}

// what k_play decided for a game (uniform over the wave); status: AO_ROOT_* of the new root
struct Played { int action, win, status; };

// k_play for game g: utils.get_action on the game's stream over pi [A] (global memory, or LDS written by this wave behind a
// barrier), the env step, and the re-rooting on the chosen child -- at once where the arena has room, else left to k_reroot
// through p.pending_root. One wave in a workgroup of its own. mt: as end_move_game.
template <int NCH>
__device__ __forceinline__ Played play_game(const TreeParams& p, const int g, const double* pi, MtDev* mt_open, uint32_t* s_mt /*[624]*/,
                                            double* s_cdf /*[256]*/) {
    const int lane = lane_id();
    MtDev own;
    MtDev& mt = mt_open ? *mt_open : own;
    if (!mt_open) mt.open(p.mt + static_cast<size_t>(g) * 624, p.mtpos + g, s_mt);
    // cdf = pi.cumsum() (sequential fp64); cdf /= cdf[-1]; searchsorted(cdf, u, 'right')
    if (lane == 0) {
        double s = 0.0;
        for (int a = 0; a < p.A; ++a) {
            const double x = pi[a];
            s = (a == 0) ? x : __dadd_rn(s, x);
            s_cdf[a] = s;
        }
    }
    __syncthreads();
    const double last = s_cdf[p.A - 1];
    const double u = mt.next_double();
    if (!mt_open) mt.close();
    int action = -1;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int a = lane + 64 * c;
        const bool gt = (a < p.A) && (__ddiv_rn(s_cdf[a], last) > u);
        const uint64_t mk = __ballot(gt);
        if (action < 0 && mk) action = 64 * c + __ffsll(static_cast<long long>(mk)) - 1;
    }
    if (action < 0) action = p.A - 1;  // pi == NaN (no visits): numpy would return A here
    // env.step: place the stone, flip the turn, check_win (env_small.py:154-176,196)
    PosR rp = pos_load(p.rootpos + g);
    const bool occupied = pos_occupied(rp, action);
    pos_place(rp, action);
    const int w = win_after_move(rp, action, p.B, p.win_mark);
    // tree reuse: the chosen child becomes the root (main.py:171 -> agents.py:84)
    const int node = p.root_node[g];
    int ch = CH_UNVISITED;
    if (node >= 0) {
        const size_t slot = node_slot(p, p.cur[g], g, node);
        const int found = find_edge<NCH>(p, slot, nodePos(p, slot)->nchild, action);
        if (found >= 0) ch = rowCH(p, slot)[found];
    }
    if (ch >= 0 && w == 0) {
        // The arena is compacted (k_reroot, launched right behind this kernel: the subtree copied into the other arena) only when
        // the next search might not fit behind what is in it: nodes_used <= keep_max = cap - sims - 1 leaves room for every
        // expansion of the next move, so the root just moves to the child and the unreachable nodes stay where they are until a
        // later move needs the room. Same trees, same trims (a subtree above keep_max nodes implies nodes_used above it), a
        // copy every (cap - subtree) / sims moves instead of every move.
        if (lane == 0) {
            if (p.nodes_used[g] <= p.keep_max && !p.compact_always) p.root_node[g] = ch;
            else p.pending_root[g] = ch + 1;
        }
    } else if (lane == 0) {
        p.nodes_used[g] = 0;
        p.root_node[g] = -1;
    }
    // the new root is a record of the reference's dict iff its parent was expanded
    const int status = (ch >= 0 && w == 0) ? 2 : ((node >= 0) ? 1 : 0);
    if (lane == 0) {
        rp.nchild = 0;
        pos_store(p.rootpos + g, rp);
        p.action[g] = action;
        p.win[g] = w;
        p.rstatus[g] = status;
        if (occupied) atomicOr(&p.err[g], ERR_BAD_MOVE);
    }
    return Played{action, w, status};
}

}  // namespace ao
