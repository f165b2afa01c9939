// tree_proofs.hip -- the exact game-theoretic facts a search tree already holds: a visited child whose position ends the game is
// stored as CH_TERMINAL (engine_types.hpp), backup only folds that into W / Q, and nothing else reads it. k_tree_proofs runs an
// exact minimax over what a game's root reaches and says which nodes are PROVEN won, lost or drawn for their side to move, in
// how many plies, and along which line; k_proof_pi (ao_set_proof_moves) lets the root's proof steer the move that is played.
// Both are READ-ONLY on the tree arena. The definition is alpha_omok_amd/utils.py: tree_proofs, proof_pi.
//
// Reference map (paths relative to the reference's 2_AlphaOmok/):
//   k_tree_proofs   (no counterpart)      reads self.tree (agents.py:52) as k_tree_stats does: the same breadth-first walk
//                                         (tree_walk.hpp), then a sweep over its levels from the deepest to the root.
//   k_proof_pi      agents.py:64-80       get_pi's `pi`, rewritten in place behind k_end_move: one-hot on the fastest proven win, or
//                                         renormalised over the children that are not proven lost. Opt-in; off, nothing runs.
//
// A node's proof word is status | plies << 2 in an int32 workspace [G][cap] in HBM, indexed by arena node (the queue alone fills
// the LDS at the largest node_cap). The waves of ONE workgroup hand the words to each other level by level: a workgroup-scope
// release, the barrier, a workgroup-scope acquire. Nothing crosses workgroups.
//
// The host side (ao_tree_proofs, ao_set_proof_moves, ao_proof_move_records, proofs_alloc) follows the kernels.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>

#include "engine.hpp"
#include "launchers.hpp"
#include "tree_walk.hpp"

namespace ao {

constexpr int kProofLevels = kMaxCells + 2;    // int32 words behind the queue: where each ply level begins, and the end of the last

inline size_t proofs_lds_bytes(int cap) {
    const size_t w = walk_lds_bytes(cap);
    const size_t b = w + static_cast<size_t>(kProofLevels) * 4;
    return w && b <= kWalkMaxLds ? b : 0;
}

__device__ __forceinline__ int wave_min_i(int v) { return -wave_max_i(-v); }

// the words of one workgroup's earlier stores are visible to all of its waves behind this
__device__ __forceinline__ void level_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// The values of a node's edges as its mover sees them (utils.tree_proofs): lane's edge e = lane + 64 c gets st[c] (AO_PROOF_*, -1
// for e >= L) and pl[c]. A terminal edge is tested again with win_after_move_by on the node's position (the stone need not be
// placed: the test looks at the cells around it), one wave-wide test per terminal edge; an expanded child reads its word.
template <int NCH>
__device__ __forceinline__ void edge_values(const TreeParams& p, const int32_t* __restrict__ words, size_t slot, const PosR& m, int L,
                                            int (&st)[NCH], int (&pl)[NCH]) {
    const int lane = lane_id();
    const int mover = m.ply & 1;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int e = lane + 64 * c;
        const int ec = e < p.Ap ? e : p.Ap - 1;
        const int ch = rowCH(p, slot)[ec];
        const int act = rowACT(p, slot)[ec];
        st[c] = e < L ? AO_PROOF_UNKNOWN : -1;
        pl[c] = 0;
        if (e < L && link_ok(p, ch)) {
            const int word = words[ch];
            const int cs = word & 3;
            st[c] = cs == AO_PROOF_WIN ? AO_PROOF_LOSS : (cs == AO_PROOF_LOSS ? AO_PROOF_WIN : cs);
            pl[c] = cs != AO_PROOF_UNKNOWN ? (word >> 2) + 1 : 0;
        }
        uint64_t term = __ballot(e < L && ch == CH_TERMINAL);
        while (term) {                                          // (wave-uniform)
            const int l = __ffsll(static_cast<long long>(term)) - 1;
            term &= term - 1;
            const int cell = read_lane(act, l);
            const int w = win_after_move_by(m, cell, p.B, p.win_mark, mover, m.ply + 1);
            if (lane == l) {
                st[c] = w == mover + 1 ? AO_PROOF_WIN : (w == 3 ? AO_PROOF_DRAW : AO_PROOF_UNKNOWN);
                pl[c] = st[c] != AO_PROOF_UNKNOWN ? 1 : 0;
            }
        }
    }
}

// the node rule: any WIN edge -> (WIN, fewest plies); else any UNKNOWN edge -> UNKNOWN; else any DRAW edge -> (DRAW, fewest plies
// among the draws); else (LOSS, most plies). A node without edges is UNKNOWN. Returns the word, wave-uniform.
template <int NCH>
__device__ __forceinline__ int node_word(const int (&st)[NCH], const int (&pl)[NCH], int L) {
    constexpr int kBig = 1 << 20;
    int win = kBig, draw = kBig, loss = -1;
    bool unk = false;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        if (st[c] == AO_PROOF_WIN) win = pl[c] < win ? pl[c] : win;
        if (st[c] == AO_PROOF_DRAW) draw = pl[c] < draw ? pl[c] : draw;
        if (st[c] == AO_PROOF_LOSS) loss = pl[c] > loss ? pl[c] : loss;
        unk = unk || st[c] == AO_PROOF_UNKNOWN;
    }
    win = wave_min_i(win);
    if (win < kBig) return AO_PROOF_WIN | (win << 2);
    if (L <= 0 || __ballot(unk)) return AO_PROOF_UNKNOWN;
    draw = wave_min_i(draw);
    if (draw < kBig) return AO_PROOF_DRAW | (draw << 2);
    return AO_PROOF_LOSS | (wave_max_i(loss) << 2);
}

// ----------------------------------------------------------------------------------------------
// k_tree_proofs: one workgroup of kWalkWaves waves per game with mask[g] != 0 and no error word.
//   forward   walk_subtree over what the root reaches (limit = cap); breadth first, so the depth never decreases along the
//             queue, and level d is the queue entries [lvl[d], lvl[d + 1])
//   backward  the levels from the deepest to the root, one barrier per level, a wave per node (the nodes of a level do not read
//             each other); the wave that holds the root writes the root's edge values by action
//   line      wave 0 follows, while the node is proven, the first edge in stored order that carries the node's own value
// root_out [G][4] = status, plies, proven nodes, nodes walked (-1: the tree reaches more nodes than the arena holds);
// child_status int8 [G][A] (-1: no edge), child_plies int16 [G][A]; line int32 [G][max_len] (-1 beyond) and line_len [G], or both
// null. A masked game without an expanded root (or with an error word) gets zeros, -1 and an empty line.
// ----------------------------------------------------------------------------------------------
template <int NCH>
__global__ __launch_bounds__(64 * kWalkWaves) void k_tree_proofs(TreeParams p, const uint8_t* __restrict__ mask, int32_t* __restrict__ ws,
                                                                 int max_len, int32_t* __restrict__ root_out, int8_t* __restrict__ child_status,
                                                                 int16_t* __restrict__ child_plies, int32_t* __restrict__ line,
                                                                 int32_t* __restrict__ line_len) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
    int32_t* lds = reinterpret_cast<int32_t*>(s_dyn);
    int32_t* s_q = lds + kWalkHdr;
    int32_t* lvl = s_q + p.cap;                           // [kProofLevels]
    const int g = blockIdx.x;
    if (mask && !mask[g]) return;                         // (uniform over the workgroup)
    const int lane = lane_id();
    const int w = threadIdx.x >> 6;
    const size_t rowA = static_cast<size_t>(g) * p.A;
    for (int a = threadIdx.x; a < p.A; a += 64 * kWalkWaves) { child_status[rowA + a] = -1; child_plies[rowA + a] = 0; }
    if (line)
        for (int k = threadIdx.x; k < max_len; k += 64 * kWalkWaves) line[static_cast<size_t>(g) * max_len + k] = -1;
    const int root = p.root_node[g];
    if (!link_ok(p, root) || p.err[g] != 0) {
        if (threadIdx.x == 0) {
            root_out[4 * g + 0] = AO_PROOF_UNKNOWN; root_out[4 * g + 1] = 0; root_out[4 * g + 2] = 0; root_out[4 * g + 3] = 0;
            if (line_len) line_len[g] = 0;
        }
        return;
    }
    const int arena = p.cur[g];
    int32_t* words = ws + static_cast<size_t>(g) * p.cap;
    const int root_ply = pos_load(nodePos(p, node_slot(p, arena, g, root))).ply;
    for (int k = threadIdx.x; k < kProofLevels; k += 64 * kWalkWaves) lvl[k] = p.cap;
    // (walk_subtree begins with a barrier: the fills above are done before any wave records a level)
    const WalkEnd end = walk_subtree<NCH>(
        p, g, arena, root, p.cap, lds,
        [&](const WalkNode& nd, const PosR& m) {
            int d = m.ply - root_ply;
            d = d < 0 ? 0 : (d > kMaxCells ? kMaxCells : d);
            if (lane == 0) atomicMin(&lvl[d], nd.h);
        },
        [](const WalkNode&, int, int, int, bool) {});
    // (behind the walk's last barrier) the deepest level: levels are contiguous, a node's parent is one level up
    int deepest = 0;
    for (int d = 1; d <= kMaxCells && lvl[d] < p.cap; ++d) deepest = d;
    const int tail = end.tail;
    int proven = 0, root_word = AO_PROOF_UNKNOWN;
    for (int d = end.over ? -1 : deepest; d >= 0; --d) {
        const int first = lvl[d];
        const int last = d == deepest ? tail : lvl[d + 1];
        for (int i = first + w; i < last; i += kWalkWaves) {
            const int node = s_q[i];
            const size_t slot = node_slot(p, arena, g, node);
            const PosR m = pos_load(nodePos(p, slot));
            const int L = clamp_nchild(p, m.nchild);
            int st[NCH], pl[NCH];
            edge_values<NCH>(p, words, slot, m, L, st, pl);
            const int word = node_word<NCH>(st, pl, L);
            if (lane == 0) words[node] = word;
            proven += (word & 3) != AO_PROOF_UNKNOWN ? 1 : 0;
            if (i == 0) {                                 // the root: its edges' values by action
                root_word = word;
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    const int e = lane + 64 * c;
                    const int act = rowACT(p, slot)[e < p.Ap ? e : p.Ap - 1];
                    if (e < L && act < p.A) {
                        child_status[rowA + act] = static_cast<int8_t>(st[c]);
                        child_plies[rowA + act] = static_cast<int16_t>(pl[c]);
                    }
                }
            }
        }
        level_barrier();
    }
    if (lane == 0) lds[2 * kWalkWaves + w] = proven;      // (the header's third block is the caller's)
    __syncthreads();
    if (w != 0) return;
    // the proof line (wave 0 held the root: root_word is its own)
    int len = 0;
    if (line && !end.over) {
        int node = root, word = root_word;
        while ((word & 3) != AO_PROOF_UNKNOWN && len < max_len) {
            const size_t slot = node_slot(p, arena, g, node);
            const PosR m = pos_load(nodePos(p, slot));
            const int L = clamp_nchild(p, m.nchild);
            int st[NCH], pl[NCH];
            edge_values<NCH>(p, words, slot, m, L, st, pl);
            int esel = -1;
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const uint64_t mk = __ballot(st[c] == (word & 3) && pl[c] == (word >> 2));
                if (esel < 0 && mk) esel = 64 * c + __ffsll(static_cast<long long>(mk)) - 1;
            }
            if (esel < 0) break;                          // (an inconsistent tree: no edge carries the node's value)
            if (lane == 0) line[static_cast<size_t>(g) * max_len + len] = rowACT(p, slot)[esel];
            ++len;
            const int ch = rowCH(p, slot)[esel];
            if (!link_ok(p, ch)) break;                   // a terminal edge ends the line
            node = ch;
            word = words[ch];
        }
    }
    if (lane == 0) {
        int total = 0;
        for (int k = 0; k < kWalkWaves; ++k) total += lds[2 * kWalkWaves + k];
        root_out[4 * g + 0] = end.over ? AO_PROOF_UNKNOWN : (root_word & 3);
        root_out[4 * g + 1] = end.over ? 0 : (root_word >> 2);
        root_out[4 * g + 2] = end.over ? 0 : total;
        root_out[4 * g + 3] = end.over ? -1 : tail;
        if (line_len) line_len[g] = len;
    }
}

// ----------------------------------------------------------------------------------------------
// k_proof_pi: utils.proof_pi on TreeParams::out_pi in place, one wave per active game; verdict[g] = AO_PM_*. An active game
// without an expanded root or with an error word (ERR_SHORT: k_end_move wrote no pi) gets AO_PM_NONE; an inactive game keeps
// its rows. out_visit / out_policy are read only.
// ----------------------------------------------------------------------------------------------
template <int NCH>
__global__ __launch_bounds__(64) void k_proof_pi(TreeParams p, const int8_t* __restrict__ child_status, const int16_t* __restrict__ child_plies,
                                                 int32_t* __restrict__ verdict) {
    constexpr int kBig = 1 << 20;
    const int g = blockIdx.x;
    if (p.active && !p.active[g]) return;
    const int lane = lane_id();
    if (!link_ok(p, p.root_node[g]) || p.err[g] != 0) {
        if (lane == 0) verdict[g] = AO_PM_NONE;
        return;
    }
    const size_t row = static_cast<size_t>(g) * p.A;
    int st[NCH], pl[NCH], vis[NCH];
    double pi[NCH];
    bool lost_pi = false, loss = false, other = false;
    int win = kBig;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int a = lane + 64 * c;
        const bool in = a < p.A;
        st[c] = in ? child_status[row + a] : -1;
        pl[c] = in ? child_plies[row + a] : 0;
        pi[c] = in ? p.out_pi[row + a] : 0.0;
        vis[c] = in ? static_cast<int>(p.out_visit[row + a]) : 0;
        if (st[c] == AO_PROOF_WIN) win = pl[c] < win ? pl[c] : win;
        loss = loss || st[c] == AO_PROOF_LOSS;
        lost_pi = lost_pi || (st[c] == AO_PROOF_LOSS && pi[c] > 0.0);
        other = other || st[c] == AO_PROOF_UNKNOWN || st[c] == AO_PROOF_DRAW;
    }
    win = wave_min_i(win);
    int v = AO_PM_NONE, pick = -1;
    double s = 0.0;
    if (win < kBig) {
        // the WIN edge with the fewest plies; ties to the larger visit count, then to the lowest action
        v = AO_PM_WIN;
        int best = -1;
#pragma unroll
        for (int c = 0; c < NCH; ++c)
            if (st[c] == AO_PROOF_WIN && pl[c] == win) best = vis[c] > best ? vis[c] : best;
        best = wave_max_i(best);
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const uint64_t mk = __ballot(st[c] == AO_PROOF_WIN && pl[c] == win && vis[c] == best);
            if (pick < 0 && mk) pick = 64 * c + __ffsll(static_cast<long long>(mk)) - 1;
        }
    } else if (__ballot(loss) && __ballot(other) && __ballot(lost_pi)) {
        v = AO_PM_PRUNED;
        // s = the sum of pi over the edges that are not LOSS: sequential fp64 in ascending action order, on one lane (as play_game's cdf)
        if (lane == 0) {
            for (int a = 0; a < p.A; ++a) {
                const int sa = child_status[row + a];
                if (sa == AO_PROOF_UNKNOWN || sa == AO_PROOF_DRAW) s = __dadd_rn(s, p.out_pi[row + a]);
            }
        }
        s = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(s)), __builtin_amdgcn_readfirstlane(__double2loint(s)));
        if (!(s > 0.0)) {
            // every bit of pi sits on lost moves (a tau == 0 one-hot): the non-lost edge with the most visits, lowest action on ties
            v = AO_PM_MOVED;
            int best = -1;
#pragma unroll
            for (int c = 0; c < NCH; ++c)
                if (st[c] == AO_PROOF_UNKNOWN || st[c] == AO_PROOF_DRAW) best = vis[c] > best ? vis[c] : best;
            best = wave_max_i(best);
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const uint64_t mk = __ballot((st[c] == AO_PROOF_UNKNOWN || st[c] == AO_PROOF_DRAW) && vis[c] == best);
                if (pick < 0 && mk) pick = 64 * c + __ffsll(static_cast<long long>(mk)) - 1;
            }
        }
    }
    if (v != AO_PM_NONE) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int a = lane + 64 * c;
            if (a >= p.A) continue;
            double out;
            if (v == AO_PM_PRUNED) out = (st[c] == AO_PROOF_UNKNOWN || st[c] == AO_PROOF_DRAW) ? __ddiv_rn(pi[c], s) : 0.0;
            else out = a == pick ? 1.0 : 0.0;
            p.out_pi[row + a] = out;
        }
    }
    if (lane == 0) verdict[g] = v;
}

// ----------------------------------------------------------------------------------------------
// launchers: both are ao_end_move's as well (engine.hip, under ao_set_proof_moves), so launchers.hpp declares them
// ----------------------------------------------------------------------------------------------

// non-zero: queue and level table of a `cap`-node arena do not fit the LDS of one workgroup -- nothing is launched
int launch_tree_proofs(const TreeParams& p, const uint8_t* mask, int32_t* ws, int max_len, int32_t* root_out, int8_t* child_status,
                       int16_t* child_plies, int32_t* line, int32_t* line_len, hipStream_t s) {
    const size_t lds = proofs_lds_bytes(p.cap);
    if (!lds) return 1;
    AO_DISPATCH_NCH(nch_of_cells(p.A), hipLaunchKernelGGL(k_tree_proofs<NCH>, dim3(p.G), dim3(64 * kWalkWaves), lds, s, p, mask, ws, max_len,
                                                          root_out, child_status, child_plies, line, line_len));
    return 0;
}

void launch_proof_pi(const TreeParams& p, const int8_t* child_status, const int16_t* child_plies, int32_t* verdict, hipStream_t s) {
    AO_DISPATCH_NCH(nch_of_cells(p.A), hipLaunchKernelGGL(k_proof_pi<NCH>, dim3(p.G), dim3(64), 0, s, p, child_status, child_plies, verdict));
}

// ----------------------------------------------------------------------------------------------
// the host side
// ----------------------------------------------------------------------------------------------
int proofs_alloc(ao_engine* e) {
    if (e->d_pf_ws) return 0;
    const size_t G = static_cast<size_t>(e->G), A = static_cast<size_t>(e->A);
    AO_HIP(e, hipSetDevice(e->cfg.device));
    if (e->pool.alloc(e, &e->d_pf_root, 4 * G) || e->pool.alloc(e, &e->d_pf_status, G * A) || e->pool.alloc(e, &e->d_pf_plies, G * A) ||
        e->pool.alloc(e, &e->d_pf_verdict, G) || e->pool.alloc(e, &e->d_pf_ws, G * static_cast<size_t>(e->tp.cap)))
        return 1;
    AO_HIP(e, hipMemsetAsync(e->d_pf_verdict, 0, sizeof(int32_t) * G, e->stream));
    return 0;
}

}  // namespace ao

extern "C" {

// utils.tree_proofs of every masked game
int ao_tree_proofs(ao_engine* e, const uint8_t* mask, int32_t max_len, int32_t* root, int8_t* child_status, int16_t* child_plies,
                   int32_t* line, int32_t* line_len) {
    if (roll_refuses(e, "ao_tree_proofs")) return 1;
    if (e->in_move) return e->fail("ao_tree_proofs inside a move (between ao_begin_move and ao_end_move)");
    if (max_len < 1 || max_len > e->A) return e->fail("ao_tree_proofs: max_len must be in 1..A");
    const size_t G = static_cast<size_t>(e->G), A = static_cast<size_t>(e->A), GL = G * static_cast<size_t>(max_len);
    // workspace layout: line [G][max_len] and line_len [G] (int32), root [G][4] (int32), plies [G][A] (int16), status [G][A], mask [G]
    const size_t o_len = 4 * GL, o_root = o_len + 4 * G, o_plies = o_root + 16 * G, o_status = o_plies + 2 * G * A, o_mask = o_status + G * A;
    if (readout_begin(e, "ao_tree_proofs", o_mask + G) || proofs_alloc(e)) return 1;
    uint8_t* h_mask = e->h_ro.data() + o_mask;
    readout_mask(e, mask, h_mask);
    unsigned char* d = e->d_ro.p;
    AO_HIP(e, hipMemcpyAsync(d + o_mask, h_mask, G, hipMemcpyHostToDevice, e->stream));
    if (ao::launch_tree_proofs(e->tp, d + o_mask, e->d_pf_ws, max_len, reinterpret_cast<int32_t*>(d + o_root), reinterpret_cast<int8_t*>(d + o_status),
                               reinterpret_cast<int16_t*>(d + o_plies), reinterpret_cast<int32_t*>(d), reinterpret_cast<int32_t*>(d + o_len), e->stream))
        return queue_refused(e, "ao_tree_proofs");
    AO_HIP(e, hipGetLastError());
    AO_HIP(e, hipMemcpyAsync(e->h_ro.data(), d, o_mask, hipMemcpyDeviceToHost, e->stream));
    AO_HIP(e, hipStreamSynchronize(e->stream));
    const unsigned char* h = e->h_ro.data();
    const int32_t* h_root = reinterpret_cast<const int32_t*>(h + o_root);
    for (size_t g = 0; g < G; ++g)
        if (h_mask[g] && h_root[4 * g + 3] < 0) return e->fail("ao_tree_proofs: game " + std::to_string(g) + ": the tree reaches more nodes than the arena holds (inconsistent tree)");
    for (size_t g = 0; g < G; ++g) {
        if (!h_mask[g]) continue;
        if (root) std::memcpy(root + 4 * g, h_root + 4 * g, 16);
        if (child_status) std::memcpy(child_status + g * A, h + o_status + g * A, A);
        if (child_plies) std::memcpy(child_plies + g * A, h + o_plies + 2 * g * A, 2 * A);
        if (line) std::memcpy(line + g * max_len, h + 4 * g * max_len, 4 * static_cast<size_t>(max_len));
        if (line_len) line_len[g] = reinterpret_cast<const int32_t*>(h + o_len)[g];
    }
    return 0;
}

int ao_set_proof_moves(ao_engine* e, int enable) {
    if (roll_refuses(e, "ao_set_proof_moves")) return 1;
    if (e->in_move) return e->fail("ao_set_proof_moves inside a move (between ao_begin_move and ao_end_move)");
    if (enable) {
        if (!ao::reroot_fits(e->tp)) return queue_refused(e, "ao_set_proof_moves");
        if (proofs_alloc(e)) return 1;
        if (e->pm_verdict.empty()) e->pm_verdict.assign(e->G, 0);
    }
    e->proof_moves = enable != 0;
    return 0;
}

int ao_proof_move_records(ao_engine* e, int32_t* verdict, int64_t totals[4], int reset) {
    if (verdict)
        for (int g = 0; g < e->G; ++g) verdict[g] = e->pm_verdict.empty() ? 0 : e->pm_verdict[g];
    if (totals) std::memcpy(totals, e->pm_totals, sizeof(e->pm_totals));
    if (reset) std::fill(e->pm_totals, e->pm_totals + 4, 0);
    return 0;
}

}  // extern "C"
