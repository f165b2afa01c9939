// engine.hip -- host driver of the batched self-play engine and the C ABI of include/omok_hip.h.
//
// Per move decision (ZeroAgent.get_pi, agents.py:60-132) the host does exactly three things:
//   1. draws each game's Dirichlet noise from the game's own MT19937 stream (host_rng.hpp;
//      the state is read back from HBM, 2.5 KB per game per move, and written back),
//   2. queues the kernels: k_begin_move, then per simulation k_select -> evaluator ->
//      k_expand_backup, then k_end_move (and k_play for self-play),
//   3. copies the [G][A] result vectors back.
// Everything else lives in HBM and in the kernels of tree_kernels.hip.
//
// Two drivers queue those launches, MoveSearch under ao_search* (here) and the rolling search under ao_roll_* (roll.hip), on one
// footing: what a move is (ao::roll_next_move), its Dirichlet draw (draw_noise), the launch plan and the ring of row counters
// (LaunchLoop), what a failure leaves behind (clear_game_errors). DESIGN.md section 4 says what each driver adds.
//
// This file: the engine's lifecycle, seeding, the symmetry and leaf-tactics switches, the root bar, roots and reset, the step-wise
// protocol, MoveSearch with the fp16-range recovery, and the small getters. ao_engine itself is engine.hpp's; the host drivers of
// the rolling search, the tree read-out, the proven outcomes, the root tactics and the tree snapshots stand beside their kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "engine.hpp"
#include "host_rng.hpp"
#include "launchers.hpp"
#include "symmetry.hpp"
#include "tactics_limits.hpp"

// The keys of the games as the device must see them. A seed call ends here as well: an episode's symmetries follow its seed.
static int sym_upload(ao_engine* e) {
    if (!e->sym_on) return 0;
    AO_HIP(e, hipMemcpyAsync(e->d_sym_key, e->sym_keys.data(), sizeof(uint32_t) * e->G, hipMemcpyHostToDevice, e->stream));
    AO_HIP(e, hipStreamSynchronize(e->stream));
    return 0;
}
static void sym_reseed(ao_engine* e, int g, uint32_t seed) {
    e->sym_seed[g] = seed;
    e->sym_keys[g] = ao::leaf_key(e->sym_base, seed);
}

// ---- the helpers that the engine's other files call as well (declared in engine.hpp) ----------------
namespace ao {

// Inside an open roll the engine's games move on their own clocks: everything that begins, ends or steps a move of the whole
// engine, moves roots or reads trees in bulk is refused until ao_roll_end.
int roll_refuses(ao_engine* e, const char* who) {
    if (!e->roll.open) return 0;
    return e->fail(std::string(who) + ": a roll is open (ao_roll_begin ... ao_roll_end); drain it (ao_roll_drain, ao_roll_run) and close it with ao_roll_end first");
}
// ... and what touches single games is refused for a game that is in a move of the roll
int roll_refuses_game(ao_engine* e, const char* who, int g) {
    if (!e->roll.open || !e->roll.in_move[g]) return 0;
    return e->fail(std::string(who) + ": game " + std::to_string(g) + " is in a move of the open roll");
}

// a launcher refused by walk_lds_bytes (tree_walk.hpp); ao_create's node_cap <= 15000 keeps every engine below that bound
int queue_refused(ao_engine* e, const char* who) {
    return e->fail(std::string(who) + ": the breadth-first queue of a node_cap = " + std::to_string(e->tp.cap) + " arena does not fit the LDS of a workgroup");
}

// leaves the engine usable after a failure: the games' error words cleared, nothing queued any more
void clear_game_errors(ao_engine* e) {
    (void)hipMemsetAsync(e->tp.err, 0, sizeof(int32_t) * e->G, e->stream);
    (void)hipStreamSynchronize(e->stream);
}

// herr [G]: the games' error words as just read from the device. The first game with one fails the call with a message that
// names it; the words are cleared and no move is in flight afterwards.
int report_game_errors(ao_engine* e, const int32_t* herr) {
    for (int g = 0; g < e->G; ++g) {
        if (!herr[g]) continue;
        std::string m = "game " + std::to_string(g) + ":";
        if (herr[g] & ao::ERR_NODE_CAP) m += " tree arena full (raise ao_config.node_cap)";
        if (herr[g] & ao::ERR_PATH) m += " no selectable child (priors are NaN: the policy summed to 0 over the legal moves -- the reference's prior /= prior.sum(), agents.py:189 -- or the tree is inconsistent)";
        if (herr[g] & ao::ERR_BAD_MOVE) m += " move onto an occupied cell";
        if (herr[g] & ao::ERR_SHORT) {
            // the reference always runs num_mcts simulations (agents.py:105-132): a pi from fewer visits is never handed out
            int32_t dt[2] = {0, 0};
            (void)hipMemcpy(&dt[0], e->tp.sims_done + g, sizeof(int32_t), hipMemcpyDeviceToHost);
            (void)hipMemcpy(&dt[1], e->tp.sims_target + g, sizeof(int32_t), hipMemcpyDeviceToHost);
            int nshort = 0, nact = 0;
            for (int k = 0; k < e->G; ++k) { nshort += (herr[k] & ao::ERR_SHORT) ? 1 : 0; nact += e->active[k] ? 1 : 0; }
            m += " search ended after " + std::to_string(dt[0]) + " of " + std::to_string(dt[1]) + " simulations (" + std::to_string(nshort) + " of " +
                 std::to_string(nact) + " active games are short; rows per simulation: " +
                 (e->row_cap > 0 ? std::to_string(e->row_cap) : std::string("one per game")) + ")";
        }
        // leave the engine usable: the error words are cleared and no move is in flight (the caller resets the game)
        clear_game_errors(e);
        e->in_move = false;
        e->ended = false;
        return e->fail(m);
    }
    return 0;
}

// The Dirichlet draws of the games that begin a move with noise, as (game, staging row of its stream in h_mt / h_pos and of its
// noise in h_noise). Every game has its own stream, so the draws do not depend on how the list is cut up: a short one inline, a
// long one on the process's persistent host pool (host_rng.hpp: hardware threads / LOCAL_WORLD_SIZE, at most 32) in chunks of
// 16, so that the ranks of a node do not oversubscribe the host at the start of every move.
void draw_noise(ao_engine* e, const std::vector<std::pair<int32_t, size_t>>& draws) {
    auto work = [&](int k0, int k1) {
        for (int k = k0; k < k1; ++k) {
            const auto [g, row] = draws[k];
            ao::HostMT r{e->h_mt + row * 624, e->h_pos + row, &e->has_gauss[g], &e->gauss[g]};
            r.dirichlet(e->cfg.alpha, e->A - static_cast<int>(e->moves[g].size()), e->h_noise + row * e->Ap);
        }
    };
    const int n = static_cast<int>(draws.size());
    if (n < 64) work(0, n);
    else ao::HostPool::get().run(n, 16, work);
}

// A move that ao::roll_next_move refuses fails the call with a message that names the game (and, in a by-ply table, the ply).
int move_refused(ao_engine* e, const char* who, int g, const ao::RollMove& m, const std::string& at_ply) {
    if (m.refuse == 1)
        return e->fail(std::string(who) + ": game " + std::to_string(g) + ": sims " + std::to_string(m.budget) + at_ply + " is outside 1.." +
                       std::to_string(e->S) + " (the arena and the descent bounds were sized by ao_config.sims)");
    if (m.refuse == 2)
        return e->fail(std::string(who) + ": game " + std::to_string(g) + ": noise asked for on an engine created without noise");
    return 0;
}

// k_settle's counters (settle_queue below), once the stream behind it has been synchronised
void settle_harvest(ao_engine* e, int* unfinished, int* owed) {
    *unfinished = e->h_settle[0];
    *owed = e->h_settle[1];
    e->settled_total += e->h_settle[2];
    e->saved_total += e->h_settle[3];
    e->move_saved += e->h_settle[3];
}

// The pending bar of the masked games (null: all) is dropped: their position changes (ao_play, ao_reset, ao_set_root(s)).
int bar_forget(ao_engine* e, const uint8_t* mask) {
    if (e->bar_keep || (!e->bar_pending && !e->bar_on_device)) return 0;
    bool left = false;
    AO_HIP(e, hipSetDevice(e->cfg.device));
    for (int g = 0; g < e->G; ++g) {
        if (!mask || mask[g]) {
            e->bar_has[g] = 0;
            if (e->bar_on_device)
                AO_HIP(e, hipMemsetAsync(e->d_bar + static_cast<size_t>(g) * ao::kBBWords, 0, sizeof(uint64_t) * ao::kBBWords, e->stream));
        }
        left = left || e->bar_has[g];
    }
    e->bar_pending = left;
    if (!mask) e->bar_on_device = false;
    return 0;
}

// The pending masks as bitboards of barred actions in h_bar, for the games of `act` [G]: the empty cells of a game that its row
// does not allow (ones on stones are ignored). A row that allows none of its game's empty cells is an error that names the game;
// *any: some game is barred from some cell.
int bar_build(ao_engine* e, const std::vector<uint8_t>& act, bool* any, const char* who) {
    const int G = e->G, A = e->A;
    *any = false;
    std::fill(e->h_bar.begin(), e->h_bar.end(), 0ull);
    if (!e->bar_pending) return 0;
    std::vector<uint8_t> stone(A);
    for (int g = 0; g < G; ++g) {
        if (!act[g] || !e->bar_has[g]) continue;
        std::fill(stone.begin(), stone.end(), 0);
        for (int32_t m : e->moves[g]) stone[m] = 1;
        const uint8_t* row = e->bar_allowed.data() + static_cast<size_t>(g) * A;
        uint64_t* bits = e->h_bar.data() + static_cast<size_t>(g) * ao::kBBWords;
        int open = 0, barred = 0;
        for (int a = 0; a < A; ++a) {
            if (stone[a]) continue;
            if (row[a]) { ++open; continue; }
            bits[a >> 6] |= 1ull << (a & 63);
            ++barred;
        }
        if (open == 0 && barred > 0)
            return e->fail(std::string(who) + ": game " + std::to_string(g) + ": the root bar allows no empty cell of the position");
        *any = *any || barred > 0;
    }
    return 0;
}

}  // namespace ao

int LaunchLoop::plan(ao_engine* e_, ao_net* net, int rows) {
    *this = LaunchLoop{e_};
    cap_rows = rows;
    // the network announces the interleaved input layout it wants for a batch of cap_rows boards
    ao::net_plan(net, cap_rows, &e->tp.il_group, &e->tp.nchq, &in_kind);
    // The padding channels of the fp32 input batch (planes 5..31 of a 32-channel slab) are zero and stay zero: the
    // encoder only writes the quads that hold planes (16 B per lane at a 2 KB stride are partial-line writes --
    // rocprof showed 152 MB of HBM writes per launch for a 42 MB batch). A change of layout re-zeroes the buffer.
    // The split-fp16 kernels take the planes as BITS instead (in_kind 2): one byte per cell, 81 contiguous bytes per
    // leaf, and the fp32 batch is not written at all.
    if (in_kind != 2 && (e->il_group_zeroed != e->tp.il_group || e->il_nchq_zeroed != e->tp.nchq)) {
        AO_HIP(e, hipMemsetAsync(e->tp.batch_il, 0, e->il_bytes, e->stream));
        e->il_group_zeroed = e->tp.il_group;
        e->il_nchq_zeroed = e->tp.nchq;
    }
    // select | net | expand+select | net | ... | expand(+idle select): one launch fewer per simulation
    // than the step-wise protocol, same device code (tree_device.hpp).
    lt_serial = getenv("AO_LEAF_TACTICS_SERIAL") != nullptr;   // (read per search, as AO_CATCHUP_ROUNDS is)
    p = e->tp;
    p.batch_nchw = nullptr; p.policy = e->d_policy; p.value = e->d_value; p.row_of_game = e->d_row;
    p.nchq_live = (e->cfg.inplanes + 3) / 4;
    net_in = p.batch_il;
    if (in_kind == 2) {
        net_in = reinterpret_cast<const float*>(e->d_planes_u8);
        p.batch_u8 = e->d_planes_u8;
        p.batch_il = nullptr;
    }
    return 0;
}

int LaunchLoop::zero_ring() { AO_HIP(e, hipMemsetAsync(e->d_live, 0, sizeof(unsigned) * ao_engine::kLive, e->stream)); return 0; }
unsigned* LaunchLoop::slot(int64_t i) const { return per_sim ? e->d_live + (i % ao_engine::kLive) : nullptr; }
unsigned LaunchLoop::counted(int64_t i) const { return e->h_live[slot(i) - e->d_live]; }

int LaunchLoop::advance() {
    ++launch;
    if (wraps(launch) && (harvest(launch) || zero_ring())) return 1;   // more than kLive launches since the ring was zeroed: sum it up, zero it
    p.live = slot(launch);
    return 0;
}

int LaunchLoop::harvest(int64_t upto) {   // (each of the launches [harvested, upto) was followed by a network launch)
    if (!per_sim || upto <= harvested) return 0;
    const ao::RingSpans s = ao::ring_spans(harvested, upto, ao_engine::kLive);
    AO_HIP(e, hipMemcpyAsync(e->h_live + s.first, e->d_live + s.first, sizeof(unsigned) * s.head, hipMemcpyDeviceToHost, e->stream));
    if (s.tail > 0) AO_HIP(e, hipMemcpyAsync(e->h_live, e->d_live, sizeof(unsigned) * s.tail, hipMemcpyDeviceToHost, e->stream));
    AO_HIP(e, hipStreamSynchronize(e->stream));
    if (traffic) *traffic += sizeof(unsigned) * (s.head + s.tail);
    for (int64_t i = harvested; i < upto; ++i) e->rs.add(counted(i), cap_rows);
    harvested = upto;
    return 0;
}

// the solver on the leaves that stand in p.leaf_pos, queued on `s` (leaf_tactics.hip)
static void leaf_tactics_search(ao_engine* e, const ao::TreeParams& p, hipStream_t s) {
    ao::LeafTacticsParams q{};
    q.leaf_pos = p.leaf_pos; q.leaf_status = p.leaf_status; q.active = p.active;
    q.G = p.G; q.B = p.B; q.A = p.A; q.win_mark = p.win_mark; q.max_depth = e->lt_depth; q.max_nodes = e->lt_nodes;
    q.proven = e->d_lt_proven; q.counts = e->d_lt_counts;
    ao::launch_leaf_tactics(q, s);
}

int LaunchLoop::leaf_tactics(bool before_net) {
    if (e->lt_depth == 0) return 0;
    if (before_net) {
        if (lt_serial) return 0;
        AO_HIP(e, hipEventRecord(e->lt_ready, e->stream));
        AO_HIP(e, hipStreamWaitEvent(e->lt_stream, e->lt_ready, 0));
        leaf_tactics_search(e, p, e->lt_stream);
        AO_HIP(e, hipGetLastError());
        AO_HIP(e, hipEventRecord(e->lt_done, e->lt_stream));
        return 0;
    }
    if (lt_serial) leaf_tactics_search(e, p, e->stream);
    else AO_HIP(e, hipStreamWaitEvent(e->stream, e->lt_done, 0));
    ao::launch_leaf_values(e->d_lt_proven, p.row_of_game, e->d_value, p.G, e->stream);
    AO_HIP(e, hipGetLastError());
    return 0;
}

extern "C" {

const char* ao_version(void) { return "alpha_omok_amd 0.1 (gfx950)"; }
int ao_abi_version(void) { return AO_ABI_VERSION; }
int ao_guard_check(int32_t* blocks, int32_t* damaged, char* msg, int cap) { return ao::guard_check(blocks, damaged, msg, cap); }
int ao_guard_block(int32_t index, void** ptr, int64_t* bytes, int64_t* guard) { return ao::guard_block(index, ptr, bytes, guard); }
int ao_guard_mode(int64_t* guard, int32_t* fill) {
    if (guard) *guard = static_cast<int64_t>(ao::guard::guard_bytes(getenv("AO_POOL_GUARD")));
    if (fill) *fill = ao::guard::fill_byte(getenv("AO_POOL_FILL"));
    return 0;
}

const char* ao_last_error(const ao_engine* e) { return e ? e->err.c_str() : ao::create_error<ao_engine>().c_str(); }
void* ao_stream(ao_engine* e) { return e ? e->stream : nullptr; }

int ao_sync(ao_engine* e) {
    AO_HIP(e, hipStreamSynchronize(e->stream));
    return 0;
}

int ao_set_stream(ao_engine* e, void* stream) {
    AO_HIP(e, hipSetDevice(e->cfg.device));
    AO_HIP(e, hipStreamSynchronize(e->stream));
    e->stream = stream ? static_cast<hipStream_t>(stream) : e->own_stream;
    return 0;
}

void ao_destroy(ao_engine* e) {
    if (!e) return;
    hipSetDevice(e->cfg.device);
    if (e->stream) hipStreamSynchronize(e->stream);
    roll_destroy(e);   // (before any buffer goes: a batch of the roll's solver may still be running)
    if (e->lt_stream) {   // (a call that failed between the solver's launch and its join may have left it running)
        hipStreamSynchronize(e->lt_stream);
        if (e->lt_ready) hipEventDestroy(e->lt_ready);
        if (e->lt_done) hipEventDestroy(e->lt_done);
        hipStreamDestroy(e->lt_stream);
    }
    e->pool.free_all();
    if (e->h_mt) hipHostFree(e->h_mt);
    if (e->h_pos) hipHostFree(e->h_pos);
    if (e->h_noise) hipHostFree(e->h_noise);
    if (e->h_out) hipHostFree(e->h_out);
    if (e->h_i32) hipHostFree(e->h_i32);
    if (e->h_live) hipHostFree(e->h_live);
    if (e->h_settle) hipHostFree(e->h_settle);
    e->timer.destroy();
    if (e->own_stream) hipStreamDestroy(e->own_stream);
    delete e;
}

static int create_impl(ao_engine* e, const ao_config* cfg) {
    e->cfg = *cfg;
    ao_config& c = e->cfg;
    if (c.board < 3 || c.board > ao::kMaxBoard) return e->fail("board must be in 3..15");
    if (c.win_mark <= 0) c.win_mark = (c.board == 3) ? 3 : 5;
    // (the five-in-a-row test looks four cells each way from the new stone: marks up to 5. A mark ABOVE the board size is also
    // accepted -- no line can win, the full board is the only end: what ZeroAgent.win_mark = 10 does in the reference, and how the
    // parity suite gets descents that run the whole board)
    if (c.win_mark > 5 && c.win_mark <= c.board) return e->fail("win_mark must be <= 5 (or above the board size: no line wins)");
    if (c.sims < 1) return e->fail("sims must be >= 1");
    if (c.inplanes < 3 || c.inplanes > 9 || (c.inplanes % 2) == 0) return e->fail("inplanes must be 3, 5, 7 or 9");
    if (c.games < 1) return e->fail("games must be >= 1");
    if (c.c_puct == 0.0) c.c_puct = 5.0;
    if (c.alpha == 0.0) c.alpha = 10.0 / static_cast<double>(c.board * c.board);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return e->fail("no HIP device available");
    if (c.device < 0 || c.device >= ndev) return e->fail("device ordinal out of range");
    AO_HIP(e, hipSetDevice(c.device));
    if (c.arena_fraction < 0.0 || c.arena_fraction > 0.90) return e->fail("arena_fraction must be in (0, 0.90] (0 = the default 0.40)");
    const double arena_fraction = c.arena_fraction > 0.0 ? c.arena_fraction : 0.40;
    if (c.node_cap == 0) {
        // Default arena: 16 x (sims + 1) expanded nodes per game where the part is large enough, never less than
        // 4 x (sims + 1). Re-rooting keeps the chosen child's subtree, so with a share f of the root's visits in that
        // child the kept tree settles at f / (1 - f) x sims nodes: 4 x holds f <= 0.75 (a random-init network stays far
        // below), 16 x holds f <= 0.93 -- what a trained, sharp policy needs, and the reference's dict never forgets
        // (agents.py:52). Measured with a network trained by this engine (profiles/r4_trained_*): 10.5 M move decisions at
        // 16 x without a single trim; one self_play(4096) at 11.4 x: 38 of 259 k re-rootings trimmed. The number is
        // DETERMINISTIC for a given device model: bounded by 40 % of the device's TOTAL memory for the two arenas (4096
        // games x 400 sims on a 288 GB MI355X: ~5900 nodes = 14.7 x sims, 124 GB -- trees are what the HBM is for, and two
        // such engines still fit side by side), not by what
        // happens to be free when the engine is created -- whether re-rooting has to forget subtrees (ao_trim_stats) must
        // not depend on the GPU's other tenants.
        const int Ap_ = (c.board * c.board + 15) / 16 * 16;
        const double node_bytes = ao::node_rec_bytes(Ap_);   // the node record: P 8 B + N, Q, CH, W 4 B + ACT 1 B per edge slot + the position, padded to 128
        size_t free_b = 0, total_b = 0;
        long cap = 16L * (c.sims + 1);
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
            cap = std::min<long>(cap, static_cast<long>(arena_fraction * static_cast<double>(total_b) / (2.0 * c.games * node_bytes)));
        cap = std::max<long>(cap, 4L * (c.sims + 1));
        c.node_cap = static_cast<int32_t>(std::min<long>(cap, 15000));
    } else if (c.node_cap < 0) {
        // node_cap = -1, opt-in: grow into the HBM that is free right now -- up to a quarter of it, at most
        // 16 x (sims + 1) -- for sharp (trained) policies that keep more of the tree from move to move. 4096 games x
        // 400 sims on a 288 GB part: ~3400 nodes per arena instead of 1604. The chosen value is reported by ao_node_cap.
        const int Ap_ = (c.board * c.board + 15) / 16 * 16;
        const double node_bytes = ao::node_rec_bytes(Ap_);   // the node record: P 8 B + N, Q, CH, W 4 B + ACT 1 B per edge slot + the position, padded to 128
        size_t free_b = 0, total_b = 0;
        long cap = 4L * (c.sims + 1);
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            const double room = 0.25 * static_cast<double>(free_b) / (2.0 * c.games * node_bytes);
            cap = std::max<long>(cap, std::min<long>(static_cast<long>(room), 16L * (c.sims + 1)));
        }
        c.node_cap = static_cast<int32_t>(std::min<long>(cap, 15000));
        e->node_cap_auto = 1;
    }
    if (c.node_cap < c.sims + 2) return e->fail("node_cap must be at least sims + 2");
    if (c.node_cap > 15000) return e->fail("node_cap must be <= 15000");
    AO_HIP(e, hipStreamCreateWithFlags(&e->own_stream, hipStreamNonBlocking));
    e->stream = e->own_stream;

    const int A = c.board * c.board, Ap = (A + 15) / 16 * 16, G = c.games;
    const int Gp = (G + ao::kGroup - 1) / ao::kGroup * ao::kGroup;
    e->A = A; e->Ap = Ap; e->G = G; e->Gp = Gp; e->S = c.sims;
    ao::TreeParams& p = e->tp;
    p.B = c.board; p.A = A; p.Ap = Ap; p.C = c.inplanes; p.win_mark = c.win_mark; p.G = G;
    p.cap = c.node_cap; p.maxd = A + 2; p.noise = c.noise ? 1 : 0;
    p.keep_max = c.node_cap - c.sims - 1;
    p.compact_always = getenv("AO_COMPACT_ALWAYS") != nullptr;   // developer switch: re-root by copying after every move (rounds 1 - 5)
    p.nchq = (((c.inplanes + 3) / 4) + 7) & ~7;  // worst case of the network's input layouts (net_plan)
    p.nchq_live = p.nchq;
    p.il_group = ao::kGroup;
    p.c_puct = c.c_puct;

    p.rec = ao::node_rec_bytes(Ap);                        // one interleaved record per node (engine_types.hpp)
    // The default arena (ao_config.node_cap == 0) is sized from the device's TOTAL memory: other tenants -- a second engine, torch's
    // training state, a device replay -- may leave less. It then shrinks (x 3/4 per attempt, never below 4 x (sims + 1)) until the
    // allocation succeeds; ao_node_cap reports what was chosen. An explicit node_cap fails as it always did.
    for (;;) {
        const size_t slots = static_cast<size_t>(2) * G * p.cap;
        void* arena = nullptr;
        const hipError_t st = e->pool.alloc_bytes(&arena, slots * p.rec);
        if (st == hipSuccess) {
            p.arena = static_cast<unsigned char*>(arena);
            break;
        }
        (void)hipGetLastError();
        const int floor_cap = 4 * (c.sims + 1);
        if (cfg->node_cap != 0 || p.cap <= floor_cap)
            return e->fail(std::string("hipMalloc(") + std::to_string(slots * p.rec) + " B for the tree arenas): " + hipGetErrorString(st));
        p.cap = std::max(floor_cap, p.cap / 4 * 3);
        c.node_cap = p.cap;
        p.keep_max = c.node_cap - c.sims - 1;
    }
    if (e->pool.alloc(e, &p.cur, G) || e->pool.alloc(e, &p.root_node, G) || e->pool.alloc(e, &p.nodes_used, G) ||
        e->pool.alloc(e, &p.rootpos, G) || e->pool.alloc(e, &p.mt, static_cast<size_t>(G) * 624) ||
        e->pool.alloc(e, &p.mtpos, G) || e->pool.alloc(e, &p.noise_buf, static_cast<size_t>(G) * Ap) ||
        e->pool.alloc(e, &p.sims_target, G) || e->pool.alloc(e, &p.sims_done, G) || e->pool.alloc(e, &p.gflags, G) ||
        e->pool.alloc(e, &p.rstatus, G) || e->pool.alloc(e, &p.pending_root, G) || e->pool.alloc(e, &p.leaf_status, G) || e->pool.alloc(e, &p.path_len, G) ||
        e->pool.alloc(e, &p.path_node, static_cast<size_t>(G) * p.maxd) ||
        e->pool.alloc(e, &p.path_edge, static_cast<size_t>(G) * p.maxd) || e->pool.alloc(e, &p.leaf_pos, G) ||
        e->pool.alloc(e, &p.err, G) || e->pool.alloc(e, &p.trimmed, static_cast<size_t>(G) * 2) || e->pool.alloc(e, &p.stats, static_cast<size_t>(G) * 4) ||
        e->pool.alloc(e, &p.out_pi, static_cast<size_t>(G) * A) || e->pool.alloc(e, &p.out_visit, static_cast<size_t>(G) * A) ||
        e->pool.alloc(e, &p.out_policy, static_cast<size_t>(G) * A) || e->pool.alloc(e, &p.action, G) ||
        e->pool.alloc(e, &p.win, G) || e->pool.alloc(e, &e->d_active, G) || e->pool.alloc(e, &e->d_tau, G) ||
        e->pool.alloc(e, &e->d_extra, static_cast<size_t>(G) * A + 4 * static_cast<size_t>(G)) || e->pool.alloc(e, &e->d_mask, G))
        return 1;
    // evaluation batches of the native network: interleaved input, policy/value rows for Gp boards
    float* il = nullptr;
    if (e->pool.alloc(e, &il, static_cast<size_t>(Gp) * A * p.nchq * 4) ||
        e->pool.alloc(e, &e->d_policy, static_cast<size_t>(Gp) * A) || e->pool.alloc(e, &e->d_value, Gp))
        return 1;
    p.u8_row = A <= 128 ? 128 : 256;
    if (e->pool.alloc(e, &e->d_planes_u8, static_cast<size_t>(Gp) * p.u8_row) || e->pool.alloc(e, &e->d_row, 2 * static_cast<size_t>(G))) return 1;
    if (e->pool.alloc(e, &e->d_mt_backup, static_cast<size_t>(G) * 624) || e->pool.alloc(e, &e->d_pos_backup, G)) return 1;
    if (e->pool.alloc(e, &e->d_live, ao_engine::kLive) || e->pool.alloc(e, &e->d_log_games, G) || e->pool.alloc(e, &e->d_ctl, 8) || e->pool.alloc(e, &e->d_order, G)) return 1;
    if (e->pool.alloc(e, &e->d_settled, G) || e->pool.alloc(e, &e->d_early, G) || e->pool.alloc(e, &e->d_settle, 4)) return 1;
    AO_HIP(e, hipMemsetAsync(e->d_settled, 0, G, e->stream));
    if (e->pool.alloc(e, &e->d_bar, static_cast<size_t>(G) * ao::kBBWords) || e->pool.alloc(e, &e->d_sym_key, G)) return 1;
    p.sym_key = nullptr;
    e->sym_seed.resize(G);
    e->sym_keys.resize(G);
    for (int g = 0; g < G; ++g) sym_reseed(e, g, static_cast<uint32_t>(g));
    e->h_bar.assign(static_cast<size_t>(G) * ao::kBBWords, 0);
    e->bar_has.assign(G, 0);
    p.bar = nullptr;
    e->order_on = !(getenv("AO_TREE_ORDER") && atoi(getenv("AO_TREE_ORDER")) == 0);
    p.order = nullptr;
    AO_HIP(e, hipMemsetAsync(e->d_row, 0, sizeof(int32_t) * 2 * G, e->stream));
    AO_HIP(e, hipMemsetAsync(e->d_live, 0, sizeof(unsigned) * ao_engine::kLive, e->stream));
    p.row_of_game = nullptr;
    p.live = nullptr;
    p.row_cap = 0;
    p.ctl = nullptr; p.ctl_cur = 0; p.live_prev = nullptr; p.row_target = 0; p.max_levels = 0;
    AO_HIP(e, hipMemsetAsync(e->d_planes_u8, 0, static_cast<size_t>(Gp) * p.u8_row, e->stream));
    p.batch_u8 = nullptr;
    e->il_bytes = static_cast<size_t>(Gp) * A * p.nchq * 4 * sizeof(float);
    AO_HIP(e, hipMemsetAsync(il, 0, e->il_bytes, e->stream));
    p.batch_il = il;
    p.tau = e->d_tau;
    p.active = e->d_active;

    // np.sqrt(total_n) for every reachable integer total (correctly rounded by IEEE sqrt)
    const int lut_n = c.sims * (A + 2) + 8;
    std::vector<double> lut(lut_n);
    for (int i = 0; i < lut_n; ++i) lut[i] = std::sqrt(static_cast<double>(i));
    double* d_lut = nullptr;
    if (e->pool.alloc(e, &d_lut, lut_n)) return 1;
    AO_HIP(e, hipMemcpy(d_lut, lut.data(), sizeof(double) * lut_n, hipMemcpyHostToDevice));
    p.sqrt_lut = d_lut; p.sqrt_lut_n = lut_n;

    AO_HIP(e, hipHostMalloc(reinterpret_cast<void**>(&e->h_mt), sizeof(uint32_t) * 624 * G, hipHostMallocDefault));
    AO_HIP(e, hipHostMalloc(reinterpret_cast<void**>(&e->h_pos), sizeof(int32_t) * G, hipHostMallocDefault));
    AO_HIP(e, hipHostMalloc(reinterpret_cast<void**>(&e->h_noise), sizeof(double) * G * Ap, hipHostMallocDefault));
    AO_HIP(e, hipHostMalloc(reinterpret_cast<void**>(&e->h_out), sizeof(double) * 3 * G * A, hipHostMallocDefault));
    AO_HIP(e, hipHostMalloc(reinterpret_cast<void**>(&e->h_i32), sizeof(int32_t) * 4 * G, hipHostMallocDefault));
    AO_HIP(e, hipHostMalloc(reinterpret_cast<void**>(&e->h_live), sizeof(unsigned) * (ao_engine::kLive + 8), hipHostMallocDefault));
    AO_HIP(e, hipHostMalloc(reinterpret_cast<void**>(&e->h_settle), sizeof(int32_t) * 4, hipHostMallocDefault));
    std::memset(e->h_noise, 0, sizeof(double) * G * Ap);

    e->moves.assign(G, {});
    e->status.assign(G, AO_ROOT_FRESH);
    e->over.assign(G, 0);
    e->active.assign(G, 1);
    e->bonus.assign(G, 0);
    e->has_gauss.assign(G, 0);
    e->gauss.assign(G, 0.0);
    for (int g = 0; g < G; ++g) {
        ao::HostMT::seed(e->h_mt + static_cast<size_t>(g) * 624, static_cast<uint32_t>(g));
        e->h_pos[g] = 624;
    }
    AO_HIP(e, hipMemcpyAsync(p.mt, e->h_mt, sizeof(uint32_t) * 624 * G, hipMemcpyHostToDevice, e->stream));
    AO_HIP(e, hipMemcpyAsync(p.mtpos, e->h_pos, sizeof(int32_t) * G, hipMemcpyHostToDevice, e->stream));
    AO_HIP(e, hipMemsetAsync(p.stats, 0, sizeof(unsigned) * 4 * G, e->stream));
    AO_HIP(e, hipMemsetAsync(p.trimmed, 0, sizeof(int32_t) * 2 * G, e->stream));
    AO_HIP(e, hipMemsetAsync(p.noise_buf, 0, sizeof(double) * G * Ap, e->stream));
    ao::launch_reset(p, nullptr, e->stream);
    AO_HIP(e, hipStreamSynchronize(e->stream));
    return 0;
}

int ao_create(const ao_config* cfg, ao_engine** out) {
    if (!cfg || !out) { ao::create_error<ao_engine>() = "null argument"; return 1; }
    ao_engine* e = new ao_engine();
    return ao::finish_create(e, create_impl(e, cfg), out, ao_destroy);
}

// ---- RNG -------------------------------------------------------------------------------------
int ao_set_rng_state(ao_engine* e, int g, const uint32_t* mt, int32_t pos, int32_t has_gauss, double gauss) {
    if (g < 0 || g >= e->G) return e->fail("game index out of range");
    if (e->in_move) return e->fail("ao_set_rng_state / ao_seed inside a move (the move's Dirichlet draw has already consumed the old stream)");
    if (roll_refuses_game(e, "ao_set_rng_state / ao_seed", g)) return 1;
    AO_HIP(e, hipSetDevice(e->cfg.device));
    AO_HIP(e, hipMemcpyAsync(e->tp.mt + static_cast<size_t>(g) * 624, mt, sizeof(uint32_t) * 624,
                             hipMemcpyHostToDevice, e->stream));
    AO_HIP(e, hipMemcpyAsync(e->tp.mtpos + g, &pos, sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    AO_HIP(e, hipStreamSynchronize(e->stream));
    e->has_gauss[g] = has_gauss;
    e->gauss[g] = gauss;
    return 0;
}

int ao_get_rng_state(ao_engine* e, int g, uint32_t* mt, int32_t* pos, int32_t* has_gauss, double* gauss) {
    if (g < 0 || g >= e->G) return e->fail("game index out of range");
    AO_HIP(e, hipSetDevice(e->cfg.device));
    AO_HIP(e, hipMemcpyAsync(mt, e->tp.mt + static_cast<size_t>(g) * 624, sizeof(uint32_t) * 624,
                             hipMemcpyDeviceToHost, e->stream));
    AO_HIP(e, hipMemcpyAsync(pos, e->tp.mtpos + g, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    AO_HIP(e, hipStreamSynchronize(e->stream));
    if (has_gauss) *has_gauss = e->has_gauss[g];
    if (gauss) *gauss = e->gauss[g];
    return 0;
}

int ao_seed(ao_engine* e, int g, uint32_t seed) {
    std::vector<uint32_t> mt(624);
    ao::HostMT::seed(mt.data(), seed);
    if (ao_set_rng_state(e, g, mt.data(), 624, 0, 0.0)) return 1;
    sym_reseed(e, g, seed);
    return sym_upload(e);
}

int ao_seed_games(ao_engine* e, const int32_t* games, const uint32_t* seeds, int32_t n) {
    AO_HIP(e, hipSetDevice(e->cfg.device));
    if (n <= 0) return 0;
    if (e->in_move) return e->fail("ao_seed_games inside a move");
    for (int k = 0; k < n; ++k)
        if (games[k] < 0 || games[k] >= e->G) return e->fail("ao_seed_games: game index out of range");
    for (int k = 0; k < n; ++k)
        if (roll_refuses_game(e, "ao_seed_games", games[k])) return 1;
    AO_HIP(e, hipStreamSynchronize(e->stream));   // (the pinned staging rows are free)
    for (int k = 0; k < n; ++k) {
        const int g = games[k];
        ao::HostMT::seed(e->h_mt + static_cast<size_t>(g) * 624, seeds[k]);
        e->h_pos[g] = 624;
        e->has_gauss[g] = 0;
        e->gauss[g] = 0.0;
        AO_HIP(e, hipMemcpyAsync(e->tp.mt + static_cast<size_t>(g) * 624, e->h_mt + static_cast<size_t>(g) * 624, sizeof(uint32_t) * 624,
                                 hipMemcpyHostToDevice, e->stream));
        AO_HIP(e, hipMemcpyAsync(e->tp.mtpos + g, e->h_pos + g, sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
        sym_reseed(e, g, seeds[k]);
    }
    AO_HIP(e, hipStreamSynchronize(e->stream));
    return sym_upload(e);
}

int ao_seed_all(ao_engine* e, const uint32_t* seeds) {
    if (e->in_move) return e->fail("ao_seed_all inside a move");
    for (int g = 0; g < e->G; ++g)
        if (roll_refuses_game(e, "ao_seed_all", g)) return 1;
    AO_HIP(e, hipSetDevice(e->cfg.device));
    AO_HIP(e, hipStreamSynchronize(e->stream));
    for (int g = 0; g < e->G; ++g) {
        ao::HostMT::seed(e->h_mt + static_cast<size_t>(g) * 624, seeds[g]);
        e->h_pos[g] = 624;
        e->has_gauss[g] = 0;
        e->gauss[g] = 0.0;
        sym_reseed(e, g, seeds[g]);
    }
    AO_HIP(e, hipMemcpyAsync(e->tp.mt, e->h_mt, sizeof(uint32_t) * 624 * e->G, hipMemcpyHostToDevice, e->stream));
    AO_HIP(e, hipMemcpyAsync(e->tp.mtpos, e->h_pos, sizeof(int32_t) * e->G, hipMemcpyHostToDevice, e->stream));
    AO_HIP(e, hipStreamSynchronize(e->stream));
    return sym_upload(e);
}

// ---- leaf symmetries -------------------------------------------------------------------------
// The switch changes what the kernels of the NEXT launch see: e->tp, and the copy an open roll launches with.
static void sym_publish(ao_engine* e) {
    e->tp.sym_key = e->sym_on ? e->d_sym_key : nullptr;
    if (e->roll.open) e->roll.loop.p.sym_key = e->tp.sym_key;
}

int ao_set_leaf_symmetry(ao_engine* e, int enable, uint32_t base_key) {
    if (e->in_move) return e->fail("ao_set_leaf_symmetry inside a move (its leaves so far were evaluated under the old keys)");
    for (int g = 0; g < e->G; ++g)
        if (roll_refuses_game(e, "ao_set_leaf_symmetry", g)) return 1;
    AO_HIP(e, hipSetDevice(e->cfg.device));
    e->sym_on = enable != 0;
    e->sym_base = enable ? base_key : 0u;
    for (int g = 0; g < e->G; ++g) e->sym_keys[g] = ao::leaf_key(e->sym_base, e->sym_seed[g]);
    if (sym_upload(e)) return 1;
    sym_publish(e);
    return 0;
}

int ao_set_leaf_symmetry_keys(ao_engine* e, const int32_t* games, const uint32_t* keys, int32_t n) {
    if (n <= 0) return 0;
    if (e->in_move) return e->fail("ao_set_leaf_symmetry_keys inside a move (its leaves so far were evaluated under the old keys)");
    if (!e->sym_on) return e->fail("ao_set_leaf_symmetry_keys: leaf symmetries are off (ao_set_leaf_symmetry switches them on)");
    if (!games || !keys) return e->fail("ao_set_leaf_symmetry_keys: null buffer");
    for (int k = 0; k < n; ++k)
        if (games[k] < 0 || games[k] >= e->G) return e->fail("ao_set_leaf_symmetry_keys: game index out of range");
    for (int k = 0; k < n; ++k)
        if (roll_refuses_game(e, "ao_set_leaf_symmetry_keys", games[k])) return 1;
    AO_HIP(e, hipSetDevice(e->cfg.device));
    for (int k = 0; k < n; ++k) e->sym_keys[games[k]] = keys[k];
    return sym_upload(e);
}

// ---- leaf tactics ------------------------------------------------------------------------------
// The limits live in the engine, where both launch loops read them at every launch (LaunchLoop::leaf_tactics): an open roll
// needs no copy. Refused like ao_set_leaf_symmetry: a move's leaves so far were valued under the old switch.
int ao_set_leaf_tactics(ao_engine* e, int32_t max_depth, int32_t max_nodes) {
    if (max_depth != 0) {   // (before anything touches the device)
        const std::string bad = ao::fw_limits_error("ao_set_leaf_tactics", max_depth, max_nodes, ao::kLeafMaxNodes);
        if (!bad.empty()) return e->fail(bad);
        if (e->tp.win_mark < 3 || e->tp.win_mark > 5 || e->tp.win_mark > e->cfg.board)
            return e->fail("ao_set_leaf_tactics: the solver needs win_mark in 3..5 and at most the board size");
    }
    if (e->in_move) return e->fail("ao_set_leaf_tactics inside a move (its leaves so far were valued under the old switch)");
    for (int g = 0; g < e->G; ++g)
        if (roll_refuses_game(e, "ao_set_leaf_tactics", g)) return 1;
    if (max_depth != 0 && !e->lt_stream) {
        AO_HIP(e, hipSetDevice(e->cfg.device));
        if (!e->d_lt_proven && (e->pool.alloc(e, &e->d_lt_proven, e->G) || e->pool.alloc(e, &e->d_lt_counts, static_cast<size_t>(e->G) * 4))) return 1;
        AO_HIP(e, hipMemsetAsync(e->d_lt_proven, 0, e->G, e->stream));
        AO_HIP(e, hipMemsetAsync(e->d_lt_counts, 0, sizeof(int32_t) * 4 * e->G, e->stream));
        AO_HIP(e, hipStreamSynchronize(e->stream));
        if (!e->lt_ready) AO_HIP(e, hipEventCreateWithFlags(&e->lt_ready, hipEventDisableTiming));
        if (!e->lt_done) AO_HIP(e, hipEventCreateWithFlags(&e->lt_done, hipEventDisableTiming));
        AO_HIP(e, hipStreamCreateWithFlags(&e->lt_stream, hipStreamNonBlocking));
    }
    e->lt_depth = max_depth;
    e->lt_nodes = max_depth != 0 ? max_nodes : 0;
    return 0;
}

int ao_leaf_tactics_stats(ao_engine* e, int64_t out[4], int32_t* per_game, int reset) {
    for (int k = 0; out && k < 4; ++k) out[k] = 0;
    if (per_game) std::fill(per_game, per_game + static_cast<size_t>(e->G) * 4, 0);
    if (!e->d_lt_counts) return 0;   // never switched on
    AO_HIP(e, hipSetDevice(e->cfg.device));
    AO_HIP(e, hipStreamSynchronize(e->stream));
    AO_HIP(e, hipStreamSynchronize(e->lt_stream));
    std::vector<int32_t> h(static_cast<size_t>(e->G) * 4);
    AO_HIP(e, hipMemcpy(h.data(), e->d_lt_counts, sizeof(int32_t) * h.size(), hipMemcpyDeviceToHost));
    for (size_t i = 0; out && i < h.size(); ++i) out[i & 3] += h[i];
    if (per_game) std::copy(h.begin(), h.end(), per_game);
    if (reset) AO_HIP(e, hipMemset(e->d_lt_counts, 0, sizeof(int32_t) * h.size()));
    return 0;
}

// ---- the root bar ----------------------------------------------------------------------------
int ao_set_root_bar(ao_engine* e, const uint8_t* allowed) {
    if (roll_refuses(e, "ao_set_root_bar")) return 1;
    if (e->in_move) return e->fail("ao_set_root_bar inside a move (between ao_begin_move and ao_end_move)");
    e->bar_on_device = false;
    std::fill(e->bar_has.begin(), e->bar_has.end(), allowed ? 1 : 0);
    e->bar_pending = allowed != nullptr;
    if (allowed) e->bar_allowed.assign(allowed, allowed + static_cast<size_t>(e->G) * e->A);
    return 0;
}

// ---- game / tree state -----------------------------------------------------------------------
int ao_reset(ao_engine* e, const uint8_t* mask) {
    for (int g = 0; g < e->G; ++g)
        if ((!mask || mask[g]) && roll_refuses_game(e, "ao_reset", g)) return 1;
    AO_HIP(e, hipSetDevice(e->cfg.device));
    if (bar_forget(e, mask)) return 1;
    const uint8_t* dmask = nullptr;
    if (mask) {
        AO_HIP(e, hipMemcpyAsync(e->d_mask, mask, e->G, hipMemcpyHostToDevice, e->stream));
        dmask = e->d_mask;
    }
    ao::launch_reset(e->tp, dmask, e->stream);
    AO_HIP(e, hipStreamSynchronize(e->stream));
    for (int g = 0; g < e->G; ++g) {
        if (mask && !mask[g]) continue;
        e->moves[g].clear();
        e->status[g] = AO_ROOT_FRESH;
        e->over[g] = 0;
    }
    e->in_move = false;
    return 0;
}

// Walks the listed games along their new ids in ONE launch (k_walk: a workgroup per listed game).
// ids[k] / ns[k]: full move list of games[k]. Games whose new id does not extend the kept one are reset first.
static int set_roots_impl(ao_engine* e, int count, const int32_t* games, const int32_t* const* ids, const int32_t* ns,
                          int32_t* status) {
    if (roll_refuses(e, "ao_set_root(s)")) return 1;
    AO_HIP(e, hipSetDevice(e->cfg.device));
    if (count <= 0) return 0;
    const int G = e->G, A = e->A;
    std::vector<uint8_t> seen(G, 0);
    for (int k = 0; k < count; ++k) {
        if (games[k] < 0 || games[k] >= G) return e->fail("game index out of range");
        if (seen[games[k]]) return e->fail("ao_set_roots: a game is listed twice");
        seen[games[k]] = 1;
        if (ns[k] < 0 || ns[k] > A) return e->fail("move list too long");
    }
    if (bar_forget(e, seen.data())) return 1;
    // staging: [count][A] new moves, then games / counts / prev_known (device reads), then status (device writes)
    e->h_walk.assign(static_cast<size_t>(count) * A + 4 * static_cast<size_t>(count), 0);
    int32_t* h_extra = e->h_walk.data();
    int32_t* h_games = h_extra + static_cast<size_t>(count) * A;
    int32_t* h_m = h_games + count;
    int32_t* h_pk = h_m + count;
    std::vector<uint8_t> rmask;
    for (int k = 0; k < count; ++k) {
        const int g = games[k];
        const std::vector<int32_t>& cur = e->moves[g];
        const int n = ns[k];
        const bool extends = static_cast<size_t>(n) >= cur.size() && std::equal(cur.begin(), cur.end(), ids[k]);
        int first = 0;
        int prev_known = (e->status[g] != AO_ROOT_FRESH) ? 1 : 0;
        if (!extends) {
            if (rmask.empty()) rmask.assign(G, 0);
            rmask[g] = 1;
            prev_known = 0;
        } else {
            first = static_cast<int>(cur.size());
        }
        h_games[k] = g;
        h_m[k] = n - first;
        h_pk[k] = prev_known;
        std::copy(ids[k] + first, ids[k] + n, h_extra + static_cast<size_t>(k) * A);
    }
    if (!rmask.empty() && ao_reset(e, rmask.data())) return 1;
    int32_t* d_games = e->d_extra + static_cast<size_t>(count) * A;
    AO_HIP(e, hipMemcpyAsync(e->d_extra, h_extra, sizeof(int32_t) * (static_cast<size_t>(count) * A + 3 * static_cast<size_t>(count)),
                             hipMemcpyHostToDevice, e->stream));
    if (ao::launch_walk(e->tp, count, d_games, e->d_extra, A, d_games + count, d_games + 2 * count, d_games + 3 * count, e->stream))
        return queue_refused(e, "ao_set_roots");
    AO_HIP(e, hipGetLastError());
    int32_t* h_st = h_pk + count;
    AO_HIP(e, hipMemcpyAsync(h_st, d_games + 3 * count, sizeof(int32_t) * count, hipMemcpyDeviceToHost, e->stream));
    AO_HIP(e, hipStreamSynchronize(e->stream));
    bool bad = false;
    std::vector<uint8_t> bmask;
    for (int k = 0; k < count; ++k) {
        const int g = games[k];
        if (h_st[k] < 0) {
            if (bmask.empty()) bmask.assign(G, 0);
            bmask[g] = 1;
            bad = true;
            if (status) status[k] = -1;
            continue;
        }
        e->moves[g].assign(ids[k], ids[k] + ns[k]);
        e->status[g] = h_st[k];
        e->over[g] = 0;
        if (status) status[k] = h_st[k];
    }
    if (bad) {
        ao_reset(e, bmask.data());
        return e->fail("ao_set_root: illegal move in the id (occupied cell or out of range)");
    }
    return 0;
}

int ao_set_root(ao_engine* e, int g, const int32_t* mv, int32_t n, int32_t* status) {
    return set_roots_impl(e, 1, &g, &mv, &n, status);
}

int ao_set_roots(ao_engine* e, const uint8_t* mask, const int32_t* moves, int32_t stride, const int32_t* n, int32_t* status) {
    if (!moves || !n) return e->fail("ao_set_roots: null argument");
    std::vector<int32_t> games, ns;
    std::vector<const int32_t*> ids;
    for (int g = 0; g < e->G; ++g) {
        if (mask && !mask[g]) continue;
        games.push_back(g);
        ns.push_back(n[g]);
        ids.push_back(moves + static_cast<size_t>(g) * stride);
        if (n[g] > stride) return e->fail("ao_set_roots: n[g] exceeds the row stride");
    }
    std::vector<int32_t> st(games.size(), 0);
    const int rc = set_roots_impl(e, static_cast<int>(games.size()), games.data(), ids.data(), ns.data(), st.data());
    if (status)
        for (size_t k = 0; k < games.size(); ++k) status[games[k]] = st[k];
    return rc;
}

int ao_get_moves(ao_engine* e, int g, int32_t* out, int32_t* n) {
    if (g < 0 || g >= e->G) return e->fail("game index out of range");
    std::copy(e->moves[g].begin(), e->moves[g].end(), out);
    *n = static_cast<int32_t>(e->moves[g].size());
    return 0;
}

// ---- one move decision -----------------------------------------------------------------------
// sims / noise: per-game budgets and noise switches of ao_begin_move_opts (NULL = the engine's configuration)
static int begin_move_impl(ao_engine* e, const uint8_t* active, const int32_t* sims, const uint8_t* noise) {
    if (roll_refuses(e, "ao_begin_move")) return 1;
    AO_HIP(e, hipSetDevice(e->cfg.device));
    const int G = e->G, Ap = e->Ap;
    ao::TreeParams& p = e->tp;
    // nothing is touched before every value is known to be in range: a refused call leaves the engine as it was (so the games of
    // this move are worked out beside the engine and become e->active once nothing can refuse the call any more)
    std::vector<uint8_t> act(G);
    std::vector<ao::RollMove> mv(G);   // what each game's move is (roll_schedule.hpp): the caller's one budget and one switch per game are table rows of stride 1
    for (int g = 0; g < G; ++g) act[g] = (active ? active[g] : 1) && !e->over[g];
    for (int g = 0; g < G; ++g) {
        if (!act[g]) continue;
        mv[g] = ao::roll_next_move(static_cast<int>(e->moves[g].size()), -1, sims ? sims + g : nullptr, 1, noise ? noise + g : nullptr, 1,
                                   p.noise != 0, e->S, e->status[g]);
        if (move_refused(e, "ao_begin_move_opts", g, mv[g])) return 1;
    }
    // the bar of this move: bitboards that ao_root_tactics left on the device, or the caller's masks (ao_set_root_bar) built here
    const bool bar_dev = e->bar_on_device;
    bool bar_any = false;
    if (!bar_dev && e->bar_pending && bar_build(e, act, &bar_any, "ao_begin_move")) return 1;
    e->active = act;
    const bool bar_pass = bar_dev || bar_any || e->bar_dirty;   // (with none of them the launches are those of an engine without bars)
    if (bar_pass && !bar_dev) {
        if (!bar_any) std::fill(e->h_bar.begin(), e->h_bar.end(), 0ull);
        AO_HIP(e, hipMemcpyAsync(e->d_bar, e->h_bar.data(), sizeof(uint64_t) * e->h_bar.size(), hipMemcpyHostToDevice, e->stream));
    }
    p.bar = bar_pass ? e->d_bar : nullptr;
    e->bar_dirty = bar_dev || bar_any;
    // consumed: the bar is valid for one move (the fp16-range recovery puts `used_*` back for the move it repeats)
    e->used_pending = e->bar_pending; e->used_on_device = bar_dev;
    if (e->bar_pending) { e->used_allowed = e->bar_allowed; e->used_has = e->bar_has; }
    e->bar_pending = false; e->bar_on_device = false;
    std::fill(e->bar_has.begin(), e->bar_has.end(), 0);
    int32_t* target = e->h_i32;
    int32_t* flags = e->h_i32 + G;
    int maxt = 0;
    e->target_sum = 0;
    e->move_saved = 0;
    std::vector<std::pair<int32_t, size_t>> draws;   // (no draw for a game without noise: its stream is not touched)
    for (int g = 0; g < G; ++g) {                    // (a game that is not in this move: all zero)
        e->bonus[g] = mv[g].target - mv[g].budget;   // a fresh root's own expansion (agents.py:107-111)
        target[g] = mv[g].target;
        flags[g] = mv[g].gflags;
        if (mv[g].draw) draws.emplace_back(g, g);
        maxt = std::max(maxt, target[g]);
        e->target_sum += target[g];
    }
    if (p.noise) {
        // The Dirichlet draw is the first consumer of the stream in a move in every case:
        // re-noise of an inherited root (agents.py:97) or the root expansion of sim 0 (:194).
        AO_HIP(e, hipMemcpyAsync(e->h_mt, p.mt, sizeof(uint32_t) * 624 * G, hipMemcpyDeviceToHost, e->stream));
        AO_HIP(e, hipMemcpyAsync(e->h_pos, p.mtpos, sizeof(int32_t) * G, hipMemcpyDeviceToHost, e->stream));
        AO_HIP(e, hipStreamSynchronize(e->stream));
        draw_noise(e, draws);   // (staging row = game: the streams of all games travel)
        AO_HIP(e, hipMemcpyAsync(p.mt, e->h_mt, sizeof(uint32_t) * 624 * G, hipMemcpyHostToDevice, e->stream));
        AO_HIP(e, hipMemcpyAsync(p.mtpos, e->h_pos, sizeof(int32_t) * G, hipMemcpyHostToDevice, e->stream));
        AO_HIP(e, hipMemcpyAsync(p.noise_buf, e->h_noise, sizeof(double) * G * Ap, hipMemcpyHostToDevice, e->stream));
    }
    AO_HIP(e, hipMemcpyAsync(p.sims_target, target, sizeof(int32_t) * G, hipMemcpyHostToDevice, e->stream));
    AO_HIP(e, hipMemcpyAsync(p.gflags, flags, sizeof(int32_t) * G, hipMemcpyHostToDevice, e->stream));
    AO_HIP(e, hipMemcpyAsync(e->d_active, e->active.data(), G, hipMemcpyHostToDevice, e->stream));
    if (e->order_on && e->row_cap > 0 && e->row_cap < G) ao::launch_order(p, e->d_order, e->stream);   // (reads the move's stats that the next line clears)
    AO_HIP(e, hipMemsetAsync(p.stats, 0, sizeof(unsigned) * 4 * G, e->stream));
    if (e->settled_dirty) {
        AO_HIP(e, hipMemsetAsync(e->d_settled, 0, G, e->stream));
        e->settled_dirty = false;
    }
    ao::launch_begin_move(p, e->stream);
    // the pinned staging buffers are reused by the next call: make sure the copies are done
    AO_HIP(e, hipStreamSynchronize(e->stream));
    e->sims_left = maxt;
    e->in_move = true;
    e->ended = false;
    e->leaf_open = false;
    return 0;
}

int ao_begin_move(ao_engine* e, const uint8_t* active) { return begin_move_impl(e, active, nullptr, nullptr); }

int ao_begin_move_opts(ao_engine* e, const uint8_t* active, const int32_t* sims, const uint8_t* noise) {
    return begin_move_impl(e, active, sims, noise);
}

int ao_sims_left(ao_engine* e) { return e->sims_left; }

// k_settle on the engine's stream, counters zeroed in front of it and copied to the pinned words behind it; settle_harvest reads
// them once the stream has been synchronised
static int settle_queue(ao_engine* e, const uint8_t* dmask, int stop_now) {
    AO_HIP(e, hipMemsetAsync(e->d_settle, 0, sizeof(int32_t) * 4, e->stream));
    ao::launch_settle(e->tp, dmask, stop_now, e->leaf_open ? 1 : 0, e->d_settled, e->d_settle, e->stream);
    AO_HIP(e, hipGetLastError());
    AO_HIP(e, hipMemcpyAsync(e->h_settle, e->d_settle, sizeof(int32_t) * 4, hipMemcpyDeviceToHost, e->stream));
    e->settled_dirty = true;
    return 0;
}

int ao_settle(ao_engine* e, const uint8_t* mask, int stop_now, int32_t* unfinished) {
    if (roll_refuses(e, "ao_settle")) return 1;
    if (!e->in_move) return e->fail("ao_settle outside ao_begin_move/ao_end_move");
    AO_HIP(e, hipSetDevice(e->cfg.device));
    const uint8_t* dmask = nullptr;
    if (mask) {
        AO_HIP(e, hipMemcpyAsync(e->d_mask, mask, e->G, hipMemcpyHostToDevice, e->stream));
        dmask = e->d_mask;
    }
    if (settle_queue(e, dmask, stop_now)) return 1;
    AO_HIP(e, hipStreamSynchronize(e->stream));
    int left = 0, owed = 0;
    settle_harvest(e, &left, &owed);
    e->sims_left = owed;
    if (unfinished) *unfinished = left;
    return 0;
}

int ao_search_sims(ao_engine* e, int32_t* sims_run, uint8_t* settled, int64_t* settled_total, int64_t* saved_total) {
    AO_HIP(e, hipSetDevice(e->cfg.device));
    const int G = e->G;
    if (sims_run) {
        std::vector<int32_t> done(G);
        AO_HIP(e, hipMemcpyAsync(done.data(), e->tp.sims_done, sizeof(int32_t) * G, hipMemcpyDeviceToHost, e->stream));
        AO_HIP(e, hipStreamSynchronize(e->stream));
        for (int g = 0; g < G; ++g) sims_run[g] = e->active[g] ? std::max(0, done[g] - e->bonus[g]) : 0;
    }
    if (settled) {
        AO_HIP(e, hipMemcpyAsync(settled, e->d_settled, G, hipMemcpyDeviceToHost, e->stream));
        AO_HIP(e, hipStreamSynchronize(e->stream));
        for (int g = 0; g < G; ++g) settled[g] = e->active[g] ? settled[g] : 0;
    }
    if (settled_total) *settled_total = e->settled_total;
    if (saved_total) *saved_total = e->saved_total;
    return 0;
}

int ao_collect_leaves(ao_engine* e, float* dev_planes_nchw) {
    if (roll_refuses(e, "ao_collect_leaves")) return 1;
    if (!e->in_move) return e->fail("ao_collect_leaves outside ao_begin_move/ao_end_move");
    AO_HIP(e, hipSetDevice(e->cfg.device));
    ao::TreeParams p = e->tp;
    p.batch_nchw = dev_planes_nchw;
    if (dev_planes_nchw) p.batch_il = nullptr;   // an external evaluator only needs the NCHW planes
    else e->il_group_zeroed = -1;                // full-width write in whatever layout was planned last
    ao::launch_select(p, e->stream);
    AO_HIP(e, hipGetLastError());
    e->leaf_open = true;
    return 0;
}

int ao_apply_evals(ao_engine* e, const float* dev_policy, const float* dev_value) {
    if (roll_refuses(e, "ao_apply_evals")) return 1;
    if (!e->in_move) return e->fail("ao_apply_evals outside ao_begin_move/ao_end_move");
    AO_HIP(e, hipSetDevice(e->cfg.device));
    ao::TreeParams p = e->tp;
    p.policy = dev_policy;
    p.value = dev_value;
    if (e->lt_depth != 0) {
        // leaf tactics: the caller's values stay untouched -- the tree launch reads a copy in which the proven leaves hold +1
        AO_HIP(e, hipMemcpyAsync(e->d_value, dev_value, sizeof(float) * e->G, hipMemcpyDeviceToDevice, e->stream));
        leaf_tactics_search(e, p, e->stream);
        ao::launch_leaf_values(e->d_lt_proven, p.row_of_game, e->d_value, e->G, e->stream);
        p.value = e->d_value;
    }
    ao::launch_expand_backup(p, e->stream);
    AO_HIP(e, hipGetLastError());
    if (e->sims_left > 0) --e->sims_left;
    e->leaf_open = false;
    return 0;
}

static int check_game_errors(ao_engine* e) {
    int32_t* herr = e->h_i32 + 2 * e->G;
    AO_HIP(e, hipMemcpyAsync(herr, e->tp.err, sizeof(int32_t) * e->G, hipMemcpyDeviceToHost, e->stream));
    AO_HIP(e, hipStreamSynchronize(e->stream));
    return report_game_errors(e, herr);
}

int ao_end_move(ao_engine* e, const int8_t* tau, double* pi, double* visit, double* policy) {
    if (roll_refuses(e, "ao_end_move")) return 1;
    if (!e->in_move) return e->fail("ao_end_move without ao_begin_move");
    AO_HIP(e, hipSetDevice(e->cfg.device));
    const int G = e->G, A = e->A;
    ao::TreeParams p = e->tp;
    if (tau) {
        AO_HIP(e, hipMemcpyAsync(e->d_tau, tau, G, hipMemcpyHostToDevice, e->stream));
        p.tau = e->d_tau;
    } else {
        p.tau = nullptr;
    }
    ao::launch_end_move(p, e->stream);
    int32_t* hv = e->h_i32;   // (the action row of ao_play: free until then)
    if (e->proof_moves) {
        // the proofs of the active games behind k_end_move (which wrote the error word of a short game), then pi in place
        if (ao::launch_tree_proofs(p, p.active, e->d_pf_ws, 1, e->d_pf_root, e->d_pf_status, e->d_pf_plies, nullptr, nullptr, e->stream))
            return queue_refused(e, "ao_end_move (proof moves)");
        ao::launch_proof_pi(p, e->d_pf_status, e->d_pf_plies, e->d_pf_verdict, e->stream);
        AO_HIP(e, hipGetLastError());
        AO_HIP(e, hipMemcpyAsync(hv, e->d_pf_verdict, sizeof(int32_t) * G, hipMemcpyDeviceToHost, e->stream));
    }
    const size_t n = static_cast<size_t>(G) * A;
    if (pi) AO_HIP(e, hipMemcpyAsync(e->h_out, p.out_pi, sizeof(double) * n, hipMemcpyDeviceToHost, e->stream));
    if (visit) AO_HIP(e, hipMemcpyAsync(e->h_out + n, p.out_visit, sizeof(double) * n, hipMemcpyDeviceToHost, e->stream));
    if (policy) AO_HIP(e, hipMemcpyAsync(e->h_out + 2 * n, p.out_policy, sizeof(double) * n, hipMemcpyDeviceToHost, e->stream));
    if (check_game_errors(e)) return 1;  // synchronises the stream
    if (pi) std::memcpy(pi, e->h_out, sizeof(double) * n);
    if (visit) std::memcpy(visit, e->h_out + n, sizeof(double) * n);
    if (policy) std::memcpy(policy, e->h_out + 2 * n, sizeof(double) * n);
    if (e->proof_moves)
        for (int g = 0; g < G; ++g)
            if (e->active[g]) {
                e->pm_verdict[g] = hv[g];
                e->pm_totals[hv[g] & 3] += 1;
            }
    // after a search every searched root is expanded (it was expanded by sim 0 at the latest)
    for (int g = 0; g < G; ++g)
        if (e->active[g]) e->status[g] = AO_ROOT_EXPANDED;
    e->in_move = false;
    e->ended = true;
    return 0;
}

int ao_play(ao_engine* e, int32_t* action, int32_t* win) {
    if (roll_refuses(e, "ao_play")) return 1;
    if (!e->ended) return e->fail("ao_play must follow ao_end_move");
    AO_HIP(e, hipSetDevice(e->cfg.device));
    const int G = e->G;
    if (bar_forget(e, e->active.data())) return 1;
    if (ao::launch_play(e->tp, e->stream)) return queue_refused(e, "ao_play");
    int32_t* ha = e->h_i32;
    int32_t* hw = e->h_i32 + G;
    int32_t* hs = e->h_i32 + 3 * G;
    AO_HIP(e, hipMemcpyAsync(ha, e->tp.action, sizeof(int32_t) * G, hipMemcpyDeviceToHost, e->stream));
    AO_HIP(e, hipMemcpyAsync(hw, e->tp.win, sizeof(int32_t) * G, hipMemcpyDeviceToHost, e->stream));
    AO_HIP(e, hipMemcpyAsync(hs, e->tp.rstatus, sizeof(int32_t) * G, hipMemcpyDeviceToHost, e->stream));
    if (check_game_errors(e)) return 1;
    for (int g = 0; g < G; ++g) {
        if (!e->active[g]) {
            if (action) action[g] = -1;
            if (win) win[g] = e->over[g];
            continue;
        }
        e->moves[g].push_back(ha[g]);
        e->status[g] = hs[g];
        e->over[g] = hw[g];
        if (action) action[g] = ha[g];
        if (win) win[g] = hw[g];
    }
    e->ended = false;
    return 0;
}

// what ao_search_opts adds to ao_search: per-game budgets and noise switches (ao_begin_move_opts), the games that may be settled
// (k_settle) and how often the loop looks. All null / 0: ao_search.
struct SearchOpts {
    const int32_t* sims = nullptr;
    const uint8_t* noise = nullptr;
    const uint8_t* early_stop = nullptr;
    int settle_every = 0;
};

// One move of ao_search between begin_move_impl and ao_end_move: what its phases share. search_impl runs them top to bottom:
// plan (rows and layout), run_sims (the simulations, with settling), run_planned_extra and run_catch_up (over-subscription),
// finish (row statistics). The arithmetic of the schedule is search_schedule.hpp's; the launch plan and the ring of row counters
// are LaunchLoop's, as under the rolling search.
struct MoveSearch {
    ao_engine* const e;
    ao_net* const net;
    const SearchOpts& opts;
    const DevSwitches& dev = DevSwitches::process();
    // ---- the plan, fixed once plan() has run
    int rows = 0;                  // active games
    LaunchLoop loop;               // cap_rows: ao_set_row_cap's, or one per active game; of p also ctl, ctl_cur, live_prev and row_target change per launch
    ao::StepNet step{};            // the fused per-game step (k_step_board)
    bool fused = false;            // a few games on the per-board path: heads, tree step and the next leaf's conv1 are one launch per game
    bool oversub = false;          // rows per simulation (loop.per_sim), and fewer of them than active games
    bool catch_up = false;         // games may be short of their simulations after the nominal number of launches
    bool settle_on = false;        // k_settle runs every opts.settle_every simulations and in every catch-up round
    ao::SitWindow win{};           // over-subscription: the sit-out window the move starts with (the device takes it from there, sit_window)
    int64_t rows_live_before = 0;  // e->rs.rows_live when the move began (ask_frac)
    // ---- progress
    bool first_sim = true;
    int traced = 0;                // launches whose row counters AO_ROW_TRACE has printed
    bool sit_off = false, all_done = false;   // the catch-up rounds have switched the window off: nobody sits out any more; settling found no unfinished game
    int nominal_sims = 0;          // e->sims_left when the loop began
    std::chrono::steady_clock::time_point t0;   // ... and the time (AO_LAUNCH_TIMING)

    void set_sit(int64_t i) {
        loop.p.ctl = (oversub && !sit_off) ? e->d_ctl : nullptr;
        loop.p.ctl_cur = i & 1;
        loop.p.live_prev = (oversub && i > 0 && !loop.wraps(i)) ? loop.slot(i - 1) : nullptr;   // (the ring was zeroed at a wrap: no demand reading for that launch)
        loop.p.row_target = win.row_target;
    }

    int plan() {
        // The network runs on the ACTIVE games only. Two regimes (engine_types.hpp, TreeParams::live):
        //  * a handful of games on the per-board path with the fused per-game step: the host packs the active games to the front of
        //    the evaluation batch once per move (row_of_game / game_of_row);
        //  * everything else (round 5): the tree kernel hands out the rows PER SIMULATION -- a game whose new leaf needs the network takes
        //    the next row, a terminal leaf takes none (agents.py:171-178,216-221: the reference evaluates it and throws the result
        //    away) -- and counts them in one device word per launch that the trunk kernels read: groups without a live row exit at
        //    once, no host read-back in the loop. With a trained network 11 - 19 % of all leaves are terminal. ao_set_row_cap bounds
        //    the rows of one simulation BELOW the number of games (over-subscription: 5120 games on the 4096 rows = 256 groups the
        //    resident trunk fills the chip with); a leaf that finds the batch full waits for the next launch (LS_WAIT), the catch-up
        //    rounds run until every game has its simulations. A game's search is strictly sequential in every regime: same bits.
        e->h_row.assign(2 * static_cast<size_t>(e->G), 0);
        for (int g = 0; g < e->G; ++g)
            if (e->active[g]) {
                e->h_row[e->G + rows] = g;
                e->h_row[g] = rows++;
            }
        if (rows == 0) return 0;
        const int cap_rows = (!dev.static_rows && e->row_cap > 0 && e->row_cap < rows) ? e->row_cap : rows;
        if (loop.plan(e, net, cap_rows)) return 1;
        ao::TreeParams& p = loop.p;
        // A few games (the per-board network path): heads, tree step and the next leaf's conv1 are ONE launch per game
        // (k_step_board), the network is asked for the residual blocks alone -- 9 launches per simulation instead of 11.
        // (not with leaf tactics: the step computes its own heads, no launch stands between the value and its reader. A one-game
        // ZeroAgent then pays the 11 launches per simulation of the unfused path plus the solver's two: DESIGN.md section 4)
        fused = cap_rows == rows && e->lt_depth == 0 && ao::net_step_params(net, rows, e->d_policy, e->d_value, &step) != 0;
        // (AO_DYNAMIC_ROWS is opt-in: the hand-out costs one atomic per workgroup on one word, ~11 ns each -- 10 us on top of a 20 us tree
        // kernel when 4096 descents of equal depth arrive together, profiles/r5a_row_alloc_atomics.txt; it pays when leaves are terminal)
        loop.per_sim = !fused && !dev.static_rows && (e->row_cap > 0 || dev.dynamic_rows);
        if (loop.per_sim) {
            if (loop.zero_ring()) return 1;
            p.row_cap = static_cast<unsigned>(cap_rows);
        } else {
            AO_HIP(e, hipMemcpyAsync(e->d_row, e->h_row.data(), sizeof(int32_t) * 2 * e->G, hipMemcpyHostToDevice, e->stream));
        }
        oversub = loop.per_sim && cap_rows < rows;   // more active games than rows per simulation: search_schedule.hpp, SitWindow
        p.order = (oversub && e->order_on && e->row_cap > 0 && e->row_cap < e->G) ? e->d_order : nullptr;
        p.max_levels = loop.per_sim ? dev.descent_budget : 0;
        catch_up = oversub || p.max_levels > 0;
        rows_live_before = e->rs.rows_live;
        // Settling (k_settle): every settle_every simulations, and in every catch-up round, the games of the early_stop mask whose move
        // is decided get their targets lowered and the loop goes on with the largest number of simulations still owed -- or ends.
        // Off (no mask or settle_every 0): nothing is launched and nothing is read back.
        settle_on = opts.early_stop != nullptr && opts.settle_every > 0;
        if (settle_on) AO_HIP(e, hipMemcpyAsync(e->d_early, opts.early_stop, e->G, hipMemcpyHostToDevice, e->stream));
        win.row_target = static_cast<unsigned>(cap_rows);
        if (oversub) {
            win = ao::sit_window(rows, e->G, cap_rows, e->ask_frac);
            const float sf = static_cast<float>(win.sit0);
            unsigned* init = e->h_live + ao_engine::kLive;   // (pinned; every move ends with a stream synchronisation)
            std::memset(init, 0, 8 * sizeof(unsigned));
            init[0] = win.sit0;
            std::memcpy(&init[2], &sf, 4);
            AO_HIP(e, hipMemcpyAsync(e->d_ctl, init, 8 * sizeof(unsigned), hipMemcpyHostToDevice, e->stream));
        }
        return 0;
    }

    // AO_ROW_TRACE, behind whatever may have harvested: the launches that the loop has summed up since the last call
    void trace_rows() {
        const int from = traced;
        traced = static_cast<int>(loop.harvested);
        if (!dev.row_trace || traced <= from) return;
        fprintf(stderr, "AO_ROW_TRACE %d active games, %d rows, launches %d..%d, rows asked for:", rows, loop.cap_rows, from, traced - 1);
        for (int i = from; i < traced; ++i) fprintf(stderr, " %u", loop.counted(i));
        fprintf(stderr, "\n");
    }

    // what: 1 = policy + value, 2 = simulation count + leaf status (the fused step computes the heads AND moves on to the next leaf
    // in one kernel: the two halves of a record are taken on either side of it)
    void log_evals(int what) {
        if (e->log_n > 0 && (e->log_sim + 1) * e->log_n * (e->A + 3) <= e->log_cap) {
            ao::launch_eval_log(e->d_log_games, e->log_n, e->d_row, e->d_policy, e->d_value, e->A,
                                e->log_dev + e->log_sim * e->log_n * (e->A + 3), e->tp.sims_done, e->tp.leaf_status, what, e->stream);
            if (what & 1) ++e->log_sim;
        }
    }

    // the one place that queues a network launch followed by a tree launch
    int one_sim() {
        if (loop.leaf_tactics(true)) return 1;
        if (ao::net_forward_il(net, loop.net_in, loop.cap_rows, e->d_policy, e->d_value, e->stream, loop.in_kind, fused ? (first_sim ? 3 : 2) : 7,
                               loop.slot(loop.launch), static_cast<unsigned>(loop.cap_rows)))
            return e->fail(std::string("network forward failed: ") + ao_net_last_error(net));
        first_sim = false;
        log_evals(fused ? 2 : 3);   // (before the tree kernel moves on / hands out the next simulation's rows)
        if (loop.leaf_tactics(false)) return 1;   // (behind the log: it records what the network said)
        const bool timed = e->timer.tick();   // (see ao_tree_timing)
        if (timed) e->timer.begin(e->stream);
        if (loop.advance()) return 1;
        trace_rows();
        if (fused) {
            ao::launch_step_board(loop.p, step, rows, e->d_row + e->G, e->stream);
            log_evals(1);              // (the heads of this simulation ran inside the step kernel)
        } else {
            set_sit(loop.launch);
            ao::launch_expand_select(loop.p, e->stream);
        }
        if (timed) e->timer.end(e->stream);
        AO_HIP(e, hipGetLastError());
        return 0;
    }

    // the first selection, then e->sims_left simulations; with settling the loop looks every opts.settle_every of them
    // (Replaying the per-simulation launch sequence as a HIP graph was measured and is slower than
    // eager launches here: 71.7 vs 65.7 us per simulation for one game)
    int run_sims() {
        if (e->sims_left > 0) {
            loop.p.live = loop.slot(0);
            set_sit(0);
            ao::launch_select(loop.p, e->stream);
            AO_HIP(e, hipGetLastError());
        }
        t0 = std::chrono::steady_clock::now();
        nominal_sims = e->sims_left;
        int since_settle = 0;
        e->leaf_open = e->sims_left > 0;
        while (e->sims_left > 0) {
            const int rc = one_sim();
            --e->sims_left;
            if (rc) return 1;
            if (settle_on && e->sims_left > 0 && ++since_settle >= opts.settle_every) {
                since_settle = 0;
                int unfinished = 0, owed = 0;
                if (settle_queue(e, e->d_early, 0)) return 1;
                AO_HIP(e, hipStreamSynchronize(e->stream));
                settle_harvest(e, &unfinished, &owed);
                all_done = unfinished == 0;
                // (without over-subscription every unfinished game advances by one simulation per launch: `owed` launches are exactly
                // what is left; with it they are a lower bound and the catch-up rounds find the rest)
                e->sims_left = all_done ? 0 : std::min(e->sims_left, owed);
            }
        }
        return 0;
    }

    // over-subscribed, without settling: the launches that the sit-out window costs every game
    int run_planned_extra() {
        if (!(oversub && win.sit_idx > 0 && !settle_on)) return 0;
        const int extra = ao::planned_extra_launches(nominal_sims, e->G, win.sit_idx);
        for (int k = 0; k < extra; ++k)
            if (one_sim()) return 1;
        return 0;
    }

    // Leaves that found their simulation's batch full were expanded one launch later, so some games are short of their
    // simulations: rounds of launches by the rule of search_schedule.hpp's CatchUp. The reference ALWAYS runs num_mcts
    // simulations (agents.py:105-132), so the loop ends in exactly two ways: every active game has its simulations, or an
    // error. Whatever is still short when it ends is reported by k_end_move (ERR_SHORT) -- no result is built from fewer
    // visits than asked for.
    int run_catch_up() {
        if (!catch_up || all_done) return 0;
        const int G = e->G;
        int32_t* h_done = e->h_i32;
        int32_t* h_target = e->h_i32 + G;
        int32_t* h_err = e->h_i32 + 2 * G;
        ao::CatchUp rule(loop.cap_rows, e->S, DevSwitches::catchup_rounds(), DevSwitches::catchup_window_off());
        sit_off = rule.window_off;
        while (rule.open()) {
            if (settle_on && settle_queue(e, e->d_early, 0)) return 1;
            AO_HIP(e, hipMemcpyAsync(h_done, e->tp.sims_done, sizeof(int32_t) * G, hipMemcpyDeviceToHost, e->stream));
            AO_HIP(e, hipMemcpyAsync(h_target, e->tp.sims_target, sizeof(int32_t) * G, hipMemcpyDeviceToHost, e->stream));
            AO_HIP(e, hipMemcpyAsync(h_err, e->tp.err, sizeof(int32_t) * G, hipMemcpyDeviceToHost, e->stream));
            AO_HIP(e, hipStreamSynchronize(e->stream));
            if (settle_on) { int unfinished = 0, owed = 0; settle_harvest(e, &unfinished, &owed); }
            int64_t sum = 0;
            int mx = 0;
            bool bad = false;
            for (int g = 0; g < G; ++g) {
                if (!e->active[g]) continue;
                bad = bad || h_err[g] != 0;
                const int d = h_target[g] - h_done[g];
                if (d > 0) { sum += d; mx = std::max(mx, d); }
            }
            const int extra = rule.next(sum, mx, bad, loop.p.max_levels != 0);
            if (extra == 0) break;
            sit_off = rule.window_off;
            for (int k = 0; k < extra; ++k)
                if (one_sim()) return 1;
        }
        return 0;
    }

    // the row statistics of the move, and the share of its simulations that asked for a row: the next move's window
    int finish() {
        if (loop.harvest(loop.launch)) return 1;
        trace_rows();
        const int64_t sims_wanted = e->target_sum - e->move_saved;   // (the budgets actually set, less what settling took away)
        if (oversub && sims_wanted > 0)
            e->ask_frac = static_cast<double>(e->rs.rows_live - rows_live_before) / static_cast<double>(sims_wanted);
        if (dev.launch_timing) {
            const auto lt1 = std::chrono::steady_clock::now();
            (void)hipStreamSynchronize(e->stream);
            const auto lt2 = std::chrono::steady_clock::now();
            fprintf(stderr, "AO_LAUNCH_TIMING %d simulations: launches enqueued in %.1f us each, stream drained %.1f us after the last enqueue\n", nominal_sims,
                    std::chrono::duration<double, std::micro>(lt1 - t0).count() / (nominal_sims > 0 ? nominal_sims : 1),
                    std::chrono::duration<double, std::micro>(lt2 - lt1).count());
        }
        return 0;
    }
};

static int search_impl(ao_engine* e, ao_net* net, const uint8_t* active, const int8_t* tau, double* pi, double* visit, double* policy,
                       bool may_recover, const SearchOpts& opts);

// The split-fp16 trunk clamps activations beyond the fp16 range and reports it: the evaluations of such a move are
// not the fp32-equivalent ones the engine promises (checked before the per-game errors: clamped evaluations are what
// makes priors degenerate). The move is then searched AGAIN, transparently, on the fp32-MFMA trunk: the games of this
// move get their pre-move MT19937 streams back and FRESH trees at their current positions (ao_set_roots semantics:
// what the search inherited from earlier moves is forgotten -- the one deviation from the reference, which would
// have searched on top of its inherited counts), the caller gets a result instead of an exception and the event is
// counted (ao_fp16_range_events; the Python layer turns it into a warning). The network returns to its requested
// mode afterwards; from the third event of the SAME weights on (counted per network object since its last
// ao_net_finalize) it stays on the fp32-MFMA trunk -- a checkpoint that keeps leaving the range would otherwise search
// every move twice -- until new weights are loaded or ao_net_set_mode is called.
static int recover_fp16_range(ao_engine* e, ao_net* net, const uint8_t* active, const int8_t* tau, double* pi, double* visit,
                              double* policy, bool may_recover, const SearchOpts& opts) {
    clear_game_errors(e);
    e->in_move = false;
    e->ended = false;
    if (!may_recover)
        return e->fail("ao_search: an activation left the fp16 range (|x| > 65504) in the split-fp16 trunk during the repeated move");
    const int G = e->G;
    std::vector<uint8_t> mask(G, 0);
    std::vector<int32_t> games, ns;
    std::vector<std::vector<int32_t>> saved;
    for (int g = 0; g < G; ++g) {
        if (!e->active[g]) continue;
        mask[g] = 1;
        games.push_back(g);
        saved.push_back(e->moves[g]);
        ns.push_back(static_cast<int32_t>(e->moves[g].size()));
    }
    std::vector<const int32_t*> ids;
    for (auto& m : saved) ids.push_back(m.data());
    AO_HIP(e, hipMemcpyAsync(e->tp.mt, e->d_mt_backup, sizeof(uint32_t) * 624 * G, hipMemcpyDeviceToDevice, e->stream));
    AO_HIP(e, hipMemcpyAsync(e->tp.mtpos, e->d_pos_backup, sizeof(int32_t) * G, hipMemcpyDeviceToDevice, e->stream));
    e->has_gauss = e->has_gauss_backup;
    e->gauss = e->gauss_backup;
    // the repeated move is searched under the bar of the first attempt: what begin_move_impl consumed is pending again (the
    // bitboards of an on-device bar are still in d_bar; k_begin_move only reads them), and resetting the games does not drop it
    e->bar_pending = e->used_pending; e->bar_on_device = e->used_on_device;
    if (e->used_pending) { e->bar_allowed = e->used_allowed; e->bar_has = e->used_has; }
    e->bar_keep = true;
    const int rc_reset = ao_reset(e, mask.data()) || set_roots_impl(e, static_cast<int>(games.size()), games.data(), ids.data(), ns.data(), nullptr);
    e->bar_keep = false;
    if (rc_reset) return 1;
    ao::net_fp16_fallback_begin(net);                // mode 2 for the repeated move
    ++e->fp16_events;
    e->fp16_games_redone += static_cast<int64_t>(games.size());
    const int rc = search_impl(e, net, active, tau, pi, visit, policy, false, opts);   // (same budgets, noise switches and mask)
    ao::net_fp16_fallback_end(net);                  // back to the requested mode, unless these weights did it three times
    return rc;
}

static int search_impl(ao_engine* e, ao_net* net, const uint8_t* active, const int8_t* tau, double* pi, double* visit, double* policy,
                       bool may_recover, const SearchOpts& opts) {
    if (roll_refuses(e, "ao_search")) return 1;
    if (!net) return e->fail("ao_search: null network");
    std::string why;
    if (ao::net_check(net, e->cfg.board, e->cfg.inplanes, e->cfg.device, &why)) return e->fail("ao_search: " + why);
    if (may_recover) {
        // what recover_fp16_range needs to run this move again: the streams as they are NOW
        AO_HIP(e, hipSetDevice(e->cfg.device));
        AO_HIP(e, hipMemcpyAsync(e->d_mt_backup, e->tp.mt, sizeof(uint32_t) * 624 * e->G, hipMemcpyDeviceToDevice, e->stream));
        AO_HIP(e, hipMemcpyAsync(e->d_pos_backup, e->tp.mtpos, sizeof(int32_t) * e->G, hipMemcpyDeviceToDevice, e->stream));
        e->has_gauss_backup = e->has_gauss;
        e->gauss_backup = e->gauss;
    }
    if (begin_move_impl(e, active, opts.sims, opts.noise)) return 1;
    MoveSearch m{e, net, opts};
    if (m.plan()) return 1;
    if (m.rows == 0) return ao_end_move(e, tau, pi, visit, policy);
    if (m.run_sims() || m.run_planned_extra() || m.run_catch_up() || m.finish()) return 1;
    int32_t nflags = 0;
    if (ao_net_status(net, e->stream, &nflags, 1)) return e->fail(std::string("ao_net_status: ") + ao_net_last_error(net));
    if (nflags & AO_NET_FP16_RANGE) return recover_fp16_range(e, net, active, tau, pi, visit, policy, may_recover, opts);
    return ao_end_move(e, tau, pi, visit, policy);
}

int ao_search(ao_engine* e, ao_net* net, const uint8_t* active, const int8_t* tau, double* pi,
              double* visit, double* policy) {
    return search_impl(e, net, active, tau, pi, visit, policy, true, SearchOpts{});
}

int ao_search_opts(ao_engine* e, ao_net* net, const uint8_t* active, const int8_t* tau, const int32_t* sims, const uint8_t* noise,
                   const uint8_t* early_stop, int32_t settle_every, double* pi, double* visit, double* policy) {
    if (settle_every < 0) return e->fail("ao_search_opts: settle_every must be >= 0");
    SearchOpts o;
    o.sims = sims; o.noise = noise; o.early_stop = early_stop; o.settle_every = settle_every;
    return search_impl(e, net, active, tau, pi, visit, policy, true, o);
}

int ao_set_row_cap(ao_engine* e, int32_t rows) {
    if (roll_refuses(e, "ao_set_row_cap")) return 1;
    if (rows < 0) return e->fail("ao_set_row_cap: negative");
    if (e->in_move) return e->fail("ao_set_row_cap inside a move");
    e->row_cap = rows;
    return 0;
}

int ao_row_stats(ao_engine* e, int64_t* launches, int64_t* rows_live, int64_t* rows_launched, int64_t* waits) {
    if (launches) *launches = e->rs.launches;
    if (rows_live) *rows_live = e->rs.rows_live;
    if (rows_launched) *rows_launched = e->rs.rows_launched;
    if (waits) *waits = e->rs.waits;
    return 0;
}

int ao_set_eval_log(ao_engine* e, const int32_t* games, int32_t n, float* dev_log, int64_t capacity_floats) {
    if (roll_refuses(e, "ao_set_eval_log")) return 1;
    if (n < 0 || n > e->G) return e->fail("ao_set_eval_log: bad game count");
    if (e->in_move) return e->fail("ao_set_eval_log inside a move");
    AO_HIP(e, hipSetDevice(e->cfg.device));
    for (int k = 0; k < n; ++k)
        if (games[k] < 0 || games[k] >= e->G) return e->fail("ao_set_eval_log: game index out of range");
    if (n > 0) {
        if (!dev_log) return e->fail("ao_set_eval_log: null log buffer");
        AO_HIP(e, hipMemcpyAsync(e->d_log_games, games, sizeof(int32_t) * n, hipMemcpyHostToDevice, e->stream));
        AO_HIP(e, hipStreamSynchronize(e->stream));
    }
    e->log_n = n;
    e->log_dev = dev_log;
    e->log_cap = n > 0 ? capacity_floats : 0;
    e->log_sim = 0;
    return 0;
}

int ao_eval_log_count(ao_engine* e) { return static_cast<int>(e->log_sim); }

int ao_fp16_range_events(ao_engine* e, int64_t* moves_repeated, int64_t* games_redone) {
    if (moves_repeated) *moves_repeated = e->fp16_events;
    if (games_redone) *games_redone = e->fp16_games_redone;
    return 0;
}

int ao_host_threads(void) { return static_cast<int>(ao::HostPool::budget()); }

int ao_node_cap(ao_engine* e, int32_t* node_cap, int32_t* from_free_memory) {
    if (node_cap) *node_cap = e->cfg.node_cap;
    if (from_free_memory) *from_free_memory = e->node_cap_auto;
    return 0;
}

// ---- introspection ---------------------------------------------------------------------------
int ao_get_root_children(ao_engine* e, int g, int32_t* act, double* n, double* w, double* q, double* pr,
                         int32_t* count) {
    if (g < 0 || g >= e->G) return e->fail("game index out of range");
    AO_HIP(e, hipSetDevice(e->cfg.device));
    AO_HIP(e, hipStreamSynchronize(e->stream));
    int32_t cur = 0, root = -1;
    AO_HIP(e, hipMemcpy(&cur, e->tp.cur + g, 4, hipMemcpyDeviceToHost));
    AO_HIP(e, hipMemcpy(&root, e->tp.root_node + g, 4, hipMemcpyDeviceToHost));
    *count = 0;
    if (root < 0) return 0;
    const size_t slot = ao::node_slot(e->tp, cur, g, root);
    ao::Pos m;
    AO_HIP(e, hipMemcpy(&m, ao::nodePos(e->tp, slot), sizeof(m), hipMemcpyDeviceToHost));
    const int L = m.nchild;
    std::vector<int32_t> hn(L); std::vector<float> hw(L), hq(L); std::vector<double> hp(L); std::vector<uint8_t> ha(L);
    AO_HIP(e, hipMemcpy(hn.data(), ao::rowN(e->tp, slot), 4 * L, hipMemcpyDeviceToHost));
    AO_HIP(e, hipMemcpy(hw.data(), ao::rowW(e->tp, slot), 4 * L, hipMemcpyDeviceToHost));
    AO_HIP(e, hipMemcpy(hq.data(), ao::rowQ(e->tp, slot), 4 * L, hipMemcpyDeviceToHost));
    AO_HIP(e, hipMemcpy(hp.data(), ao::rowP(e->tp, slot), 8 * L, hipMemcpyDeviceToHost));
    AO_HIP(e, hipMemcpy(ha.data(), ao::rowACT(e->tp, slot), L, hipMemcpyDeviceToHost));
    for (int i = 0; i < L; ++i) {
        if (act) act[i] = ha[i];
        if (n) n[i] = hn[i];
        if (w) w[i] = hw[i];
        if (q) q[i] = hq[i];
        if (pr) pr[i] = hp[i];
    }
    *count = L;
    return 0;
}

int ao_tree_nodes(ao_engine* e, int g, int64_t* expanded, int64_t* dict_entries) {
    if (g < 0 || g >= e->G) return e->fail("game index out of range");
    AO_HIP(e, hipSetDevice(e->cfg.device));
    AO_HIP(e, hipStreamSynchronize(e->stream));
    int32_t cur = 0, used = 0, root = -1;
    AO_HIP(e, hipMemcpy(&cur, e->tp.cur + g, 4, hipMemcpyDeviceToHost));
    AO_HIP(e, hipMemcpy(&used, e->tp.nodes_used + g, 4, hipMemcpyDeviceToHost));
    AO_HIP(e, hipMemcpy(&root, e->tp.root_node + g, 4, hipMemcpyDeviceToHost));
    // What the root reaches (what del_parents would leave): the arena may also hold nodes of earlier roots that no search can reach
    // any more -- it is compacted only when the next search needs their room (k_play) -- so the records in use are walked from the root.
    int64_t nodes = 0, entries = 0;
    if (used > 0 && root >= 0) {
        std::vector<unsigned char> recs(static_cast<size_t>(used) * e->tp.rec);
        AO_HIP(e, hipMemcpy(recs.data(), ao::node_rec(e->tp, ao::node_slot(e->tp, cur, g, 0)), recs.size(), hipMemcpyDeviceToHost));
        std::vector<int32_t> queue{root};
        for (size_t head = 0; head < queue.size(); ++head) {
            const unsigned char* rec = recs.data() + static_cast<size_t>(queue[head]) * e->tp.rec;
            const ao::Pos* m = reinterpret_cast<const ao::Pos*>(rec + 25u * e->tp.Ap);
            const int32_t* ch = reinterpret_cast<const int32_t*>(rec + 16u * e->tp.Ap);
            entries += m->nchild;
            for (int i = 0; i < m->nchild; ++i)
                if (ch[i] >= 0 && ch[i] < used && queue.size() < static_cast<size_t>(used)) queue.push_back(ch[i]);
        }
        nodes = static_cast<int64_t>(queue.size());
        entries += 1;
    }
    if (expanded) *expanded = nodes;
    if (dict_entries) *dict_entries = entries;
    return 0;
}

int ao_tree_timing(ao_engine* e, int enable, double* ms_total, int64_t* launches) {
    AO_HIP(e, hipSetDevice(e->cfg.device));
    return e->timer.enable(e, enable, ms_total, launches);   // enable = n > 1: every n-th launch carries the event pair (their cost: see net_forward_il)
}

int ao_trim_stats(ao_engine* e, int64_t* subtrees_dropped, int64_t* reroots_trimmed) {
    AO_HIP(e, hipSetDevice(e->cfg.device));
    std::vector<int32_t> per(static_cast<size_t>(e->G) * 2);
    AO_HIP(e, hipMemcpyAsync(per.data(), e->tp.trimmed, sizeof(int32_t) * per.size(), hipMemcpyDeviceToHost, e->stream));
    AO_HIP(e, hipStreamSynchronize(e->stream));
    int64_t a = 0, b = 0;
    for (int g = 0; g < e->G; ++g) { a += per[2 * static_cast<size_t>(g)]; b += per[2 * static_cast<size_t>(g) + 1]; }
    if (subtrees_dropped) *subtrees_dropped = a;
    if (reroots_trimmed) *reroots_trimmed = b;
    return 0;
}

int ao_search_stats(ao_engine* e, int64_t* levels, int64_t* ties, int64_t* terminal, int64_t* evaluated) {
    AO_HIP(e, hipSetDevice(e->cfg.device));
    std::vector<unsigned> per(static_cast<size_t>(e->G) * 4);
    AO_HIP(e, hipMemcpyAsync(per.data(), e->tp.stats, sizeof(unsigned) * per.size(), hipMemcpyDeviceToHost, e->stream));
    AO_HIP(e, hipStreamSynchronize(e->stream));
    unsigned long long h[4] = {0, 0, 0, 0};
    for (int g = 0; g < e->G; ++g)
        for (int k = 0; k < 4; ++k) h[k] += per[static_cast<size_t>(g) * 4 + k];
    if (levels) *levels = static_cast<int64_t>(h[0]);
    if (ties) *ties = static_cast<int64_t>(h[1]);
    if (terminal) *terminal = static_cast<int64_t>(h[2]);
    if (evaluated) *evaluated = static_cast<int64_t>(h[3]);
    return 0;
}

}  // extern "C"
