// replay_ring.hpp -- the replay memory's handle, shared by replay.hip (extend / gather / read) and replay_snapshot.hip
// (export / import): three rings in HBM, deque index i in slot (head + i) % cap.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/omok_hip.h"

struct ao_replay {
    int B = 0, C = 0, A = 0, device = 0;
    int64_t cap = 0, head = 0, count = 0;  // deque index i lives in slot (head + i) % cap
    float* s_ring = nullptr;
    double* pi_ring = nullptr;
    float* z_ring = nullptr;
    // staging (grow-only)
    float* st_s = nullptr; double* st_pi = nullptr; float* st_z = nullptr; long* st_idx = nullptr;
    int64_t st_n = 0, st_m = 0;
    short* st_mv = nullptr; int* st_ep = nullptr; int* st_ply = nullptr;   // moves-based extend: episodes' moves, (episode, ply) per sample
    int64_t st_mv_n = 0, st_ep_n = 0;
    std::string err;
    int fail(const std::string& m) { err = m; return 1; }
};

// what ao_replay_last_error(NULL) returns: the failed ao_replay_create or ao_replay_snapshot_check of this thread
inline thread_local std::string g_replay_create_error;

#define RP_HIP(r, call)                                                                        \
    do {                                                                                       \
        hipError_t st_ = (call);                                                               \
        if (st_ != hipSuccess) return (r)->fail(std::string(#call) + ": " + hipGetErrorString(st_)); \
    } while (0)
