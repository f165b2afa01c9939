// replay_ring.hpp -- the replay memory's handle, shared by replay.hip (extend / gather / read) and replay_snapshot.hip
// (export / import): three rings in HBM, deque index i in slot (head + i) % cap.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/omok_hip.h"
#include "host_handle.hpp"

// ao_replay_last_error(NULL) (ao::create_error<ao_replay>) speaks of this thread's failed ao_replay_create or ao_replay_snapshot_check
struct ao_replay : ao::HandleBase {
    int B = 0, C = 0, A = 0, device = 0;
    int64_t cap = 0, head = 0, count = 0;  // deque index i lives in slot (head + i) % cap
    ao::DevPool pool;
    float* s_ring = nullptr;
    double* pi_ring = nullptr;
    float* z_ring = nullptr;
    // staging (grow-only)
    ao::DevBuf<float> st_s{&pool}; ao::DevBuf<double> st_pi{&pool}; ao::DevBuf<float> st_z{&pool}; ao::DevBuf<long> st_idx{&pool};
    ao::DevBuf<short> st_mv{&pool}; ao::DevBuf<int> st_ep{&pool}; ao::DevBuf<int> st_ply{&pool};   // moves-based extend: episodes' moves, (episode, ply) per sample
};
