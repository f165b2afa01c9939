// replay_snapshot_check.hpp -- the canonical form of a replay snapshot (ao_replay_snapshot, include/omok_hip.h). Host code
// only, no HIP: the check walks lengths that come from a file, so it is kept where a host sanitizer can reach it
// (tools/replay_snapshot_check_main.cpp builds it into a stand-alone program). ao_replay_import runs it before anything is
// uploaded: what passes here lets k_replay_unpack (replay_snapshot.hip) read only inside the uploaded arrays.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/omok_hip.h"

namespace ao {

// bits of a snapshot word that stand for cells at or above A (zero when A fills its last word)
inline uint64_t replay_tail_bits(int A) { return (A % 64) ? ~0ull << (A % 64) : 0ull; }

// Empty string: the snapshot is canonical. Otherwise the first violation, naming the field.
inline std::string replay_snapshot_check(const ao_replay_snapshot* s) {
    if (!s) return "null snapshot";
    if (s->board < 3 || s->board > 15) return "board: must be in 3..15";
    if (s->inplanes < 1 || s->inplanes > 32) return "inplanes: must be in 1..32";
    if (s->format != 1) return "format: " + std::to_string(s->format) + " is not a known format (1)";
    const int A = s->board * s->board, W = (A + 63) / 64, C = s->inplanes;
    if (s->words != W) return "words: " + std::to_string(s->words) + ", a board of " + std::to_string(s->board) + " has " + std::to_string(W);
    if (s->entries < 0) return "entries: negative";
    if (s->pi_values < 0) return "pi_values: negative";
    if (s->raw_entries < 0) return "raw_entries: negative";
    if (s->entries > 0 && (!s->kind || !s->z || !s->bits || !s->pi_mask)) return "kind / z / bits / pi_mask: null array";
    if (s->pi_values > 0 && !s->pi_val) return "pi_val: null array";
    if (s->raw_entries > 0 && !s->raw) return "raw: null array";
    const uint64_t tail = replay_tail_bits(A);
    auto at = [](int64_t i, const std::string& m) { return "entry " + std::to_string(i) + ": " + m; };
    int64_t psum = 0, rsum = 0;
    for (int64_t i = 0; i < s->entries; ++i) {
        if (s->kind[i] > 1) return at(i, "kind: " + std::to_string(s->kind[i]) + " is neither 0 nor 1");
        const uint64_t* b = s->bits + static_cast<size_t>(i) * C * W;
        for (int c = 0; c < C; ++c) {
            for (int w = 0; w < W; ++w)
                if (s->kind[i] == 1 && b[c * W + w]) return at(i, "bits: plane " + std::to_string(c) + " of a kind-1 entry is not zero");
            if (b[c * W + W - 1] & tail) return at(i, "bits: plane " + std::to_string(c) + " has a bit at or above cell " + std::to_string(A));
        }
        const uint64_t* m = s->pi_mask + static_cast<size_t>(i) * W;
        if (m[W - 1] & tail) return at(i, "pi_mask: a bit at or above cell " + std::to_string(A));
        for (int w = 0; w < W; ++w) psum += __builtin_popcountll(m[w]);
        rsum += s->kind[i];
        if (psum > s->pi_values) return at(i, "pi_values: the masks' popcounts pass the " + std::to_string(s->pi_values) + " values of pi_val");
        if (rsum > s->raw_entries) return at(i, "raw_entries: the kind-1 entries pass the " + std::to_string(s->raw_entries) + " entries of raw");
    }
    if (psum != s->pi_values) return "pi_values: pi_val holds " + std::to_string(s->pi_values) + " values, the masks' popcounts sum to " + std::to_string(psum);
    if (rsum != s->raw_entries) return "raw_entries: raw holds " + std::to_string(s->raw_entries) + " entries, " + std::to_string(rsum) + " entries are kind 1";
    for (int64_t k = 0; k < s->pi_values; ++k) {
        uint64_t u;
        std::memcpy(&u, s->pi_val + k, sizeof u);
        if (u == 0) return "pi_val: value " + std::to_string(k) + " is the all-zero pattern, which a mask bit never stands for";
    }
    return std::string();
}

}  // namespace ao
