// Drives alpha_omok_amd/csrc/pool_guard.hpp on plain host memory (tests/test_pool_guard_host.py). One command per input line,
// one output line per command:
//   round TEXT             -> guard bytes for AO_POOL_GUARD=TEXT ("-" stands for unset)
//   fill TEXT              -> fill byte for AO_POOL_FILL=TEXT ("-" stands for unset)
//   layout BYTES GUARD     -> total body_offset rear_offset
//   new BYTES GUARD FILL   -> ordinal of a new block: malloc(total), all of it filled, registered
//   poke I OFF VALUE       -> "ok": writes VALUE at body + OFF of live block I (OFF < 0: front guard, OFF >= bytes: rear guard)
//   body I                 -> number of body bytes of live block I that differ from its fill
//   free I                 -> "ok": checks the guards as the pool does at free time (damage becomes sticky), then frees
//   check CAP              -> blocks damaged strlen|message with '\n' shown as ';' (guards are repaired as ao_guard_check does)
//   live                   -> number of live blocks
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "pool_guard.hpp"

namespace g = ao::guard;

static unsigned char* base_of(const g::Entry& e) { return static_cast<unsigned char*>(e.ptr) - g::body_offset(e.guard); }

static g::Damage damage_of(const g::Entry& e) {
    const unsigned char* base = base_of(e);
    return g::compare(base, base + g::rear_offset(e.bytes, e.guard), e.guard, e.fill);
}

int main() {
    g::Registry& reg = g::registry();
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "round" || cmd == "fill") {
            std::string text;
            in >> text;
            const char* t = text == "-" ? nullptr : text.c_str();
            if (cmd == "round") std::printf("%zu\n", g::guard_bytes(t));
            else std::printf("%d\n", static_cast<int>(g::fill_byte(t)));
        } else if (cmd == "layout") {
            size_t bytes = 0, guard = 0;
            in >> bytes >> guard;
            std::printf("%zu %zu %zu\n", g::total_bytes(bytes, guard), g::body_offset(guard), g::rear_offset(bytes, guard));
        } else if (cmd == "new") {
            size_t bytes = 0, guard = 0;
            int fill = 0;
            in >> bytes >> guard >> fill;
            const size_t total = g::total_bytes(bytes, guard);
            unsigned char* base = static_cast<unsigned char*>(std::malloc(total));
            std::memset(base, fill, total);
            std::lock_guard<std::mutex> lock(reg.mu);
            const g::Entry& e = reg.add(0, base + g::body_offset(guard), bytes, guard, static_cast<uint8_t>(fill));
            std::printf("%llu\n", static_cast<unsigned long long>(e.ordinal));
        } else if (cmd == "poke") {
            int i = 0, value = 0;
            long long off = 0;
            in >> i >> off >> value;
            const g::Entry& e = reg.live.at(i);
            if (off < -static_cast<long long>(e.guard) || off >= static_cast<long long>(e.bytes + e.guard)) {
                std::printf("outside the allocation\n");
                continue;
            }
            static_cast<unsigned char*>(e.ptr)[off] = static_cast<unsigned char>(value);
            std::printf("ok\n");
        } else if (cmd == "body") {
            int i = 0;
            in >> i;
            const g::Entry& e = reg.live.at(i);
            std::printf("%lld\n", static_cast<long long>(g::scan(static_cast<const uint8_t*>(e.ptr), e.bytes, e.fill).count));
        } else if (cmd == "free") {
            int i = 0;
            in >> i;
            std::lock_guard<std::mutex> lock(reg.mu);
            const g::Entry e = reg.live.at(i);
            if (reg.find(e.ptr) != i) {
                std::printf("find disagrees\n");
                continue;
            }
            reg.remove(i);
            const g::Damage d = damage_of(e);
            if (d.any()) reg.sticky.push_back(g::describe(e, d) + " [found when freed]");
            std::free(base_of(e));
            std::printf("ok\n");
        } else if (cmd == "check") {
            int cap = 0;
            in >> cap;
            std::lock_guard<std::mutex> lock(reg.mu);
            std::vector<std::string> fresh;
            for (const g::Entry& e : reg.live) {
                const g::Damage d = damage_of(e);
                if (!d.any()) continue;
                fresh.push_back(g::describe(e, d));
                std::memset(base_of(e), e.fill, e.guard);
                std::memset(base_of(e) + g::rear_offset(e.bytes, e.guard), e.fill, e.guard);
            }
            const std::vector<std::string> all = reg.take_report(fresh);
            // a canary behind the message: write_report must stay within cap
            std::vector<char> msg(static_cast<size_t>(cap > 0 ? cap : 0) + 8, '#');
            g::write_report(all, msg.data(), cap);
            bool canary = true;
            for (size_t k = static_cast<size_t>(cap > 0 ? cap : 0); k < msg.size(); ++k) canary = canary && msg[k] == '#';
            std::string text = cap > 0 ? std::string(msg.data()) : std::string();
            for (char& c : text) if (c == '\n') c = ';';
            std::printf("%zu %zu %zu%s|%s\n", reg.live.size(), all.size(), text.size(), canary ? "" : " OVERRUN", text.c_str());
        } else if (cmd == "live") {
            std::printf("%zu\n", reg.live.size());
        } else {
            std::printf("unknown command\n");
        }
    }
    {
        std::lock_guard<std::mutex> lock(reg.mu);
        for (const g::Entry& e : reg.live) std::free(base_of(e));
        reg.live.clear();
    }
    return 0;
}
