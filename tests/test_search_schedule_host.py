"""The launch schedule of ao_search on the host: alpha_omok_amd/csrc/search_schedule.hpp, compiled into a stand-alone program
(tests/host/search_schedule_main.cpp) with the host C++ compiler and fed cases on stdin. What it prints is compared with the same
formulas written out below in Python -- restated from search_impl as it stood before the header existed (the sit-out window, the
planned extra launches, the catch-up loop's stall rule, the row statistics), not from the header -- and with values worked out
by hand. The spans of the row-counter ring that a harvest reads are restated as the list of words they must cover."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "alpha_omok_amd", "csrc")
MAIN = os.path.join(REPO, "tests", "host", "search_schedule_main.cpp")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler on this machine")
    exe = str(tmp_path_factory.mktemp("search_schedule") / "search_schedule")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", CSRC, MAIN, "-o", exe], check=True)

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return run


# ---- the formulas, restated ----------------------------------------------------------------------------------------------------
def _lround(x):   # C's lround for x >= 0: halves away from zero
    assert x >= 0
    t = math.floor(x)
    return int(t) + (1 if x - t >= 0.5 else 0)


def window(rows, G, cap_rows, ask_frac):
    f = min(1.0, max(0.5, ask_frac))
    slack = 2.5 * math.sqrt(float(cap_rows) * (1.0 - f)) + 4.0
    row_target = int(max(1.0, cap_rows - slack))
    askers = min(float(rows), float(math.floor(row_target / f)))
    sit_idx = _lround((rows - askers) * G / float(rows))
    if sit_idx >= G:
        sit_idx = G - 1
    askers0 = min(float(rows), float(row_target))
    sit0 = _lround((rows - askers0) * G / float(rows))
    if sit0 >= G:
        sit0 = G - 1
    return row_target, sit_idx, sit0


def planned(sims, G, sit_idx):
    return int(math.ceil(float(sims) * G / float(G - sit_idx))) - sims - 8


def catch_up(cap_rows, S, override, window_off, level_budget, script):
    """The catch-up loop over scripted (sum of deficits, largest deficit, any error) readings: per round the launches it runs and
    whether the window is off, 'stop' where the rule ends the loop, 'closed' where the round bound does; and the rounds read."""
    max_rounds = override if override >= 0 else 4 * (S + 2)
    out, last_sum, stalled, rounds = [], -1, 0, 0
    for total, mx, bad in script:
        if rounds >= max_rounds:
            return out + ["closed"], rounds
        rounds += 1
        if mx == 0 or bad:
            return out + ["stop"], rounds
        if total == last_sum and not level_budget:
            if not window_off:
                window_off = True
            else:
                stalled += 1
                if stalled >= 2:
                    return out + ["stop"], rounds
        else:
            stalled = 0
        last_sum = total
        extra = max(mx, (total + cap_rows - 1) // cap_rows)
        if window_off:
            extra = max(extra, 2)
        out.append("%d:%d" % (extra, 1 if window_off else 0))
    if rounds >= max_rounds:
        out.append("closed")
    return out, rounds


def ledger(cap_rows, wants):
    return (len(wants), sum(min(w, cap_rows) for w in wants), cap_rows * len(wants), sum(max(w - cap_rows, 0) for w in wants))


def _c_line(cap_rows, S, override, window_off, level_budget, script):
    return "C %d %d %d %d %d %d " % (cap_rows, S, override, window_off, level_budget, len(script)) + \
        " ".join("%d %d %d" % r for r in script)


def _c_expect(cap_rows, S, override, window_off, level_budget, script):
    out, rounds = catch_up(cap_rows, S, override, bool(window_off), bool(level_budget), script)
    return " ".join(["C"] + out + ["rounds=%d" % rounds])


# ---- the sit-out window ----------------------------------------------------------------------------------------------------------
def test_sit_out_window(program):
    cases = [(5120, 5120, 4096, 0.85), (72, 72, 48, 1.0), (72, 72, 48, 0.3), (72, 72, 71, 0.9), (5120, 5120, 5119, 0.85),
             (2, 2, 1, 1.0), (2, 8192, 1, 0.5), (8192, 8192, 1, 0.7), (24, 24, 16, 1.0), (24, 24, 16, 1.7)]
    rng = np.random.default_rng(20)
    for _ in range(400):
        G = int(rng.integers(2, 8193))
        rows = int(rng.integers(2, G + 1))
        cap = int(rng.integers(1, rows))
        cases.append((rows, G, cap, float(rng.uniform(0.2, 1.3))))
    got = program(["W %d %d %d %s" % (r, G, c, float(f).hex()) for r, G, c, f in cases])
    for (rows, G, cap, frac), line in zip(cases, got):
        assert 1 <= cap < rows <= G <= 8192
        row_target, sit_idx, sit0 = (int(x) for x in line.split()[1:])
        assert (row_target, sit_idx, sit0) == window(rows, G, cap, frac), (rows, G, cap, frac, line)
        assert 1 <= row_target <= cap
        assert 0 <= sit_idx < G and 0 <= sit0 < G
        assert sit0 >= sit_idx          # (the clamp makes the share <= 1: the starting window is never the narrower one)
    # by hand: no terminal leaves -> 4 rows of slack, 44 of 72 games descend; a share below 0.5 counts as 0.5
    assert got[1] == "W 44 28 28"
    assert got[2] == "W 31 10 41" and got[2] == program(["W 72 72 48 %s" % (0.5).hex()])[0]


def test_planned_extra_launches(program):
    cases = [(400, 5120, 1024), (400, 5120, 0), (48, 72, 28), (16, 24, 8), (1, 2, 1), (800, 8192, 8191)]
    rng = np.random.default_rng(21)
    for _ in range(200):
        G = int(rng.integers(2, 8193))
        cases.append((int(rng.integers(1, 1601)), G, int(rng.integers(0, G))))
    got = program(["P %d %d %d" % c for c in cases])
    for c, line in zip(cases, got):
        assert int(line.split()[1]) == planned(*c), (c, line)
    assert got[0] == "P 92"             # 400 * 5120 / 4096 = 500 launches, 100 more than the simulations, 8 short of that
    assert got[1] == "P -8"             # nobody sits out: none (the loop over a negative count runs nothing)


# ---- the catch-up rule -----------------------------------------------------------------------------------------------------------
CATCH_UP = {
    # steady progress ends when nobody is short: max(largest deficit, all deficits / 16 rows) launches per round
    "progress": ((16, 16, -1, 0, 0, [(40, 5, 0), (20, 3, 0), (4, 2, 0), (0, 0, 0)]), "C 5:0 3:0 2:0 stop rounds=4"),
    # an error word ends it at once, whatever the deficits
    "error": ((16, 16, -1, 0, 0, [(40, 5, 1), (20, 3, 0)]), "C stop rounds=1"),
    # a repeated sum: the window goes off and every round runs 2 launches at least; two more repeats are a stall
    "stall": ((16, 16, -1, 0, 0, [(10, 1, 0)] * 6), "C 1:0 2:1 2:1 stop rounds=4"),
    # progress after the window went off: the stall count starts again, the window stays off
    "progress_after_off": ((16, 16, -1, 0, 0, [(10, 1, 0)] * 3 + [(8, 1, 0)] * 3), "C 1:0 2:1 2:1 2:1 2:1 stop rounds=6"),
    # with a level budget a round may pass without a finished simulation: a repeated sum is no stall
    "level_budget": ((16, 16, -1, 0, 1, [(10, 1, 0)] * 5 + [(0, 0, 0)]), "C 1:0 1:0 1:0 1:0 1:0 stop rounds=6"),
    # the window off from the start (AO_CATCHUP_WINDOW_OFF): two repeats are the stall
    "window_off_from_start": ((16, 16, -1, 1, 0, [(10, 1, 0)] * 4), "C 2:1 2:1 stop rounds=3"),
    # an override of 0 rounds (AO_CATCHUP_ROUNDS=0) reads nothing and launches nothing
    "no_rounds": ((16, 16, 0, 0, 0, [(10, 1, 0)]), "C closed rounds=0"),
    "no_rounds_empty": ((16, 16, 0, 0, 0, []), "C closed rounds=0"),
    "two_rounds": ((16, 16, 2, 0, 0, [(40, 5, 0), (30, 5, 0), (20, 5, 0)]), "C 5:0 5:0 closed rounds=2"),
    # large deficits: the rows of a launch bound the progress, ceil(1000 / 16) = 63
    "many_short": ((16, 16, -1, 0, 0, [(1000, 3, 0), (0, 0, 0)]), "C 63:0 stop rounds=2"),
}


@pytest.mark.parametrize("name", sorted(CATCH_UP))
def test_catch_up_rule(program, name):
    args, expect = CATCH_UP[name]
    assert _c_expect(*args) == expect          # the restatement against the hand-written answer
    assert program([_c_line(*args)])[0] == expect


def test_catch_up_round_bound(program):
    """4 (S + 2) rounds at the most, however long progress trickles in."""
    for S in (1, 2, 16):
        script = [(10000 - k, 1, 0) for k in range(4 * (S + 2) + 5)]
        line = program([_c_line(16, S, -1, 0, 0, script)])[0]
        assert line == _c_expect(16, S, -1, 0, 0, script)
        assert line.endswith("closed rounds=%d" % (4 * (S + 2))) and line.count(":0") == 4 * (S + 2)


def test_catch_up_rule_random_scripts(program):
    rng = np.random.default_rng(22)
    lines, expect = [], []
    for _ in range(300):
        cap = int(rng.integers(1, 64))
        script, total = [], int(rng.integers(1, 400))
        for _ in range(int(rng.integers(0, 30))):
            total = max(0, total - int(rng.integers(0, 3)) * int(rng.integers(0, 20)))   # often no progress at all
            script.append((total, 0 if total == 0 else int(rng.integers(1, total + 1)), int(rng.random() < 0.02)))
        args = (cap, int(rng.integers(1, 6)), int(rng.choice([-1, -1, -1, 0, 3])), int(rng.random() < 0.2), int(rng.random() < 0.2), script)
        lines.append(_c_line(*args))
        expect.append(_c_expect(*args))
    assert program(lines) == expect


# ---- the row statistics ----------------------------------------------------------------------------------------------------------
def test_row_ledger(program):
    # 16 rows; launches that asked for 0, 5, 16 (full), 17 and 40 rows: 53 rows did work, 80 were launched, 1 + 24 leaves waited
    assert ledger(16, [0, 5, 16, 17, 40]) == (5, 53, 80, 25)
    assert program(["L 16 5 0 5 16 17 40"])[0] == "L 5 53 80 25"
    assert program(["L 16 0"])[0] == "L 0 0 0 0"
    rng = np.random.default_rng(23)
    cases = [(int(rng.integers(1, 5000)), [int(w) for w in rng.integers(0, 9000, size=int(rng.integers(0, 50)))]) for _ in range(100)]
    cases.append((4096, [2 ** 32 - 1] * 3))   # (a counter word's range)
    got = program(["L %d %d %s" % (cap, len(w), " ".join(map(str, w))) for cap, w in cases])
    for (cap, w), line in zip(cases, got):
        assert tuple(int(x) for x in line.split()[1:]) == ledger(cap, w)


# ---- the spans of the row-counter ring -------------------------------------------------------------------------------------------
def ring_words(harvested, upto, ring):
    """The ring words that hold the counters of the launches [harvested, upto), in launch order: launch i counts in word i % ring."""
    return [i % ring for i in range(harvested, upto)]


def test_ring_spans(program):
    RING = 2048
    by_hand = {
        (0, 0): "R 0 0 0", (700, 700): "R 0 0 0", (700, 650): "R 0 0 0",      # an empty range copies nothing
        (100, 164): "R 100 64 0",                                             # inside the ring: one span
        (2000, 2048): "R 2000 48 0",                                          # ends exactly at the wrap: still one span, no empty tail
        (4000, 4096): "R 1952 96 0",                                          # ... at the second wrap
        (2040, 2060): "R 2040 8 12",                                          # crosses the wrap: the end of the ring, then its start
        (0, 2048): "R 0 2048 0", (2048, 4096): "R 0 2048 0",                  # a full ring from its first word
        (5, 2053): "R 5 2043 5",                                              # a full ring from the middle
    }
    cases = [(h, u, RING) for h, u in by_hand]
    rng = np.random.default_rng(24)
    for _ in range(300):
        ring = int(rng.choice([1, 2, 7, 64, RING]))
        h = int(rng.integers(0, 5 * ring + 1))
        cases.append((h, h + int(rng.integers(0, ring + 1)), ring))
    cases.append((2 ** 33 + 2040, 2 ** 33 + 2060, RING))                      # (launch counts of a long roll are 64-bit)
    got = program(["R %d %d %d" % c for c in cases])
    for (h, u, ring), line in zip(cases, got):
        first, head, tail = (int(x) for x in line.split()[1:])
        assert 0 <= first < ring and head >= 0 and tail >= 0 and first + head <= ring and head + tail <= ring, (h, u, ring, line)
        assert tail == 0 or first + head == ring                              # a second span only behind the ring's end
        assert list(range(first, first + head)) + list(range(tail)) == ring_words(h, u, ring), (h, u, ring, line)
        if (h, u) in by_hand and ring == RING:
            assert line == by_hand[(h, u)], (h, u, line)
    assert got[-1] == "R 2040 8 12"
