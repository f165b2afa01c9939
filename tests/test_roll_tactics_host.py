"""The host rules of the solver beside the rolling loop: alpha_omok_amd/csrc/roll_schedule.hpp, compiled into a stand-alone
program (tests/host/roll_tactics_main.cpp) with the host C++ compiler and fed cases on stdin, as test_roll_schedule_host.py
does for the roll's own rules. What it prints is compared with the rules restated below from the text of the feature -- a
proven win with solved_sims = k > 0 searches min(budget, k) simulations, everything else its budget; a waiting game is never
turned; a batch's games begin once its event has been reached and it has been held for `hold` further turns beyond the first
later turn, or at once when the host had to wait for it; the host waits when a batch is to be started and every slot is busy,
or when nothing is searching and a batch is pending -- and with cases worked out by hand. Also here: the entry points exist
and the layouts that existing callers rely on are unchanged."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "alpha_omok_amd", "csrc")
MAIN = os.path.join(REPO, "tests", "host", "roll_tactics_main.cpp")
RT_NONE, RT_WIN, RT_DEFEND, RT_LOST = 0, 1, 2, 3
OUT, SEARCHING, WAITING = 0, 1, 2


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    exe = str(tmp_path_factory.mktemp("roll_tactics") / "roll_tactics")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", CSRC, MAIN, "-o", exe], check=True)

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return run


# ---- the rules, restated ---------------------------------------------------------------------------------------------------------
def solved_budget(budget, verdict, k):
    return min(budget, k) if verdict == RT_WIN and k > 0 else budget


def game_turns(state, done, target, idle):
    return state == SEARCHING and bool(idle) and done == target


def batch_begins(done, age, hold, blocked):
    return bool(blocked) or (bool(done) and age >= 1 + hold)


def must_block(busy, slots, starts, searching, pending):
    return (bool(starts) and busy >= slots) or (searching == 0 and pending > 0)


# ---- the budget of a solved game ---------------------------------------------------------------------------------------------------
def test_solved_budget_by_hand(program):
    cases = ["S 40 1 6", "S 4 1 6", "S 6 1 6", "S 40 1 0", "S 40 2 6", "S 40 3 6", "S 40 0 6", "S 1 1 1", "S 40 1 40"]
    want = ["S 6", "S 4", "S 6", "S 40", "S 40", "S 40", "S 40", "S 1", "S 40"]
    assert ["S %d" % solved_budget(*map(int, c.split()[1:])) for c in cases] == want
    assert program(cases) == want


def test_solved_budget_random(program):
    rng = np.random.default_rng(47)
    cases = [(int(rng.integers(1, 401)), int(rng.integers(0, 4)), int(rng.integers(0, 401))) for _ in range(800)]
    got = program(["S %d %d %d" % c for c in cases])
    for c, line in zip(cases, got):
        assert line == "S %d" % solved_budget(*c), c


# ---- a waiting game is never turned ----------------------------------------------------------------------------------------------
def test_waiting_game_never_turns(program):
    cases = [(s, d, t, l) for s in (OUT, SEARCHING, WAITING) for d in (0, 3, 4, 5) for t in (0, 4) for l in (0, 1)]
    got = program(["T %d %d %d %d" % c for c in cases])
    for c, line in zip(cases, got):
        assert line == "T %d" % game_turns(*c), c
        if c[0] == WAITING:
            assert line == "T 0"
    # by hand: the counters a game is left with by the move it just played say "finished and idle"
    assert program(["T 2 4 4 1", "T 1 4 4 1", "T 0 4 4 1", "T 2 0 0 1", "T 1 4 4 0"]) == ["T 0", "T 1", "T 0", "T 0", "T 0"]


# ---- the ring of batches ----------------------------------------------------------------------------------------------------------
def test_when_a_batch_begins_its_games(program):
    cases = [(d, a, h, b) for d in (0, 1) for a in range(5) for h in (0, 1, 2) for b in (0, 1)]
    got = program(["G %d %d %d %d" % c for c in cases])
    for c, line in zip(cases, got):
        assert line == "G %d" % batch_begins(*c), c
    # by hand. No hold: not at the turn that started it (age 0), at the first later turn if the event is reached, never before
    # it is. Hold 2: the first later turn and two more go by. A batch the host waited for begins at once.
    assert program(["G 1 0 0 0", "G 1 1 0 0", "G 0 1 0 0", "G 0 9 0 0"]) == ["G 0", "G 1", "G 0", "G 0"]
    assert program(["G 1 1 2 0", "G 1 2 2 0", "G 1 3 2 0", "G 0 3 2 0"]) == ["G 0", "G 0", "G 1", "G 0"]
    assert program(["G 0 0 2 1", "G 1 0 0 1"]) == ["G 1", "G 1"]


def test_when_the_host_must_wait(program):
    slots = int(program(["N"])[0].split()[1])
    assert slots == 4
    cases = [(b, slots, s, n, b) for b in range(slots + 1) for s in (0, 1) for n in (0, 1, 5)]
    got = program(["K %d %d %d %d %d" % c for c in cases])
    for c, line in zip(cases, got):
        assert line == "K %d" % must_block(*c), c
    # by hand: every slot busy and a batch to start; a free slot; every slot busy but nothing to start while games search;
    # nothing searching and a batch pending; nothing searching and nothing pending
    assert program(["K 4 4 1 3 4", "K 3 4 1 3 3", "K 4 4 0 3 4", "K 1 4 0 0 1", "K 0 4 0 0 0"]) == ["K 1", "K 0", "K 0", "K 1", "K 0"]


# ---- the entry points exist, the layouts stay ------------------------------------------------------------------------------------
def test_roll_tactics_entry_points():
    import inspect

    from alpha_omok_amd import _lib
    from alpha_omok_amd.engine import Engine
    hdr = open(os.path.join(REPO, "include", "omok_hip.h")).read()
    for name in ("ao_roll_set_tactics", "ao_roll_tactics_records", "ao_roll_tactics_stats"):
        assert name in _lib.SYMBOLS, name
        assert "int %s(ao_engine *e" % name in hdr, name
    assert callable(Engine.roll_tactics_stats)
    assert "tactics" in inspect.signature(Engine.roll_begin).parameters
    assert "#define AO_ABI_VERSION 2 " in hdr
    assert [f[0] for f in _lib.AoRollOpts._fields_] == ["active", "tau_plies", "sims", "sims_stride", "noise", "noise_stride", "early_stop",
                                                        "turn_every", "want_visit", "want_policy"]
    assert [f[0] for f in _lib.AoRollRecords._fields_] == ["count", "game", "ply", "action", "win", "tau", "sims", "settled", "pi", "visit", "policy"]


def test_abi_version_of_the_built_library():
    from alpha_omok_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libomok_hip.so is not built")
    assert _lib.load(build_if_missing=False).ao_abi_version() == 2
    assert _lib.load().ao_roll_tactics_stats is not None
