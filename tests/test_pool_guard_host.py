"""The pure part of the guarded allocation mode, on the host: alpha_omok_amd/csrc/pool_guard.hpp -- compiled into a stand-alone
program (tests/host/pool_guard_main.cpp) with the host C++ compiler, once plainly and once under AddressSanitizer and
UndefinedBehaviorSanitizer -- driven on plain host memory: the rounding of AO_POOL_GUARD, the layout, where damage is found
and how it is reported. No GPU."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "alpha_omok_amd", "csrc")
MAIN = os.path.join(REPO, "tests", "host", "pool_guard_main.cpp")
REPORT = re.compile(r"block #(\d+) \((\d+) B, device (\d+)\): (\d+) damaged bytes?, first at (start-|end\+)(\d+), found 0x([0-9a-f]{2}) "
                    r"\(fill 0x([0-9a-f]{2})\)( \[found when freed\])?$")


def parse_report(line):
    """One line of a damage report -> dict(ordinal, bytes, device, count, side, offset, value, fill, freed). The GPU tests
    read ao_guard_check's message with it."""
    m = REPORT.match(line)
    assert m, line
    return dict(ordinal=int(m.group(1)), bytes=int(m.group(2)), device=int(m.group(3)), count=int(m.group(4)),
                side="start" if m.group(5) == "start-" else "end", offset=int(m.group(6)), value=int(m.group(7), 16),
                fill=int(m.group(8), 16), freed=m.group(9) is not None)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def program(request, tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler on this machine")
    exe = str(tmp_path_factory.mktemp("pool_guard") / ("pool_guard_" + request.param))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall"] + flags + ["-I", CSRC, MAIN, "-o", exe, "-lpthread"], check=True)

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stderr   # a sanitizer finding ends the program with its report on stderr
        out = r.stdout.splitlines()
        assert len(out) == len(lines), r.stdout
        return out
    return run


def check_line(line):
    head, text = line.split("|", 1)
    assert "OVERRUN" not in head, line
    blocks, damaged, length = map(int, head.split())
    assert length == len(text)
    return blocks, damaged, text.split(";") if text else []


def test_rounding_of_the_guard_size(program):
    texts = ["-", "0", "1", "4095", "4096", "4097", "262144", "262145", "-5", "junk", "8192k"]
    want = [0, 0, 4096, 4096, 4096, 8192, 262144, 266240, 0, 0, 8192]
    assert [int(x) for x in program(["round " + t for t in texts])] == want


def test_fill_byte(program):
    texts = ["-", "0", "90", "0x5A", "255", "256", "-1", "junk"]
    assert [int(x) for x in program(["fill " + t for t in texts])] == [255, 0, 90, 0x5A, 255, 255, 255, 255]


def test_layout(program):
    out = program(["layout 1000 4096", "layout 0 8192", "layout 17 4096"])
    assert [tuple(map(int, o.split())) for o in out] == [(9192, 4096, 5096), (16384, 8192, 8192), (8209, 4096, 4113)]
    for total, body, rear in (tuple(map(int, o.split())) for o in out):
        assert body % 4096 == 0   # the body stays as aligned as the base


def test_a_clean_block_and_its_fill(program):
    out = program(["new 1000 4096 255", "new 0 4096 90", "body 0", "body 1", "live", "check 512", "poke 0 0 7", "poke 0 999 7", "body 0",
                   "check 512"])
    assert out[:5] == ["0", "1", "0", "0", "2"]
    assert check_line(out[5]) == (2, 0, [])
    assert out[8] == "2"                          # writes inside the body are the owner's business:
    assert check_line(out[9]) == (2, 0, [])       # no guard is damaged


@pytest.mark.parametrize("bytes_", [1000, 1, 16, 4099])
def test_damage_at_the_first_and_last_byte_of_each_guard(program, bytes_):
    G = 4096
    places = [(-G, "start", G), (-1, "start", 1), (bytes_, "end", 0), (bytes_ + G - 1, "end", G - 1)]
    for off, side, k in places:
        out = program(["new 64 4096 255", "new %d %d 90" % (bytes_, G), "poke 1 %d 165" % off, "check 512", "check 512"])
        assert out[2] == "ok"
        blocks, damaged, lines = check_line(out[3])
        assert (blocks, damaged, len(lines)) == (2, 1, 1)
        r = parse_report(lines[0])
        assert r == dict(ordinal=1, bytes=bytes_, device=0, count=1, side=side, offset=k, value=165, fill=90, freed=False)
        assert check_line(out[4]) == (2, 0, [])   # reported once: the guard was repaired
    # one byte further on either side is outside the allocation: the driver refuses it, nothing is written
    out = program(["new %d %d 90" % (bytes_, G), "poke 0 %d 1" % (-G - 1), "poke 0 %d 1" % (bytes_ + G), "check 512"])
    assert out[1] == out[2] == "outside the allocation" and check_line(out[3]) == (1, 0, [])


def test_a_byte_equal_to_the_fill_is_no_damage_and_counts_add_up(program):
    out = program(["new 100 4096 90", "poke 0 -3 90", "check 512", "poke 0 -3 1", "poke 0 -2 2", "poke 0 100 3", "check 512"])
    assert check_line(out[2]) == (1, 0, [])
    _, damaged, lines = check_line(out[6])
    assert damaged == 1
    r = parse_report(lines[0])
    assert (r["count"], r["side"], r["offset"], r["value"]) == (3, "start", 3, 1)   # the lowest address is the first


def test_several_damaged_blocks_sticky_ones_first(program):
    cmds = ["new %d 4096 255" % (10 + i) for i in range(12)]
    cmds += ["poke %d %d 0" % (i, 10 + i) for i in range(12)]   # the first byte after each block
    cmds += ["free 3", "live", "check 4096", "check 4096"]
    out = program(cmds)
    assert out[24:26] == ["ok", "11"]
    blocks, damaged, lines = check_line(out[26])
    assert (blocks, damaged) == (11, 12)
    assert len(lines) == 9 and lines[8] == "... and 4 more"           # the first eight are described
    first = parse_report(lines[0])
    assert first["ordinal"] == 3 and first["freed"] and first["bytes"] == 13   # found at free time, kept, reported first
    rest = [parse_report(x) for x in lines[1:8]]
    assert [r["ordinal"] for r in rest] == [0, 1, 2, 4, 5, 6, 7]
    assert all(r["side"] == "end" and r["offset"] == 0 and r["value"] == 0 and r["count"] == 1 and not r["freed"] for r in rest)
    assert check_line(out[27]) == (11, 0, [])                            # the sticky one is reported once


def test_the_message_is_cut_to_cap(program):
    base = ["new 100 4096 255", "poke 0 100 1"]
    full = check_line(program(base + ["check 512"])[2])[2][0]
    for cap in (1, 2, 10, len(full), len(full) + 1):
        blocks, damaged, lines = check_line(program(base + ["check %d" % cap])[2])
        assert (blocks, damaged) == (1, 1)             # the counts do not depend on the room for the text
        text = lines[0] if lines else ""
        assert text == full[:cap - 1]
    assert check_line(program(base + ["check 0"])[2]) == (1, 1, [])


def test_ordinals_count_allocations_not_live_blocks(program):
    out = program(["new 8 4096 255", "new 8 4096 255", "free 0", "new 8 4096 255", "live", "poke 1 8 9", "check 512"])
    assert out[:5] == ["0", "1", "ok", "2", "2"]
    assert parse_report(check_line(out[6])[2][0])["ordinal"] == 2


def test_library_entry_points_without_a_device(monkeypatch):
    """ao_guard_mode reads the environment at every call; with no guarded block alive ao_guard_check and ao_guard_block touch
    no device."""
    from alpha_omok_amd import engine
    monkeypatch.delenv("AO_POOL_GUARD", raising=False)
    monkeypatch.delenv("AO_POOL_FILL", raising=False)
    assert engine.guard_mode() == (0, 255)
    monkeypatch.setenv("AO_POOL_GUARD", "4097")
    monkeypatch.setenv("AO_POOL_FILL", "0x5A")
    assert engine.guard_mode() == (8192, 0x5A)
    monkeypatch.setenv("AO_POOL_GUARD", "0")
    assert engine.guard_mode() == (0, 0x5A)
    import torch
    if not torch.cuda.is_available():
        assert engine.guard_check() == (0, 0, "")
        assert engine.guard_block(0) is None and engine.guard_block(-1) is None
