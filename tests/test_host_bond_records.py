"""CPU-only test of the rule that lets inline bonds on (chemlab_amd/csrc/chem_launch_host.hpp, bond_records_fit): a bond record
keeps a partner's LDS slot in 16 bits with 0xffff for "no partner", so a staged tile may hold at most 0xffff slots (numbered
0 .. 0xfffe); beyond that CtxT::bonds_inline() answers no and the bonds go to the work list like those of a particle with more
than eight.  The rule is scanned over the whole range of the capacity (an int in the library).  The harness is compiled with
g++ from tests/host/."""
import os
import subprocess

import pytest

import helpers as H

NONE = 0xffff


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(tmp_path_factory.mktemp("host")), "bond_record_harness")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(root, "tests", "host", "bond_record_harness.cpp"), "-o", exe])
    return exe


def test_the_mark_is_the_largest_16_bit_word(harness):
    assert H.run_harness(harness, ["none"]) == [["none", "%d" % NONE]]


def test_the_answer_changes_twice_over_every_int(harness):
    """false below 0, true for 0 .. 0xffff (the largest slot of such a tile is 0xfffe < the mark), false from 0x10000 on."""
    lo, hi = -2 ** 31, 2 ** 31 - 1
    out = H.run_harness(harness, ["fit %d" % lo, "scan %d %d" % (lo, hi), "fit %d" % hi])
    assert out == [["fit", "0"], ["scan", "2", "0", "%d" % (NONE + 1)], ["fit", "0"]]


def test_capacities_around_the_limit_and_those_in_use(harness):
    caps = [-1, 0, 1, 1024, 10240, NONE - 1, NONE, NONE + 1, 2 * NONE, 2 ** 31 - 1, 2 ** 31, 2 ** 40, -2 ** 40]
    out = H.run_harness(harness, ["fit %d" % c for c in caps])
    assert [int(w[1]) for w in out] == [1 if 0 <= c <= NONE else 0 for c in caps]
    # a tile of `cap` slots numbers them 0 .. cap - 1: where the rule says yes, no slot is the mark
    assert all(c - 1 < NONE for c, w in zip(caps, out) if w[1] == "1")
