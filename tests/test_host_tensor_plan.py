"""CPU-only tests of the host rule of chemlab_amd/csrc/chem_tensor_host.hpp: which pressure-tensor kernel a context gets --
family, MODE, lanes per particle, block size -- or the refusal it gets instead, which is pair_plan's, by name.  The rule is
compared with a restatement written here, over every combination of the inputs.  The harness is compiled with g++ from
tests/host/."""
import itertools
import os
import subprocess

import pytest

import helpers as H

EINVAL, ENOTIMPL = -1, -5
TPPS = (0, 1, 2, 4, 8, 16, 32, 64)
BLOCKS = (256, 512, 1024)
FEATURE = {"coul": "with a Coulomb pair registered", "res": "with a resolution pair marked", "cap": "with a capped pair registered"}
KERNEL = {"coul": "with the Coulomb term", "res": "with the resolution scaling", "cap": "with capped pairs"}
FIELDS = ("use_tiles", "n", "opt_tpp", "pair_bs", "energy", "coul", "res", "cap", "lj_only", "uniform_lj", "cubic_tab", "diag")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(tmp_path_factory.mktemp("host")), "tensor_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", os.path.join(root, "tests", "host", "tensor_harness.cpp"), "-o", exe])
    return exe


def plan_line(c):
    return "plan " + " ".join("%d" % c[k] for k in FIELDS) + " %d %d %d %d" % (c["res_pair"] + c["cap_pair"])


def answers(harness, lines):
    out = []
    for w in H.run_harness(harness, lines):
        out.append(("refuse", int(w[1]), " ".join(w[2:])) if w[0] == "refuse" else ("ok", w[1]) + tuple(int(x) for x in w[2:]))
    return out


def built():
    """What the library builds for the tensor: tiles MODE 3..7 with one lane and 512 threads, rows MODE 0 and 4..7 with four
    lanes and 256 threads."""
    return {("t", m, 1, 512) for m in (3, 4, 5, 6, 7)} | {("r", m, 4, 256) for m in (0, 4, 5, 6, 7)}


def model(c):
    """The rule as include/chem_mi355.h states it: the refusals of the force launch, then the feature decides the MODE; no
    option moves the shape."""
    coul, res, cap = c["coul"], c["res"], c["cap"]
    for f, on in (("coul", coul), ("res", res), ("cap", cap)):
        if not on:
            continue
        if f == "res" and coul:
            return ("refuse", ENOTIMPL, "resolution-scaled type pair (%d,%d) next to a registered Coulomb pair: the two terms are not served in one context"
                    % (min(c["res_pair"]), max(c["res_pair"])))
        if f == "cap" and coul:
            return ("refuse", ENOTIMPL, "capped type pair (%d,%d) next to a registered Coulomb pair: the two terms are not served in one context" % c["cap_pair"])
        if c["opt_tpp"] > 1:
            return ("refuse", EINVAL, "option tpp = %d: %s only tpp = 1 (or 0, automatic) is built" % (c["opt_tpp"], FEATURE[f]))
        if c["pair_bs"] != 512:
            return ("refuse", EINVAL, "option pair_block = %d: %s only pair_block = 512 is built" % (c["pair_bs"], FEATURE[f]))
    feature_mode = 4 if coul else (7 if res and cap else 5 if res else 6 if cap else None)
    if not c["use_tiles"]:
        return ("ok", "r", feature_mode or 0, 4, 256, 1)
    if feature_mode and c["diag"]:
        return ("refuse", EINVAL, "debug_stamps / ablate are not built for the force kernel " + KERNEL["coul" if coul else "res" if res else "cap"])
    return ("ok", "t", feature_mode or 3, 1, 512, 1)


def sweep():
    for use_tiles, energy, coul, res, cap, lj_only, uniform_lj, cubic_tab, diag in itertools.product((0, 1), repeat=9):
        for opt_tpp, pair_bs in itertools.product(TPPS, BLOCKS):
            for n in ((100, 8000, 100000) if not use_tiles and opt_tpp == 0 else (4000,)):
                yield dict(use_tiles=use_tiles, n=n, opt_tpp=opt_tpp, pair_bs=pair_bs, energy=energy, coul=coul, res=res, cap=cap, lj_only=lj_only,
                           uniform_lj=uniform_lj, cubic_tab=cubic_tab, diag=diag, res_pair=(5, 2), cap_pair=(1, 3))


@pytest.fixture(scope="module")
def swept(harness):
    cases = list(sweep())
    return cases, answers(harness, [plan_line(c) for c in cases])


def test_built_set(harness):
    (w,) = H.run_harness(harness, ["built"])
    got = {(s.split(":")[0],) + tuple(int(x) for x in s.split(":")[1:]) for s in w[1:]}
    assert got == built()


def test_plan_matches_the_restatement(swept):
    cases, got = swept
    assert len(cases) > 10000
    for c, g in zip(cases, got):
        assert g == model(c), c


def test_every_answer_is_built_and_every_member_is_answered(swept):
    cases, got = swept
    oks = {g[1:5] for g in got if g[0] == "ok"}
    assert all(g[5] == 1 for g in got if g[0] == "ok")
    assert oks == built()


def test_energy_field_and_shape_options_do_not_move_the_answer(swept):
    """The tensor's variant depends on the family and the registered features alone."""
    cases, got = swept
    seen = {}
    for c, g in zip(cases, got):
        if g[0] != "ok":
            continue
        key = (c["use_tiles"], c["coul"], c["res"], c["cap"])
        assert seen.setdefault(key, g) == g, c
    assert len(seen) == 2 * 5      # (res or cap next to coul is refused)


def test_refusals_are_those_of_the_force_launch(harness, swept):
    """Compiled side by side: every refusal of pair_plan for the ENERGY launch is the tensor's, with the same code and text."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(os.path.dirname(harness), "launch_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", os.path.join(root, "tests", "host", "launch_harness.cpp"), "-o", exe])
    cases, got = swept
    sub = [(c, g) for c, g in zip(cases, got) if c["pair_bs"] != 1024 and c["opt_tpp"] in (0, 1, 4)]
    ref = H.run_harness(exe, [plan_line(dict(c, energy=1)) for c, _ in sub])
    nref = 0
    for (c, g), w in zip(sub, ref):
        assert (w[0] == "refuse") == (g[0] == "refuse"), c
        if w[0] == "refuse":
            nref += 1
            assert (int(w[1]), " ".join(w[2:])) == g[1:], c
    assert nref > 100
