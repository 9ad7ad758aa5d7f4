"""CPU-only tests of the host rule of chemlab_amd/csrc/chem_launch_host.hpp: which force kernel a launch gets -- family, MODE,
lanes per particle, block size, ENERGY, DIAG / CUBIC -- or the refusal it gets instead, and which bonded kernel follows.
(CtxT::launch_pair, CtxT::set_tile_lds_attr and CtxT::compute_forces turn the answer into an instantiation; on the device
tests/test_gpu_launch_variants.py runs the variants.)  The rule is compared with a model written here from the list of what the
library builds, over every combination of the inputs.  The harness is compiled with g++ from tests/host/."""
import itertools
import os
import subprocess

import pytest

import helpers as H

EINVAL, ENOTIMPL = -1, -5
TPPS = (0, 1, 2, 4, 8, 16, 32, 64)
BLOCKS = (256, 512, 1024)
SIZES = (100, 7999, 8000, 99999, 100000, 1000000)
FEATURE = {"coul": "with a Coulomb pair registered", "res": "with a resolution pair marked", "cap": "with a capped pair registered"}
KERNEL = {"coul": "with the Coulomb term", "res": "with the resolution scaling", "cap": "with capped pairs"}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(tmp_path_factory.mktemp("host")), "launch_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", os.path.join(root, "tests", "host", "launch_harness.cpp"), "-o", exe])
    return exe


def plan_line(use_tiles=1, n=4000, opt_tpp=0, pair_bs=512, energy=0, coul=0, res=0, cap=0, lj_only=0, uniform_lj=0, cubic_tab=0, diag=0,
              res_pair=(2, 5), cap_pair=(1, 3)):
    return "plan " + " ".join("%d" % v for v in (use_tiles, n, opt_tpp, pair_bs, energy, coul, res, cap, lj_only, uniform_lj, cubic_tab, diag,
                                                 res_pair[0], res_pair[1], cap_pair[0], cap_pair[1]))


def answers(harness, lines):
    """("ok", family, mode, tpp, block, energy, diag, cubic, member) or ("refuse", code, text) per line."""
    out = []
    for w in H.run_harness(harness, lines):
        out.append(("refuse", int(w[1]), " ".join(w[2:])) if w[0] == "refuse" else ("ok", w[1]) + tuple(int(x) for x in w[2:]))
    return out


# ---- what the library builds, written out ------------------------------------------------------------------------------------
def tiles_built():
    s = set()
    for mode in (0, 1, 2, 3):
        for tpp, block in itertools.product((1, 2, 4, 8), BLOCKS):
            s.add((mode, tpp, block, 0, 0))
            if mode in (0, 3):
                s.add((mode, tpp, block, 1, 0))             # ENERGY: the general kernels only
        s.add((mode, 1, 512, 0, 1))                         # DIAG: one lane, 512 threads, forces only
    for mode in (4, 5, 6, 7):
        s |= {(mode, 1, 512, 0, 0), (mode, 1, 512, 1, 0)}
    return s


def rows_built():
    return {(0, tpp, c) for tpp in (1, 2, 4, 8, 16, 32, 64) for c in (0, 1)} | {(4, 4, 1), (5, 4, 0), (6, 4, 0), (7, 4, 0)}


def model(use_tiles, n, opt_tpp, pair_bs, energy, coul, res, cap, lj_only, uniform_lj, cubic_tab, diag, res_pair, cap_pair):
    """The rule as DESIGN.md and include/chem_mi355.h state it: features first, in the order Coulomb, resolution, caps."""
    for f, on in (("coul", coul), ("res", res), ("cap", cap)):
        if not on:
            continue
        if f == "res" and coul:
            return ("refuse", ENOTIMPL, "resolution-scaled type pair (%d,%d) next to a registered Coulomb pair: the two terms are not served in one context"
                    % (min(res_pair), max(res_pair)))
        if f == "cap" and coul:
            return ("refuse", ENOTIMPL, "capped type pair (%d,%d) next to a registered Coulomb pair: the two terms are not served in one context" % cap_pair)
        if opt_tpp > 1:
            return ("refuse", EINVAL, "option tpp = %d: %s only tpp = 1 (or 0, automatic) is built" % (opt_tpp, FEATURE[f]))
        if pair_bs != 512:
            return ("refuse", EINVAL, "option pair_block = %d: %s only pair_block = 512 is built" % (pair_bs, FEATURE[f]))
    feature_mode = 4 if coul else (7 if res and cap else 5 if res else 6 if cap else None)
    if not use_tiles:                                       # rows: 256 threads, the diagnostics options are not looked at
        if feature_mode:
            return ("ok", "r", feature_mode, 4, 256, energy, 0, 1 if coul else 0)
        tpp = opt_tpp if opt_tpp else (4 if n >= 100000 else 8 if n >= 8000 else 16)
        return ("ok", "r", 0, tpp, 256, energy, 0, cubic_tab)
    if feature_mode:
        if diag:
            return ("refuse", EINVAL, "debug_stamps / ablate are not built for the force kernel " + KERNEL["coul" if coul else "res" if res else "cap"])
        return ("ok", "t", feature_mode, 1, 512, energy, 0, 0)
    tpp = min(opt_tpp, 8) if opt_tpp else 1
    if energy:
        return ("ok", "t", 3 if cubic_tab else 0, tpp, pair_bs, 1, 0, 0)
    mode = 2 if uniform_lj else 1 if lj_only else 3 if cubic_tab else 0
    if diag:
        if tpp != 1 or pair_bs != 512:
            return ("refuse", EINVAL, "debug_stamps / ablate need tpp=1 and pair_block=512")
        return ("ok", "t", mode, 1, 512, 0, 1, 0)
    return ("ok", "t", mode, tpp, pair_bs, 0, 0, 0)


def sweep():
    for use_tiles, energy, coul, res, cap, lj_only, uniform_lj, cubic_tab, diag in itertools.product((0, 1), repeat=9):
        for opt_tpp, pair_bs in itertools.product(TPPS, BLOCKS):
            # (the particle count matters to the rows' automatic lane count alone)
            for n in (SIZES if not use_tiles and opt_tpp == 0 else (4000,)):
                yield dict(use_tiles=use_tiles, n=n, opt_tpp=opt_tpp, pair_bs=pair_bs, energy=energy, coul=coul, res=res, cap=cap, lj_only=lj_only,
                           uniform_lj=uniform_lj, cubic_tab=cubic_tab, diag=diag, res_pair=(5, 2), cap_pair=(1, 3))


@pytest.fixture(scope="module")
def swept(harness):
    cases = list(sweep())
    return cases, answers(harness, [plan_line(**c) for c in cases])


def test_built_sets_are_the_ones_written_out_here(harness):
    out = H.run_harness(harness, ["tiles_built", "tiles_unlaunched", "rows_built"])
    got = [[tuple(int(x) for x in w.split(":")) for w in line[1:]] for line in out]
    assert len(got[0]) == len(set(got[0])) == 84 and set(got[0]) == tiles_built()
    assert len(got[2]) == len(set(got[2])) and set(got[2]) == rows_built()
    # carried along without a launch: ENERGY of MODE 1 and 2, ENERGY of DIAG -- disjoint from the built set
    want = {(m, t, b, 1, 0) for m in (1, 2) for t in (1, 2, 4, 8) for b in BLOCKS} | {(m, 1, 512, 1, 1) for m in (0, 1, 2, 3)}
    assert set(got[1]) == want and not (want & tiles_built())


def test_every_input_gets_the_models_answer_and_a_built_variant(swept):
    cases, got = swept
    assert 5000 < len(cases) < 50000
    tb, rb = tiles_built(), rows_built()
    nok = 0
    for c, g in zip(cases, got):
        assert g[:8] == model(**c)[:8] and (g[0] == "refuse" or len(g) == 9), (c, g, model(**c))
        if g[0] == "ok":
            nok += 1
            _, fam, mode, tpp, block, energy, diag, cubic, member = g
            assert member == 1, (c, g)
            if fam == "t":
                assert (mode, tpp, block, energy, diag) in tb and cubic == 0, (c, g)
            else:
                assert (mode, tpp, cubic) in rb and block == 256 and diag == 0, (c, g)
    assert 1000 < nok < len(cases) - 1000                   # both answers are exercised


def test_every_built_variant_is_reached_by_some_input(swept):
    cases, got = swept
    tiles = {g[2:7] for g in got if g[0] == "ok" and g[1] == "t"}
    rows = {(g[2], g[3], g[7]) for g in got if g[0] == "ok" and g[1] == "r"}
    assert tiles == tiles_built(), sorted(tiles_built() - tiles)
    assert rows == rows_built(), sorted(rows_built() - rows)
    for e in (0, 1):                                        # ... the rows in both ENERGY values
        assert {(g[2], g[3], g[7]) for g in got if g[0] == "ok" and g[1] == "r" and g[5] == e} == rows_built()


def test_lane_count_thresholds(harness):
    got = answers(harness, [plan_line(use_tiles=0, n=n) for n in SIZES] + [plan_line(use_tiles=1, n=n) for n in SIZES] +
                  [plan_line(use_tiles=1, opt_tpp=t) for t in TPPS] + [plan_line(use_tiles=0, opt_tpp=t) for t in TPPS])
    assert [g[3] for g in got[:6]] == [16, 16, 8, 8, 4, 4]
    assert [g[3] for g in got[6:12]] == [1] * 6
    assert [g[3] for g in got[12:20]] == [1, 1, 2, 4, 8, 8, 8, 8]          # tiles: at most 8 lanes
    assert [g[3] for g in got[20:28]] == [16, 1, 2, 4, 8, 16, 32, 64]


@pytest.mark.parametrize("feature", ["coul", "res", "cap"])
def test_option_limits_of_the_feature_kernels(harness, feature):
    on = {feature: 1}
    lines = [plan_line(opt_tpp=2, **on), plan_line(opt_tpp=64, use_tiles=0, energy=1, **on), plan_line(pair_bs=256, **on),
             plan_line(pair_bs=1024, use_tiles=0, **on), plan_line(opt_tpp=4, pair_bs=1024, **on), plan_line(opt_tpp=1, **on), plan_line(**on)]
    got = answers(harness, lines)
    assert got[0] == ("refuse", EINVAL, "option tpp = 2: %s only tpp = 1 (or 0, automatic) is built" % FEATURE[feature])
    assert got[1] == ("refuse", EINVAL, "option tpp = 64: %s only tpp = 1 (or 0, automatic) is built" % FEATURE[feature])
    assert got[2] == ("refuse", EINVAL, "option pair_block = 256: %s only pair_block = 512 is built" % FEATURE[feature])
    assert got[3] == ("refuse", EINVAL, "option pair_block = 1024: %s only pair_block = 512 is built" % FEATURE[feature])
    assert got[4] == ("refuse", EINVAL, "option tpp = 4: %s only tpp = 1 (or 0, automatic) is built" % FEATURE[feature])      # tpp before pair_block
    assert got[5][0] == got[6][0] == "ok"


def test_features_next_to_the_coulomb_term_name_the_pair(harness):
    got = answers(harness, [plan_line(coul=1, res=1, res_pair=(7, 3)), plan_line(coul=1, res=1, res_pair=(3, 7), use_tiles=0, energy=1),
                            plan_line(coul=1, cap=1, cap_pair=(0, 15)), plan_line(coul=1, res=1, cap=1, res_pair=(4, 4), cap_pair=(0, 15))])
    text = "resolution-scaled type pair (%d,%d) next to a registered Coulomb pair: the two terms are not served in one context"
    assert got[0] == got[1] == ("refuse", ENOTIMPL, text % (3, 7))
    assert got[2] == ("refuse", ENOTIMPL, "capped type pair (0,15) next to a registered Coulomb pair: the two terms are not served in one context")
    assert got[3] == ("refuse", ENOTIMPL, text % (4, 4))                    # resolution before caps
    # the pairs as the context finds them: the first type with a mark and its first partner; the first capped pair with a <= b
    m = [0] * 16
    m[9] |= 1 << 12; m[12] |= 1 << 9; m[6] |= 1 << 14; m[14] |= 1 << 6; m[6] |= 1 << 11; m[11] |= 1 << 6
    out = H.run_harness(harness, ["respair " + " ".join("%d" % v for v in m), "respair " + " ".join(["0"] * 15 + ["%d" % (1 << 15)]),
                                  "cappair 4 9 2 2 9 5 5 3 12", "cappair 2 15 0 0 15", "cappair 1 7 7"])
    assert [tuple(int(x) for x in w[1:]) for w in out] == [(6, 11), (15, 15), (2, 9), (0, 15), (7, 7)]


def test_diagnostics_refusals_and_precedence(harness):
    got = answers(harness, [
        plan_line(coul=1, diag=1), plan_line(res=1, diag=1), plan_line(cap=1, diag=1), plan_line(res=1, cap=1, diag=1),
        plan_line(diag=1, opt_tpp=2), plan_line(diag=1, pair_bs=256), plan_line(diag=1, pair_bs=1024, lj_only=1, uniform_lj=1),
        plan_line(diag=1), plan_line(diag=1, opt_tpp=1, uniform_lj=1, lj_only=1),
        plan_line(diag=1, opt_tpp=2, pair_bs=256, energy=1), plan_line(diag=1, use_tiles=0, opt_tpp=2),          # never on the ENERGY launch of MODE 0..3, never on rows
        plan_line(coul=1, diag=1, use_tiles=0), plan_line(cap=1, diag=1, use_tiles=0, energy=1),
        plan_line(coul=1, diag=1, opt_tpp=2), plan_line(cap=1, diag=1, pair_bs=256), plan_line(coul=1, res=1, diag=1, opt_tpp=2),
        plan_line(coul=1, res=1, diag=1), plan_line(coul=1, cap=1, diag=1, cap_pair=(2, 2))])
    not_built = "debug_stamps / ablate are not built for the force kernel "
    assert got[0] == ("refuse", EINVAL, not_built + "with the Coulomb term")
    assert got[1] == got[3] == ("refuse", EINVAL, not_built + "with the resolution scaling")
    assert got[2] == ("refuse", EINVAL, not_built + "with capped pairs")
    assert got[4] == got[5] == got[6] == ("refuse", EINVAL, "debug_stamps / ablate need tpp=1 and pair_block=512")
    assert got[7] == ("ok", "t", 0, 1, 512, 0, 1, 0, 1) and got[8] == ("ok", "t", 2, 1, 512, 0, 1, 0, 1)
    assert got[9] == ("ok", "t", 0, 2, 256, 1, 0, 0, 1) and got[10] == ("ok", "r", 0, 2, 256, 0, 0, 0, 1)
    assert got[11] == ("ok", "r", 4, 4, 256, 0, 0, 1, 1) and got[12] == ("ok", "r", 6, 4, 256, 1, 0, 0, 1)
    # an option limit wins over the diagnostics refusal, the Coulomb limit over "next to Coulomb", that one over the diagnostics
    assert got[13] == ("refuse", EINVAL, "option tpp = 2: with a Coulomb pair registered only tpp = 1 (or 0, automatic) is built")
    assert got[14] == ("refuse", EINVAL, "option pair_block = 256: with a capped pair registered only pair_block = 512 is built")
    assert got[15] == ("refuse", EINVAL, "option tpp = 2: with a Coulomb pair registered only tpp = 1 (or 0, automatic) is built")
    assert got[16][1] == ENOTIMPL and got[16][2].startswith("resolution-scaled type pair (2,5)")
    assert got[17][1] == ENOTIMPL and got[17][2].startswith("capped type pair (2,2)")


# nbent inline excl_over work_list coul14 hybrid bonds_only nb_owner -> launch kind bonds_only inline nown
BONDED = [
    ((0, 0, 0, 1, 1, 1, 1, 50), ("none", "plain", 0, 0, 0)),                 # no bonded entries
    ((0, 0, 0, 0, 0, 0, 0, 0), ("none", "plain", 0, 0, 0)),
    ((900, 1, 0, 1, 0, 0, 1, 300), ("none", "plain", 0, 0, 0)),              # all evaluated by the force kernel
    ((900, 1, 0, 0, 0, 0, 0, 300), ("none", "plain", 0, 0, 0)),
    ((900, 1, 7, 1, 0, 0, 1, 300), ("work", "plain", 1, 1, 7)),              # inline bonds: the owners with too many exclusions only
    ((900, 1, 400, 1, 0, 0, 1, 300), ("work", "plain", 1, 1, 300)),
    ((900, 1, 1 << 40, 1, 0, 0, 0, 300), ("work", "plain", 0, 1, 300)),
    ((900, 0, 0, 1, 0, 0, 0, 300), ("work", "plain", 0, 0, 300)),
    ((900, 0, 7, 1, 0, 0, 1, 300), ("work", "plain", 1, 0, 300)),
    ((900, 0, 0, 1, 0, 1, 0, 300), ("work", "hybrid", 0, 0, 300)),
    ((900, 0, 0, 1, 0, 1, 1, 300), ("work", "hybrid", 1, 0, 300)),
    ((900, 0, 0, 1, 1, 0, 0, 300), ("work", "charged", 0, 0, 300)),
    ((900, 0, 0, 1, 1, 1, 1, 300), ("work", "charged", 1, 0, 300)),          # the charged kernel carries the lambda along
    ((900, 0, 0, 0, 0, 0, 0, 300), ("each", "plain", 0, 0, 0)),
    ((900, 0, 3, 0, 0, 0, 1, 300), ("each", "plain", 0, 0, 0)),              # per particle: one build, no work list
    ((900, 1, 3, 0, 0, 0, 1, 300), ("each", "plain", 0, 0, 0)),
    ((900, 0, 0, 0, 0, 1, 1, 300), ("each", "hybrid", 0, 0, 0)),
    ((900, 0, 0, 0, 1, 0, 0, 300), ("each", "charged", 0, 0, 0)),
    ((900, 0, 0, 0, 1, 1, 0, 300), ("each", "charged", 0, 0, 0)),
    ((1 << 33, 0, 0, 1, 0, 0, 0, 2000000000), ("work", "plain", 0, 0, 2000000000)),
]


def test_bonded_plan_table(harness):
    out = H.run_harness(harness, ["bonded " + " ".join("%d" % v for v in inp) for inp, _ in BONDED])
    for (inp, want), w in zip(BONDED, out):
        assert (w[1], w[2], int(w[3]), int(w[4]), int(w[5])) == want, (inp, w)


def test_bonded_family_rule(harness):
    """bonded_kind on its own (CtxT::observe asks it without a plan): charged if a 1-4 Coulomb list exists, else hybrid."""
    want = {(0, 0): "plain", (0, 1): "hybrid", (1, 0): "charged", (1, 1): "charged"}
    out = H.run_harness(harness, ["kind %d %d" % k for k in want])
    assert [(w[0], w[1]) for w in out] == [("kind", v) for v in want.values()]
