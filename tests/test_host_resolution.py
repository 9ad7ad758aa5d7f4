"""Per-particle resolution lambda (include/chem_mi355.h, chem_nb_resolution ff.), host side: the pure routines of
chemlab_amd/csrc/chem_res_host.hpp against the plain-Python rule set of tests/dynres_ref.py (lambda(s), s_full, re-stamping,
the pieces of a run), the reference's forces against its own energy by finite differences, the bindings and the CPU
checker's refusals.  Nothing here needs a GPU.  The harness is compiled with g++ from tests/host/, once more with
-fsanitize=address,undefined."""
import os
import subprocess

import numpy as np
import pytest

import dynres_ref as D
import spline_ref as S
from chemlab_amd import _capi
from chemlab_amd import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include")] + flags +
                          [os.path.join(ROOT, "tests", "host", "resolution_harness.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if request.param == "plain":
        return build(tmp_path_factory.mktemp("host"), "resolution_harness", ["-O1"])
    return build(tmp_path_factory.mktemp("host_san"), "resolution_harness_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def drive(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return out.stdout.split("\n")


# rates that are exact binary fractions and rates that are not (1e-5 from 1e-9: the dacron example's values)
CASES = [(0.0, 0, 1 / 8), (0.0, 0, 1 / 16), (0.5, 3, 1 / 16), (0.25, 7, 1 / 8), (1e-9, 0, 1e-5), (1e-9, 12345, 1e-5), (0.3, 5, 0.1), (0.0, 0, 1 / 3),
         (0.999999, 2, 1e-7), (1.0, 4, 1 / 8), (0.2, 0, 0.0), (0.0, 10, 0.7), (1e-9, 0, 1e-3)]


def test_lambda_of_the_step_is_bit_equal(harness):
    lines, want = [], []
    for l0, s0, a in CASES:
        f = D.s_full(l0, s0, a)
        steps = {s0, s0 + 1, s0 + 7, s0 + 40, s0 + 1000}
        if f is not None:
            steps |= {max(s0, f - 1), f, f + 1, f + 5}
        for s in sorted(steps):
            lines.append("lam %r %d %r %d" % (l0, s0, a, s)); want.append(D.lam(l0, s0, a, s))
    got = [float(x.split()[1]) for x in drive(harness, lines) if x.startswith("lam")]
    assert got == want
    assert any(0.0 < w < 1.0 for w in want) and any(w == 1.0 for w in want)


def test_completion_step(harness):
    got = [int(x.split()[1]) for x in drive(harness, ["full %r %d %r" % c for c in CASES]) if x.startswith("full")]
    want = [D.s_full(*c) for c in CASES]
    assert got == [-1 if w is None else w for w in want]
    # known answers: 1/8 from 0 takes 8 steps, 1/16 from 0.5 eight; 1e-5 from 1e-9 one step more than 1e5
    assert D.s_full(0.0, 0, 1 / 8) == 8 and D.s_full(0.5, 3, 1 / 16) == 11 and D.s_full(1e-9, 0, 1e-5) == 100000
    for l0, s0, a in CASES:                                      # the definition: first step at which the expression is >= 1
        f = D.s_full(l0, s0, a)
        if f is not None and f > s0:
            assert D.lam(l0, s0, a, f) == 1.0 and D.lam(l0, s0, a, f - 1) < 1.0


def script_and_model(types, ops):
    """ops: ('setlam', i, v, s) | ('settype', i, t, s) | ('rate', t, alpha, s, new_type | None) | ('get', s) | ('next', s)
    | ('run', step, nsteps).  Returns the harness lines and what the plain-Python model expects them to print."""
    m = D.Stamps(types)
    lines, want = ["n %d %s" % (len(types), " ".join(str(t) for t in types))], []
    for op in ops:
        if op[0] == "setlam":
            lines.append("setlam %d %r %d" % op[1:]); m.set_lambda(*op[1:])
        elif op[0] == "settype":
            lines.append("settype %d %d %d" % op[1:]); m.set_type(*op[1:]); want.append("changed 1")
        elif op[0] == "rate":
            lines.append("rate %d %r %d %d" % (op[1], op[2], op[3], -1 if op[4] is None else op[4])); m.set_rate(op[1], op[2], op[3], op[4])
        elif op[0] == "get":
            lines.append("get %d" % op[1]); want.append("get")
            want += ["%.17g %d %d %.17g" % (m.st[i][0], m.st[i][1], m.types[i], m.lam(i, op[1])) for i in range(len(types))]
        elif op[0] == "next":
            lines.append("next %d" % op[1])
            fs = [f for f in (m.full(i) for i in range(len(types))) if f is not None and f > op[1]]
            want.append("next %d" % (min(fs) if fs else -1))
        elif op[0] == "run":
            lines.append("run %d %d" % op[1:])
            step, left, pcs, done = op[1], op[2], [], []
            while left > 0:                                       # the model: cut at the earliest pending s_full, complete, go on
                fs = [f for f in (m.full(i) for i in range(len(types))) if f is not None and step < f < step + left]
                ln = (min(fs) - step) if fs else left
                pcs.append(ln); step += ln; left -= ln
                c = m.complete(step)
                if c:
                    done.append("done %d %s" % (step, " ".join(str(i) for i in c)))
            want += [" ".join(["run"] + [str(p) for p in pcs])] + done
    return lines, want


def test_restamping_on_type_and_rate_changes(harness):
    types = [0, 0, 2, 2, 1, 0]
    ops = [("rate", 0, 1 / 16, 0, None), ("setlam", 0, 0.0, 0), ("setlam", 1, 0.5, 0), ("setlam", 2, 0.25, 0), ("setlam", 5, 1e-9, 0),
           ("get", 0), ("get", 4), ("settype", 0, 1, 4), ("get", 4), ("get", 20),           # type 1 has no rate: particle 0 stays at 4/16
           ("rate", 1, 1e-5, 6, None), ("get", 6), ("get", 1000),                              # ... and now creeps on from there
           ("settype", 2, 0, 9), ("get", 9), ("get", 15), ("get", 30),                         # 0.25 frozen under type 2, ramps as type 0
           ("rate", 0, 1 / 8, 10, None), ("get", 10), ("get", 12), ("get", 100),               # the rate of a type changes mid-ramp
           ("rate", 0, 0.0, 12, None), ("get", 50)]                                           # removed: everything of type 0 freezes
    lines, want = script_and_model(types, ops)
    got = [x for x in drive(harness, lines) if x]
    assert got == want


def test_run_pieces_and_completions(harness):
    types = [2, 2, 2, 0, 1, 2]
    ops = [("rate", 2, 1 / 8, 0, 1), ("rate", 0, 1 / 16, 0, None), ("setlam", 0, 0.0, 0), ("setlam", 1, 0.5, 0), ("setlam", 3, 0.0, 0),
           ("next", 0), ("run", 0, 2), ("setlam", 5, 0.0, 2), ("run", 2, 1), ("next", 3), ("run", 3, 1), ("get", 4), ("run", 4, 10), ("get", 14), ("next", 14), ("run", 14, 5), ("run", 19, 0)]
    lines, want = script_and_model(types, ops)
    got = [x for x in drive(harness, lines) if x]
    assert got == want
    assert "done 4 1" in want and "done 8 0" in want and "done 10 5" in want     # 0.5 + 4/8; 8/8; stamped at step 2: 2 + 8
    assert "run 4 2 4" in want                                                     # run(10) from 4 cuts at 8 and 10


# ---- the reference itself: forces = -grad E at fixed lambda, cap off ----------------------------------------------------------

def small_system(seed=3, n=40, L=4.0):
    rng = np.random.default_rng(seed)
    k = int(np.ceil(n ** (1 / 3)))
    g = np.stack(np.meshgrid(*[np.arange(k)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n]
    pos = g * (L / k) + rng.uniform(-0.1, 0.1, (n, 3))
    types = rng.integers(0, 3, n)
    lam = np.where(rng.random(n) < 0.2, 0.0, np.where(rng.random(n) < 0.5, 1.0, rng.uniform(0.05, 0.95, n)))
    r = 0.5 + 0.01 * np.arange(151)
    tab = S.Table(0.5, 0.01, 4.0 * (r ** -12 - r ** -6), 24.0 * (2.0 * r ** -13 - r ** -7), 3)
    matrix = {(0, 0): S.lj(1.0, 0.9, 1.5), (0, 1): S.lj(1.0, 0.8, 1.5), (0, 2): S.lj(0.7, 0.85, 1.4), (1, 1): ("tab", tab, 1.5)}
    return pos, np.array([L, L, L]), types, lam, matrix


def test_reference_forces_are_the_gradient_of_its_energy():
    """LJ pairs only in the derivative check of the marked set (the table's force column is interpolated on its own, not derived
    from its energy column, so the 1-1 table is left out of the matrix here); cap off: the cap is not conservative"""
    pos, box, types, lam, matrix = small_system()
    matrix = {k: v for k, v in matrix.items() if v[0] == "lj"}
    marked = {(0, 0): 0.0, (0, 2): 0.0}
    ref = D.total(pos, box, types, lam, matrix, marked)
    plain = D.total(pos, box, types, np.ones(len(pos)), matrix, marked)
    assert np.abs(ref["F"] - plain["F"]).max() > 1e-2 * np.abs(plain["F"]).max()
    h, worst = 1e-6, 0.0
    for i in range(0, len(pos), 3):
        for c in range(3):
            xp, xm = pos.copy(), pos.copy()
            xp[i, c] += h; xm[i, c] -= h
            fd = -(D.energy(xp, box, types, lam, matrix, marked) - D.energy(xm, box, types, lam, matrix, marked)) / (2.0 * h)
            worst = max(worst, abs(fd - ref["F"][i, c]))
    print("largest | finite difference - force |: %.3e of %.3e" % (worst, np.abs(ref["F"]).max()))
    assert worst < 1e-6 * np.abs(ref["F"]).max()                   # O(h^2 F''') = 1e-12 * 1e3 relative, plus rounding of E / h


def test_reference_limits():
    """lambda = 1 everywhere is the unscaled sum of spline_ref; a cap leaves direction and energy alone"""
    pos, box, types, lam, matrix = small_system()
    marked = {(0, 0): 0.0, (1, 1): 0.0, (0, 2): 0.0}
    one = D.total(pos, box, types, np.ones(len(pos)), matrix, marked)
    F, e_lj, e_tab = S.pair_sums(pos, box, types, matrix)
    assert np.allclose(one["F"], F, rtol=0, atol=1e-12 * np.abs(F).max()) and one["e_lj"] == pytest.approx(e_lj, rel=1e-13) and one["e_tab"] == pytest.approx(e_tab, rel=1e-13)
    free = D.total(pos, box, types, lam, matrix, marked)
    p = free["pairs"]
    m02 = p["marked"] & (p["cap"] == 0.0) & (p["w"] != 0.0)
    cap = float(np.median((np.abs(p["fs"]) * np.sqrt(p["r2"]))[m02]))
    capd = D.total(pos, box, types, lam, matrix, {(0, 2): cap, (0, 0): cap, (1, 1): cap})
    q = capd["pairs"]
    assert 0.25 <= q["capped"][m02].mean() <= 0.75
    assert np.abs(q["fs"] * np.sqrt(q["r2"]))[q["marked"]].max() <= cap * (1 + 1e-12)      # (the unmarked 0-1 pairs know no cap)
    assert np.abs(q["fs"] * np.sqrt(q["r2"]))[~q["marked"]].max() > cap
    assert np.all(np.sign(q["fs"]) == np.sign(p["fs"]))
    assert capd["e_lj"] == free["e_lj"] and capd["e_tab"] == free["e_tab"]


# ---- bindings and the CPU checker ---------------------------------------------------------------------------------------------

def test_new_symbols_are_declared_and_bound():
    hdr = set(_capi.header_symbols())
    for name in ("nb_resolution", "resolution_rate", "set_resolution", "reaction_set_resolution"):
        assert "chem_" + name in hdr and name in _capi.PRODUCT_ONLY
    assert _capi.STATE["LAMBDA"] == 13


class Recorder:
    """an engine that records the calls workloads.apply issues"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def rec(*a, **k):
            self.calls.append((name, a, k))
            return 0
        return rec


def test_workloads_apply_issues_the_resolution_calls():
    spec = dict(box=[4.0] * 3, rc=1.5, skin=0.3, dt=0.001, ids=np.arange(1, 5), types=np.zeros(4, np.int32), pos=np.zeros((4, 3)), mass=np.ones(4),
                lj=[(0, 0, 1.0, 1.0, 1.5)], resolution=[(0, 0, 0.0), (0, 2, 12.5)], res_rates=[(0, 1 / 16), dict(type_id=2, alpha=1 / 8, new_type=1, new_mass=2.0, new_q=0.5)],
                lam=np.array([0.0, 0.5, 1.0, 0.25]))
    r = Recorder()
    W.apply(spec, r, thermostat=False, reactions=False)
    names = [c[0] for c in r.calls]
    assert names.index("nb_lj") < names.index("nb_resolution") < names.index("resolution_rate") < names.index("set_resolution")
    assert [c[1] for c in r.calls if c[0] == "nb_resolution"] == [(0, 0, True, 0.0), (0, 2, True, 12.5)]
    assert [(c[1], c[2]) for c in r.calls if c[0] == "resolution_rate"] == [((0, 1 / 16), {}), ((), dict(type_id=2, alpha=1 / 8, new_type=1, new_mass=2.0, new_q=0.5))]
    (ids, lam), = [c[1] for c in r.calls if c[0] == "set_resolution"]
    assert np.array_equal(ids, spec["ids"]) and np.array_equal(lam, spec["lam"])
    plain = Recorder()
    W.apply({k: v for k, v in spec.items() if k not in ("resolution", "res_rates", "lam")}, plain, thermostat=False, reactions=False)
    assert not [c for c in plain.calls if "resolution" in c[0]]


def test_the_cpu_checker_refuses_every_resolution_call():
    from oracle.oracle import OracleEngine
    o = OracleEngine()
    msg = "resolution: the CPU checker has no per-particle lambda"
    for call in (lambda: o.nb_resolution(0, 0, True, 0.0), lambda: o.resolution_rate(0, 1 / 16), lambda: o.set_resolution([1], [0.5]),
                 lambda: o.reaction_set_resolution(0, 1, 0.0), lambda: o.get_state("LAMBDA"), lambda: o.modify_particle(1, "LAMBDA", 0.5)):
        with pytest.raises(NotImplementedError) as ei:
            call()
        assert str(ei.value) == msg
    spec = dict(box=[4.0] * 3, rc=1.5, skin=0.3, dt=0.001, ids=np.arange(1, 5), types=np.zeros(4, np.int32), pos=np.random.default_rng(0).uniform(0, 4, (4, 3)),
                mass=np.ones(4), lj=[(0, 0, 1.0, 1.0, 1.5)], resolution=[(0, 0, 0.0)])
    with pytest.raises(NotImplementedError):
        W.apply(spec, OracleEngine(), thermostat=False, reactions=False)
