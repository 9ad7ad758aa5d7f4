"""CPU-only tests of the spline kinds of the tabulated potentials (Tabulated itype 2 = Akima, 3 = natural cubic spline).

The host fitter (chemlab_amd/csrc/chem_tab_host.hpp: fit_akima, fit_natural_cubic, the two device packings, the argument
check) is compiled into tests/host/table_harness.cpp with g++ and compared with the numpy restatement of the rule set in
tests/spline_ref.py, which in turn is compared with scipy where scipy is installed.  The shim tests drive
Tabulated(itype=2|3) through reaction_parser / SetupReactions up to the engine call."""
import os
import subprocess
import types

import numpy as np
import pytest

import spline_ref as S
from chemlab_amd import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host") / "table_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "host", "table_harness.cpp"), "-o", exe])
    return exe


def run(harness, script):
    return subprocess.run([harness], input="\n".join(script) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")


def nums(v):
    return " ".join("%.17g" % x for x in v)


def fit(harness, y, itype):
    out = run(harness, ["fit %d %d %s" % (itype, len(y), nums(y))])[0].split()
    assert out[0] == "coef" and int(out[1]) == 4 * (len(y) - 1)
    return np.array([float(x) for x in out[2:]]).reshape(-1, 4)


# ---- columns ---------------------------------------------------------------------------------------------------------------

def lj_column(nrow=60, dr=0.05):
    """LJ-shaped force column on a 0.05 grid (r = 0.05 .. 3.0), clipped at +-1e4"""
    r = dr * np.arange(1, nrow + 1)
    return np.clip(24.0 * (2.0 * r ** -12 - r ** -6) / r, -1e4, 1e4)


def flat_ends_column(nrow=1750):
    """the first 20 and the last 20 rows constant (flat head, zero tail): the tie rule of the Akima slopes"""
    x = np.linspace(0.0, 1.0, nrow)
    y = 3.0 * np.cos(7.0 * x) * (1.0 - x) ** 2
    y[:20] = y[19]
    y[-20:] = 0.0
    return y


def columns():
    rng = np.random.default_rng(5)
    _, _, e34, f34 = W.synthetic_table(nrow=34, dr=0.05)
    cols = {"lj": lj_column(), "syn_e": e34, "syn_f": f34, "flat": flat_ends_column()}
    for n in (4, 5, 6, 1750):
        cols["rand%d" % n] = rng.normal(size=n)
    return cols


COLS = columns()


# ---- 1: the fitter against the restatement ------------------------------------------------------------------------------

@pytest.mark.parametrize("itype", [2, 3])
@pytest.mark.parametrize("name", sorted(COLS))
def test_fit_matches_restatement(harness, name, itype):
    y = COLS[name]
    n, scale = len(y), np.abs(y).max()
    c = fit(harness, y, itype)
    want = S.coeffs(y, itype)
    assert np.abs(c - want).max() <= 1e-12 * scale
    assert np.array_equal(c[:, 0], y[:-1])                                    # c0 = y_k: nodes reproduced exactly
    # 10^4 random points: the harness' coefficients evaluated by the restated rule against the restatement's own
    x = np.random.default_rng(1).uniform(-0.7, n - 0.3, 10000)                # (beyond both ends: the clamps)
    assert np.abs(S.evaluate(c, 0.0, 1.0, x) - S.evaluate(want, 0.0, 1.0, x)).max() <= 1e-12 * scale
    assert np.array_equal(S.evaluate(c, 0.0, 1.0, np.arange(n - 1.0)), y[:-1])
    assert np.array_equal(S.evaluate(c, 0.0, 1.0, np.array([-3.0, -1e-9])), y[[0, 0]])
    v = S.evaluate(c, 0.0, 1.0, np.array([n - 1.0, n + 5.0]))                    # beyond the grid: w = 1 in the last interval
    assert v[0] == v[1] and abs(v[0] - y[-1]) <= 1e-10 * scale
    # continuity at the interior nodes: value and first derivative; itype 3: second derivative too, zero at the ends
    assert np.abs(c[:-1].sum(1) - c[1:, 0]).max() <= 1e-10 * scale
    assert np.abs((c[:-1, 1] + 2.0 * c[:-1, 2] + 3.0 * c[:-1, 3]) - c[1:, 1]).max() <= 1e-10 * scale
    if itype == 3:
        assert np.abs((2.0 * c[:-1, 2] + 6.0 * c[:-1, 3]) - 2.0 * c[1:, 2]).max() <= 1e-10 * scale
        assert abs(2.0 * c[0, 2]) <= 1e-10 * scale and abs(2.0 * c[-1, 2] + 6.0 * c[-1, 3]) <= 1e-10 * scale


@pytest.mark.parametrize("itype", [2, 3])
def test_device_packings(harness, itype):
    """pair rows: (f c0..c3)(e c0..c3) per interval; bonded rows: (e c0, f c0) .. (e c3, f c3) -- columns fitted independently"""
    _, _, e, f = W.synthetic_table(nrow=34, dr=0.05)
    ce, cf = fit(harness, e, itype), fit(harness, f, itype)
    out = run(harness, ["pair %d 34 %s %s" % (itype, nums(e), nums(f)), "bond %d 34 %s %s" % (itype, nums(e), nums(f))])
    pair, bond = out[0].split(), out[1].split()
    assert pair[:2] == ["pair", str(8 * 33)] and bond[:2] == ["bond", str(8 * 33)]
    p = np.array([float(x) for x in pair[2:]]).reshape(33, 2, 4)
    b = np.array([float(x) for x in bond[2:]]).reshape(33, 4, 2)
    assert np.array_equal(p[:, 0], cf) and np.array_equal(p[:, 1], ce)
    assert np.array_equal(b[:, :, 0], ce) and np.array_equal(b[:, :, 1], cf)


# ---- 2: the restatement against scipy ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(COLS))
def test_restatement_matches_scipy(name):
    si = pytest.importorskip("scipy.interpolate")
    y = COLS[name]
    n, scale = len(y), np.abs(y).max()
    x = np.arange(n, dtype=np.float64)
    for itype, pp in ((2, si.Akima1DInterpolator(x, y)), (3, si.CubicSpline(x, y, bc_type="natural"))):
        want = pp.c[::-1].T                                                   # scipy: highest power first, per interval
        err = np.abs(S.coeffs(y, itype) - want).max() / scale
        print("%s itype %d: %.2e" % (name, itype, err))
        assert err <= 1e-12


# ---- 3: linear data ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("itype", [2, 3])
@pytest.mark.parametrize("n", [4, 7, 200])
def test_linear_data(harness, n, itype):
    a, b, r0, dr = 1.75, -0.625, 0.3, 0.05
    y = a + b * (r0 + dr * np.arange(n))
    c = fit(harness, y, itype)
    assert np.abs(c[:, 2:]).max() <= 1e-13 and np.abs(c[:, 1] - b * dr).max() <= 1e-13


# ---- 5: what is refused --------------------------------------------------------------------------------------------------------

def test_refused_arguments(harness):
    script = ["ok %d %d" % (it, n) for it in (0, 1, 2, 3, 4) for n in (1, 2, 3, 4)]
    got = [l for l in run(harness, script) if l]
    want = {(1, 2), (1, 3), (1, 4), (2, 4), (3, 4)}
    assert got == ["ok %d" % ((it, n) in want) for it in (0, 1, 2, 3, 4) for n in (1, 2, 3, 4)]
    for itype in (2, 3):
        assert run(harness, ["fit %d 3 1 2 4" % itype])[0] == "coef 0"          # the fitter itself returns nothing below 4 rows


# ---- 4: the shim ---------------------------------------------------------------------------------------------------------------

class StubEngine:
    """records the set-up calls the shim makes"""

    def __init__(self):
        self.calls = []
        self.n = 0

    def list_create(self, arity, kind, by_types=False):
        self.calls.append(("list_create", arity, kind, by_types))
        return len(self.calls)

    def table_create(self, r0, dr, e, f, itype=1):
        self.calls.append(("table_create", r0, dr, len(e), itype))
        return 7

    def nb_table(self, t1, t2, r0, dr, e, f, rc, itype=1):
        self.calls.append(("nb_table", t1, t2, itype))

    def __getattr__(self, name):
        def rec(*a, **k):
            self.calls.append((name, a, k))
            return 0
        return rec


def write_pot(path, nrow=40, r0=0.05, dr=0.05):
    r = r0 + dr * np.arange(nrow)
    np.savetxt(path, np.stack([r, 30.0 * (r - 0.9) ** 2, -60.0 * (r - 0.9)], 1), fmt="%15.8g")
    return str(path)


CFG = """[general]
interval: 5
nearest=1

[group_g1]
potential=Tabulated
potential_options=itype=2,filename=%s

[reaction_a]
reaction: A(0, 1) + B(0, 1) -> A(1):B(1)
cutoff: 0.9
rate: 1.0
intramolecular: False
intraresidual: False
active: True
group: g1
"""


def setup_through_the_parser(tmp_path, engine):
    from chemlab_amd import espp
    from chemlab_amd.chemlab import reaction_parser
    from chemlab_amd.chemlab.reaction_setup import SetupReactions
    pot = write_pot(tmp_path / "table_b6.pot")
    cfg_file = tmp_path / "reaction.cfg"
    cfg_file.write_text(CFG % pot)
    cfg = reaction_parser.parse_config(str(cfg_file))
    assert cfg["reactions"]["g1"]["potential_options"]["itype"] == 2
    old = espp._factory[0]
    espp.set_engine_factory(lambda: engine)
    try:
        system = espp.System()
    finally:
        espp.set_engine_factory(old)
    system.storage = types.SimpleNamespace(system=system)
    topol = types.SimpleNamespace(used_atomsym_atomtype={"A": 0, "B": 1},
                                  gt=types.SimpleNamespace(atomtypes={"A": dict(mass=1.0, charge=0.0), "B": dict(mass=1.0, charge=0.0)}))
    sr = SetupReactions(espp, system, None, topol, None, cfg)
    return sr.setup_reactions()


def test_shim_constructs_and_forwards_itype(tmp_path):
    from chemlab_amd import espp
    pot = write_pot(tmp_path / "t.pot")
    for itype in (2, 3):
        for cls in (espp.interaction.Tabulated, espp.interaction.TabulatedAngular, espp.interaction.TabulatedDihedral):
            assert cls(itype=itype, filename=pot).itype == itype
        with pytest.raises(NotImplementedError):
            espp.interaction.MixedTabulated(itype, pot, pot, mix_value=0.5, cutoff=1.5)
    with pytest.raises(NotImplementedError):
        espp.interaction.Tabulated(itype=4, filename=pot)
    eng = StubEngine()
    ar, fpls = setup_through_the_parser(tmp_path, eng)
    made = [c for c in eng.calls if c[0] == "table_create"]
    assert made == [("table_create", 0.05, pytest.approx(0.05), 40, 2)]
    assert ("list_create", 2, "TABULATED", False) in eng.calls
    assert [c for c in eng.calls if c[0] == "list_set_params"][0][1][1] == [7.0]
    # pair tables: the keyword only where the kind is not linear
    system = fpls[0][2].system
    vl = types.SimpleNamespace(system=system)
    tab = espp.interaction.VerletListTabulated(vl)
    tab.setPotential(0, 1, espp.interaction.Tabulated(itype=3, filename=pot, cutoff=1.5))
    tab.setPotential(1, 1, espp.interaction.Tabulated(itype=1, filename=pot, cutoff=1.5))
    assert [c for c in eng.calls if c[0] == "nb_table"] == [("nb_table", 0, 1, 3), ("nb_table", 1, 1, 1)]


def test_spline_tables_are_refused_on_the_cpu_checker(tmp_path, make_oracle):
    """OracleEngine interpolates linearly only: the same set-up raises instead of running with linear tables."""
    from chemlab_amd import espp
    o = make_oracle()
    with pytest.raises(NotImplementedError, match="linear tables"):
        setup_through_the_parser(tmp_path, o)
    pot = espp.interaction.Tabulated(itype=3, filename=write_pot(tmp_path / "t.pot"), cutoff=1.5)
    with pytest.raises(NotImplementedError, match="linear tables"):
        o.nb_table(0, 0, pot.r0, pot.dr, pot.e, pot.f, 1.5, itype=3)
    o.nb_table(0, 0, pot.r0, pot.dr, pot.e, pot.f, 1.5)                      # linear tables as before
    assert o.table_create(pot.r0, pot.dr, pot.e, pot.f, itype=1) == 0


def test_workloads_apply_takes_an_eighth_element():
    eng = StubEngine()
    r0, dr, e, f = W.synthetic_table(nrow=34, dr=0.05)
    spec = dict(box=[9.0] * 3, rc=1.5, skin=0.3, dt=0.002, ids=[1], types=[0], pos=[[1.0, 1.0, 1.0]], mass=[1.0],
                tables=[(0, 0, r0, dr, e, f, 1.5), (0, 1, r0, dr, e, f, 1.5, 2), (1, 1, r0, dr, e, f, 1.5, 1)])
    W.apply(spec, eng, thermostat=False, reactions=False)
    assert [c for c in eng.calls if c[0] == "nb_table"] == [("nb_table", 0, 0, 1), ("nb_table", 0, 1, 2), ("nb_table", 1, 1, 1)]
