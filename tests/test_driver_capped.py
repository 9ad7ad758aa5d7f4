"""The driver (python -m chemlab_amd.start_simulation) on the fixture tests/golden/capped: a topology shaped like the
polycondensation inputs -- types A, D, E, C; A-D and A-E are nonbond_params func 13 (`table caprad`), E-E a plain table (func 8),
the rest LJ -- and one reaction A + D -> C:E.  The fixture holds settings only; the coordinates (an 8 x 8 x 8 lattice of
alternating A and D) and the two small tables are written here.

CPU: the whole driver runs on the CPU checker, wrapped so that the call the checker does not have (nb_cap) is recorded instead of
refused -- what is checked is the driver's own wiring.  GPU (fp32): the same run on the product engine; bonds form, and the
forces at the final positions equal tests/capped_ref.py on the final types plus the harmonic bonds."""
import os
import shutil

import numpy as np
import pytest

import capped_ref as C
import spline_ref as S
from chemlab_amd import espp, start_simulation
from helpers import force_error_without_cutoff_flips

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NSIDE, BOX = 8, 9.0
A, D, E, CC = 0, 1, 2, 3                # types in the order the topology names them
CAP_AD, CAP_AE, TAB_RC, LJ_RC = 1.12, 1.1, 1.2, 1.5
BOND_K, BOND_R0 = 30.0, 1.0


def soft_table(height):
    """rows r = 0.02 k, k = 1..64: U = height (1 - r / 1.2)^2 inside 1.2, zero beyond; f = -dU/dr"""
    r = 0.02 * np.arange(1, 65)
    q = np.clip(1.0 - r / TAB_RC, 0.0, None)
    return r, height * q * q, 2.0 * height / TAB_RC * q


def stage(tmp_path):
    d = tmp_path / "capped"
    shutil.copytree(os.path.join(GOLD, "capped"), str(d))
    for name, height in (("table_A_D.pot", 20.0), ("table_A_E.pot", 16.0)):
        np.savetxt(d / name, np.stack(soft_table(height), 1), fmt="%.17g")
    rng = np.random.default_rng(5)
    g = np.stack(np.meshgrid(*[np.arange(NSIDE)] * 3, indexing="ij"), -1).reshape(-1, 3)
    a_sites = g[g.sum(1) % 2 == 0]
    lines = ["capped", "%d" % (NSIDE ** 3)]
    for m, s in enumerate(a_sites):                               # molecule m: A on an even site, D on its +x neighbour
        for k, (name, site) in enumerate((("A1", s), ("D1", (s + (1, 0, 0)) % NSIDE))):
            x = (site + 0.5) * (BOX / NSIDE) + rng.uniform(-0.03, 0.03, 3)
            lines.append("%5d%-5s%5s%5d%8.3f%8.3f%8.3f" % (m + 1, "MOL", name, 2 * m + k + 1, x[0], x[1], x[2]))
    lines.append("%10.5f%10.5f%10.5f" % (BOX, BOX, BOX))
    (d / "conf.gro").write_text("\n".join(lines) + "\n")
    return d


def product_factory(prec=32):
    from chemlab_amd.engine import Engine
    return lambda: Engine(device=0, precision=prec)


def test_fixture_holds_settings_only():
    assert sorted(os.listdir(os.path.join(GOLD, "capped"))) == ["params", "reaction.cfg", "topol.top"]


def test_driver_wires_the_caps_on_the_cpu_checker(tmp_path, monkeypatch, oracle_mod):
    rec = []

    class Recording(oracle_mod.OracleEngine):
        """the CPU checker, with the entry point it lacks recorded instead of refused (the cap's physics is not run)"""

        def nb_lj(self, *a, **k):
            rec.append(("nb_lj",) + tuple(a[:5]))
            return super().nb_lj(*a, **k)

        def nb_table(self, *a, **k):
            rec.append(("nb_table", a[0], a[1], a[6]))
            return super().nb_table(*a, **k)

        def nb_cap(self, t1, t2, caprad):
            rec.append(("nb_cap", t1, t2, caprad))

        def reaction_add(self, *a, **k):
            idx = super().reaction_add(*a, **k)
            rec.append(("reaction_add", a, k))
            return idx

    espp.set_engine_factory(lambda: Recording())
    try:
        monkeypatch.chdir(stage(tmp_path))
        res = start_simulation.main(["@params"], quiet=True)
    finally:
        espp.set_engine_factory(product_factory())
    eng = res["system"].engine
    assert eng.n == 512 and eng.step == 60
    key = lambda a, b: (min(a, b), max(a, b))
    assert {key(r[1], r[2]): r[3] for r in rec if r[0] == "nb_cap"} == {(A, D): CAP_AD, (A, E): CAP_AE}
    assert len([r for r in rec if r[0] == "nb_cap"]) == 2
    tabs = {key(r[1], r[2]): r[3] for r in rec if r[0] == "nb_table"}
    assert tabs == {(A, D): TAB_RC, (A, E): TAB_RC, (E, E): TAB_RC}
    for pair in ((A, D), (A, E)):                                  # the table first, then its cap
        first_tab = min(i for i, r in enumerate(rec) if r[0] == "nb_table" and key(r[1], r[2]) == pair)
        first_cap = min(i for i, r in enumerate(rec) if r[0] == "nb_cap" and key(r[1], r[2]) == pair)
        assert first_tab < first_cap
    lj = {key(r[1], r[2]) for r in rec if r[0] == "nb_lj"}
    assert lj == {(A, A), (D, D), (A, CC), (D, E), (D, CC), (E, CC), (CC, CC)}      # every other pair: LJ (rows or the combination rule)
    (ra,) = [r for r in rec if r[0] == "reaction_add"]
    header = open("sim0_energy_12345.csv").readline().strip().split(",")
    assert {"lj", "lj-tab", "lj-tab_cap"} <= set(header)
    assert header.index("lj-tab") < header.index("lj-tab_cap")
    names = [res["system"].getNameOfInteraction(k) for k in range(res["system"].getNumberOfInteractions())]
    inter = res["system"].getInteraction(names.index("lj-tab_cap"))
    assert type(inter) is espp.interaction.VerletListTabulatedCapped
    assert {k: p.caprad for k, p in inter.getAllPotentials().items()} == {(A, D): CAP_AD, (A, E): CAP_AE}
    assert len(eng.get_events()) > 50                              # bonds form on the checker too (under the uncapped tables)


def reference(x, types_, bonds):
    tad, tae = (S.Table(0.02, 0.02, *soft_table(h)[1:], 1) for h in (20.0, 16.0))
    lj11, ljmix, lj98 = S.lj(1.0, 1.0, LJ_RC), S.lj(np.sqrt(0.8), 0.95, LJ_RC), S.lj(0.8, 0.9, LJ_RC)
    matrix = {(A, A): lj11, (D, D): lj11, (A, D): ("tab", tad, TAB_RC), (A, E): ("tab", tae, TAB_RC), (E, E): ("tab", tae, TAB_RC),
              (A, CC): ljmix, (D, E): ljmix, (D, CC): ljmix, (E, CC): lj98, (CC, CC): lj98}
    caps = {(A, D): CAP_AD, (A, E): CAP_AE}
    box = [BOX] * 3
    ref = C.total(x, box, types_, matrix, caps, excluded=bonds)
    plain = C.total(x, box, types_, matrix, {}, excluded=bonds)
    fb, eb = S.bond_terms(np.asarray(x), np.asarray(box), bonds, lambda r: (BOND_K * (r - BOND_R0) ** 2, -2.0 * BOND_K * (r - BOND_R0)))
    return ref, plain, fb, matrix


@pytest.mark.gpu
def test_driver_runs_the_capped_tables_on_the_gpu(tmp_path, monkeypatch):
    espp.set_engine_factory(product_factory(32))
    try:
        monkeypatch.chdir(stage(tmp_path))
        res = start_simulation.main(["@params"], quiet=True)
    finally:
        espp.set_engine_factory(product_factory())
    eng = res["system"].engine
    assert eng.n == 512 and eng.step == 60
    ev = eng.get_events()
    print("%d bond events" % len(ev))
    assert 50 < len(ev) < 256                                      # bonds form, and unreacted A and D remain
    ty = eng.get_state("TYPE")
    want = np.array([A, D] * 256)
    want[ev["id_a"] - 1], want[ev["id_b"] - 1] = CC, E
    assert np.array_equal(ty, want)
    eng.thermostat_langevin(0.3, 0.0, 1)                           # (the force array of a thermostatted step holds the Langevin term too)
    eng.run(0)
    x, f = eng.get_state("POS"), eng.get_state("FORCE")
    bonds = [(int(e["id_a"]) - 1, int(e["id_b"]) - 1) for e in ev]
    ref, plain, fb, matrix = reference(x, ty, bonds)
    p = ref["pairs"]
    inside = p["inside"].astype(bool)
    part = np.abs(ref["F"] - plain["F"]).max() / np.abs(plain["F"] + fb).max()
    print("pairs inside their cap radius: %d A-D, %d A-E; the caps move %.3e of the largest force" %
          ((inside & (ty[p["j"]] + ty[p["i"]] == A + D)).sum(), (inside & (ty[p["j"]] + ty[p["i"]] == A + E)).sum(), part))
    assert (inside & (ty[p["i"]] + ty[p["j"]] == A + D)).sum() >= 5 and (inside & (ty[p["i"]] + ty[p["j"]] == A + E)).sum() >= 5
    assert part > 1e-2
    spec = dict(pos=x, box=[BOX] * 3, types=ty, lj=[(a, b) + m[1:4] for (a, b), m in matrix.items() if m[0] == "lj"],
                tables=[(a, b, m[1].r0, m[1].dr, m[1].e, m[1].f, m[2]) for (a, b), m in matrix.items() if m[0] == "tab"])
    err, flips = force_error_without_cutoff_flips(spec, f, ref["F"] + fb, 2e-5, max_flips=0)
    print("force rel err %.3e flips %d" % (err, flips))
    assert np.isfinite(f).all() and err < 2e-5 and flips == 0
    ob = eng.observe()
    assert ob["epot_tab"] == pytest.approx(ref["e_tab"], rel=1e-5) and ob["epot_lj"] == pytest.approx(ref["e_lj"], rel=1e-5)
