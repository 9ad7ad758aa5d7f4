"""The CPU restatement against the independent reference of tests/bonded_ref.py on the molecule zoo: every bonded kind, typed
lists of arity 2, 3 and 4, the seam of the dihedral, bending angles near straight and folded, bonds near rMax and at the
cutoff, tuples across faces and a corner of three anisotropic boxes.  tests/test_gpu_bonded.py runs the same zoo on the device."""
import numpy as np
import pytest

import bonded_ref as B
import spline_ref as S


@pytest.fixture(scope="module")
def evaluated(oracle_mod):
    """Per box: the zoo, the oracle's answer before and after the type changes, the reference at the oracle's positions."""
    out = {}
    for name in B.BOXES:
        z = B.zoo(name)
        o = oracle_mod.OracleEngine()
        h = B.build(o, z)
        stages = []
        types = z["types"].copy()
        for stage in ("initial", "retyped"):
            if stage == "retyped":
                for pid, ty in z["retype"]:
                    o.modify_particle(pid, "type", ty)
                    types[pid - 1] = ty
            o.run(0)
            x = o.get_state("POS")
            stages.append(dict(f=o.get_state("FORCE"), x=x, obs=o.observe(), types=types.copy(), ref=B.reference(x, z["box"], types, z["lists"], z["mol"])))
        o.close()
        out[name] = (z, h, stages)
    return out


def units(z, pred):
    return [u for u, m in enumerate(z["members"]) if pred(m)]


def test_zoo_has_what_it_promises():
    for name in B.BOXES:
        z = B.zoo(name)
        assert 300 <= z["n"] <= 1500 and len(set(z["box"].tolist())) == 3
        across = B.straddlers(z)
        assert all(len(across[k]) >= 1 for k in (0, 1, 2, "corner")), {k: len(v) for k, v in across.items()}
        kinds = {l["kind"] for l in z["lists"]}
        assert kinds == set(B.ARITY), set(B.ARITY) - kinds
        assert {l["arity"] for l in z["lists"] if l.get("typed")} == {2, 3, 4}
        orders = {}
        for m in z["members"]:
            orders.setdefault(m["name"], set()).add(m["order"])
        assert all(o >= {"ascending", "descending"} and (len(o) == 3 or n.startswith(("fene", "ljb"))) for n, o in orders.items())
        assert set(B.DEGENERATE) <= set(orders)
        # every role of every arity is played, and by ids that are not in chain order
        for l in z["lists"]:
            d = np.diff(l["ids"], axis=1)
            assert (d > 0).any() and (d < 0).any(), l["name"]
    hub = [m for m in B.zoo("tiles")["members"] if m["name"] == "hub"][0]
    rows = sum((l["ids"] == hub["ids"][0]).sum() * (2 if l["arity"] == 4 else 1) for l in B.zoo("tiles")["lists"])
    assert rows >= 8 + 28 + 2 * 6
    # the tiles box has one site per cell layer in z: members across the periodic seam and across both ghost-layer boundaries
    z = B.zoo("tiles")
    cell = z["box"][2] / z["nc"][2]
    for plane in (0.0, cell, z["box"][2] - cell):
        n = 0
        for m in z["members"]:
            dz = z["pos"][m["ids"] - 1][:, 2] - plane
            n += bool(dz.min() < 0 < dz.max())
        assert n >= 3, (plane, n)


@pytest.mark.parametrize("box", sorted(B.BOXES))
def test_oracle_matches_the_reference_on_well_conditioned_members(evaluated, box):
    z, h, stages = evaluated[box]
    for st in stages:
        err = B.molecule_errors(st["f"], st["ref"]["force"], z["mol"])
        sel = units(z, lambda m: not m["finite_only"] and m["name"] not in B.DEGENERATE)
        rel = np.array([err[u] / st["ref"]["fmax"][u] if st["ref"]["fmax"][u] > 0 else err[u] for u in sel])
        worst = sel[int(np.argmax(rel))]
        print("%s: largest oracle-to-reference error %.2e (%s, %s)" % (box, rel.max(), z["members"][worst]["name"], z["members"][worst]["order"]))
        assert rel.max() <= B.WELL, (z["members"][worst], rel.max())
        for i, l in enumerate(z["lists"]):
            if l["name"] not in B.FINITE_ONLY_LISTS:
                assert st["obs"]["epot_list"][h[i]] == pytest.approx(st["ref"]["energy"][i], rel=1e-12, abs=1e-12), l["name"]
            assert st["obs"]["list_size"][h[i]] == len(l["ids"])
        assert np.isfinite(st["f"]).all() and np.isfinite(st["obs"]["epot_list"]).all()


def test_near_degenerate_members_stay_within_twice_the_recorded_figure(evaluated):
    worst = {}
    for box, (z, h, stages) in evaluated.items():
        st = stages[0]
        err = B.molecule_errors(st["f"], st["ref"]["force"], z["mol"])
        for u, m in enumerate(z["members"]):
            if m["name"] in B.DEGENERATE:
                worst[m["name"]] = max(worst.get(m["name"], 0.0), err[u] / st["ref"]["fmax"][u])
    for name in sorted(worst):
        print("%-22s measured %.2e  recorded %.2e" % (name, worst[name], B.DEGENERATE[name]))
    for name, v in worst.items():
        assert v <= 2.0 * B.DEGENERATE[name], (name, v)
    assert set(worst) == set(B.DEGENERATE)


def test_unregistered_type_tuples_contribute_nothing_and_type_changes_move_tuples(evaluated):
    for box, (z, h, stages) in evaluated.items():
        first, second = stages
        for u in units(z, lambda m: m["name"] == "typed_unregistered"):
            p = z["members"][u]["ids"] - 1
            assert np.all(first["f"][p] == 0.0) and first["ref"]["fmax"][u] == 0.0
            assert np.abs(second["f"][p]).max() > 1.0                       # the tuples came in
        for u in units(z, lambda m: m["name"] in ("typed_forwards", "typed_palindrome")):
            p = z["members"][u]["ids"] - 1
            assert np.abs(first["ref"]["force"][p] - second["ref"]["force"][p]).max() > 1e-2 * first["ref"]["fmax"][u]
        typed = [i for i, l in enumerate(z["lists"]) if l.get("typed")]
        assert all(abs(first["ref"]["energy"][i] - second["ref"]["energy"][i]) > 1e-3 for i in typed if z["lists"][i]["name"] != "tbond_fenelj")


def test_the_cutoff_pair_sits_exactly_on_the_cutoff(evaluated):
    z, h, stages = evaluated["tiles"]
    x = stages[0]["x"]
    d = []
    for m in z["members"]:
        if m["name"] == "ljb_at":
            dx = x[m["ids"][0] - 1] - x[m["ids"][1] - 1]
            dx -= z["box"] * np.rint(dx / z["box"])
            d.append(np.sqrt((dx * dx).sum()))
    assert 2.5 in d, d


@pytest.mark.parametrize("lname", ["angc", "angh", "ncos", "dihh_b"])
def test_numpy_geometry_routines_match_the_reference(lname):
    """spline_ref.angle_terms / dihedral_terms (numpy, the oracle's formulation) against the autograd reference."""
    z = B.zoo("cells")
    l = [l for l in z["lists"] if l["name"] == lname][0]
    p = l["params"]
    fun = {"angc": lambda t: (p[0] * (1 + np.cos(t - p[1])), p[0] * np.sin(t - p[1])),
           "angh": lambda t: (p[0] * (t - p[1]) ** 2, -2 * p[0] * (t - p[1])),
           "ncos": lambda t: (p[0] * (1 + np.cos(p[2] * t - p[1])), p[0] * p[2] * np.sin(p[2] * t - p[1])),
           "dihh_b": lambda t: (0.5 * p[0] * np.arctan2(np.sin(t - p[1]), np.cos(t - p[1])) ** 2, -p[0] * np.arctan2(np.sin(t - p[1]), np.cos(t - p[1])))}[lname]
    F, E = (S.angle_terms if l["arity"] == 3 else S.dihedral_terms)(z["pos"], z["box"], l["ids"] - 1, fun)
    ref = B.reference(z["pos"], z["box"], z["types"], [l], z["mol"])
    err = B.molecule_errors(F, ref["force"], z["mol"])
    assert E == pytest.approx(ref["energy"][0], rel=1e-12)
    seen = 0
    for u, m in enumerate(z["members"]):
        if ref["fmax"][u] > 0:
            # the same formulation as the oracle, another libm call order: 10x the oracle's recorded figure where there is one
            tol = 10.0 * B.DEGENERATE[m["name"]] if m["name"] in B.DEGENERATE else B.WELL
            assert err[u] <= tol * ref["fmax"][u], (m["name"], err[u] / ref["fmax"][u])
            seen += 1
    assert seen >= 20
