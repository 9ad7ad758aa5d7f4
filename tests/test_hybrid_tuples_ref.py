"""tests/hybrid_tuples_ref.py against what is known without it, on the CPU: at lambda = 1 it is bonded_ref.reference; for the kinds
that are linear in their K (ANG_HARMONIC, ANG_COSINE, the cosine / harmonic / Ryckaert-Bellemans dihedrals, all six RB coefficients
scaled) one shared lambda is the CPU oracle run with K lambda; an entry at lambda = 0 is left out, also where its term is not
finite; what spawned() says the topology manager spawns is what the oracle's topology manager spawns.

System: hybrid_tuples_ref.scene(), the one of tests/test_gpu_hybrid_tuples.py, with every gap closed (the tuples a run of both
reactions spawns).  Its bending angles lie within 60..150 degrees and its dihedral members at least 0.5 off collinear (asserted),
so the plain bounds of tests/test_oracle_bonded.py apply: force error 1e-12 of the molecule's largest force component (B.WELL),
list energies 1e-12."""
import math

import numpy as np
import pytest

import bonded_ref as B
import hybrid_tuples_ref as T
from chemlab_amd import workloads as W

D2R = math.pi / 180
LINEAR = {                        # kind -> (parameters, indices of the parameters that scale with lambda)
    "ANG_HARMONIC": ([8.0, 1.6], [0]),
    "ANG_COSINE": ([3.0, 130 * D2R], [0]),
    "DIH_NCOS": ([2.0, 0.35, 3.0], [0]),
    "DIH_HARMONIC": ([4.0, 175 * D2R], [0]),
    "DIH_RB": ([0.5, -0.3, 0.2, 0.1, -0.1, 0.05], [0, 1, 2, 3, 4, 5]),
}


@pytest.fixture(scope="module")
def closed():
    """the scene with both reactions run: bonds, and the tuples spawned around them (births 1 and 5)"""
    s = T.scene()
    ev = [(1, a, b) for a, b in s["r0"]] + [(5, a, b) for a, b in s["r1"]]
    t3, s3, t4, s4 = T.spawned(s["bonds0"], ev, s["types"], T.REG3, T.REG4)
    assert (len(t3), len(t4)) == (475, 302) and sorted(set(s3.tolist())) == [1, 5] and sorted(set(s4.tolist())) == [1, 5]
    assert T.geometry_ok(s["pos"], s["box"], np.concatenate([t3, s["angles0"]]), np.concatenate([t4, s["dihedrals0"]]))
    # chains whose beads all react: the molecule index (a chain) is the unit the errors are scaled by
    return dict(scene=s, t3=t3, s3=s3, t4=t4, s4=s4)


def lists_of(c, kinds=("ANG_HARMONIC", "DIH_NCOS"), scale=1.0):
    out = []
    for kind in kinds:
        p, lin = LINEAR[kind]
        out.append(dict(arity=B.ARITY[kind], kind=kind, params=[v * (scale if i in lin else 1.0) for i, v in enumerate(p)],
                        ids=c["t3"] if B.ARITY[kind] == 3 else c["t4"]))
    return out


def test_ramp_is_the_one_expression():
    assert T.ramp(0.0, 0.125, 6, [1, 5, 6]).tolist() == [0.625, 0.125, 0.0]
    assert T.ramp(0.25, 0.0625, 100, [3]).tolist() == [1.0] and T.ramp(0.375, 0.0, 10 ** 9, [0]).tolist() == [0.375]      # clamps at exactly 1; rate 0 keeps lambda0


def test_lambda_one_is_the_plain_reference(closed):
    s = closed["scene"]
    for kinds in (("ANG_HARMONIC", "DIH_NCOS"), ("ANG_COSINE", "DIH_RB"), ("ANG_HARMONIC", "DIH_HARMONIC")):
        lists = lists_of(closed, kinds)
        ref = B.reference(s["pos"], s["box"], s["types"], lists, s["mol"])
        got = T.reference(s["pos"], s["box"], s["types"], lists, [1.0, np.ones(len(closed["t4"]))])
        err = B.molecule_errors(got["force"], ref["force"], s["mol"]) / ref["fmax"]
        assert err.max() <= B.WELL and np.abs(ref["force"]).max() > 1.0
        assert got["energy"] == pytest.approx(ref["energy"], rel=1e-12, abs=1e-12)
        assert all(len(u) == len(l["ids"]) for u, l in zip(got["per_entry"], lists))
        assert [float(u.sum()) for u in got["per_entry"]] == pytest.approx(got["energy"].tolist(), rel=1e-14)


@pytest.mark.parametrize("kinds", [("ANG_HARMONIC", "DIH_NCOS"), ("ANG_COSINE", "DIH_RB"), ("ANG_HARMONIC", "DIH_HARMONIC")], ids=lambda k: "+".join(k))
@pytest.mark.parametrize("lam", [0.125, 0.625])
def test_one_shared_lambda_is_the_oracle_with_k_lambda(closed, make_oracle, kinds, lam):
    s = closed["scene"]
    got = T.reference(s["pos"], s["box"], s["types"], lists_of(closed, kinds), [lam, lam])
    o = make_oracle()
    spec = dict({k: s[k] for k in ("n", "box", "rc", "skin", "dt", "ids", "types", "pos", "vel", "mass", "state", "res_id", "kT", "gamma", "seed")},
                lj=[], exclusions=None, lists=lists_of(closed, kinds, scale=lam))
    h = W.apply(spec, o, thermostat=False, reactions=False)
    o.run(0)
    fo, ob = o.get_state("FORCE"), o.observe()
    plain = B.reference(s["pos"], s["box"], s["types"], lists_of(closed, kinds), s["mol"])
    err = B.molecule_errors(got["force"], fo, s["mol"]) / (lam * plain["fmax"])
    print("%s lambda %.3f: largest error %.2e of a chain's largest force" % ("+".join(kinds), lam, err.max()))
    assert err.max() <= B.WELL                                                   # the plain bound of tests/test_oracle_bonded.py
    for k in range(2):
        assert ob["epot_list"][h[k]] == pytest.approx(got["energy"][k], rel=1e-12, abs=1e-12)
    assert np.abs(got["force"] - plain["force"]).max() > 0.3 * np.abs(plain["force"]).max()      # (full strength is far away)


def test_every_entry_has_its_own_lambda_and_zero_is_left_out(closed):
    s = closed["scene"]
    lists = lists_of(closed)
    lam3, lam4 = T.ramp(0.0, 0.125, 6, closed["s3"]), T.ramp(0.0, 0.125, 6, closed["s4"])
    assert sorted(set(lam3.tolist())) == [0.125, 0.625]
    got = T.reference(s["pos"], s["box"], s["types"], lists, [lam3, lam4])
    # the sum over the cohorts, each a shared-lambda problem
    parts = np.zeros_like(got["force"])
    energy = np.zeros(2)
    for birth in (1, 5):
        sub = [dict(lists[0], ids=closed["t3"][closed["s3"] == birth]), dict(lists[1], ids=closed["t4"][closed["s4"] == birth])]
        r = B.reference(s["pos"], s["box"], s["types"], sub, s["mol"])
        lam = float(T.ramp(0.0, 0.125, 6, birth))
        parts += lam * r["force"]; energy += lam * r["energy"]
    assert np.abs(got["force"] - parts).max() <= 1e-13 * np.abs(parts).max() and got["energy"] == pytest.approx(energy, rel=1e-13)
    # lambda = 0 on an exactly straight angle and an exactly collinear dihedral: left out, the rest unchanged
    x = s["pos"].copy()
    n, a, b, m = 1, 2, 3, 4                                    # the first chain (kind A): n a | b m
    assert closed["t3"][0].tolist() == [n, a, b] and closed["t4"][0].tolist() == [n, a, b, m]
    d = x[b - 1] - x[a - 1]
    x[n - 1] = x[a - 1] - 0.8 * d / np.linalg.norm(d)
    lam3, lam4 = np.ones(len(closed["t3"])), np.ones(len(closed["t4"]))
    lam3[0] = lam4[0] = 0.0
    z = T.reference(x, s["box"], s["types"], lists, [lam3, lam4])
    rest = B.reference(x, s["box"], s["types"], [dict(lists[0], ids=closed["t3"][1:]), dict(lists[1], ids=closed["t4"][1:])], s["mol"])
    assert np.isfinite(z["force"]).all() and np.array_equal(z["force"], rest["force"]) and z["per_entry"][0][0] == 0.0 and z["per_entry"][1][0] == 0.0
    full = T.reference(x, s["box"], s["types"], lists, [1.0, 1.0])
    assert not np.array_equal(full["force"][:4], rest["force"][:4])      # (at any other lambda the entry counts)


def test_typed_lists_drop_rows_and_keep_lambda_aligned(closed):
    s = closed["scene"]
    typed = [((3, 0, 1), [8.0, 1.6]), ((0, 1, 2), [6.0, 1.7])]           # only two of the six registered triples have parameters
    lst = dict(arity=3, kind="ANG_HARMONIC", typed=typed, ids=closed["t3"])
    lam = np.linspace(0.1, 1.0, len(closed["t3"]))
    got = T.reference(s["pos"], s["box"], s["types"], [lst], [lam])
    idx, P = B.resolve(lst, s["types"])
    assert 0 < len(idx) < len(closed["t3"]) and len(got["per_entry"][0]) == len(idx)
    keep = [k for k, t in enumerate(closed["t3"].tolist()) if tuple(int(s["types"][i - 1]) for i in t) in ((3, 0, 1), (1, 0, 3), (0, 1, 2), (2, 1, 0))]
    plain = B.reference(s["pos"], s["box"], s["types"], [dict(lst, ids=closed["t3"][keep])])
    one = T.reference(s["pos"], s["box"], s["types"], [dict(lst, ids=closed["t3"][keep])], [np.ones(len(keep))])
    assert one["per_entry"][0] * lam[keep] == pytest.approx(got["per_entry"][0], rel=1e-14) and plain["energy"][0] == pytest.approx(one["energy"][0], rel=1e-14)


def test_spawned_is_what_the_oracle_topology_manager_spawns(closed, make_oracle):
    s = closed["scene"]
    o = make_oracle()
    spec = dict({k: s[k] for k in ("n", "box", "rc", "skin", "dt", "ids", "types", "pos", "vel", "mass", "state", "res_id", "kT", "gamma", "seed")},
                lj=[(a, b, 1.0, 0.4, s["rc"]) for a in range(4) for b in range(a, 4)], exclusions=s["exclusions"],
                lists=[dict(arity=2, kind="HARMONIC", params=[20.0, 0.9], ids=s["bonds0"]),
                       dict(arity=3, kind="ANG_HARMONIC", params=[8.0, 1.6], ids=np.zeros((0, 3), np.int64), register=T.REG3),
                       dict(arity=4, kind="DIH_NCOS", params=[2.0, 0.35, 3.0], ids=np.zeros((0, 4), np.int64), register=T.REG4)])
    h = W.apply(spec, o, thermostat=False, reactions=False)
    hb = o.list_create(2, "HARMONIC")
    o.list_set_params(hb, [30.0, 1.0])
    o.reaction_init(1, True, 0, 4)
    common = dict(delta_1=1, delta_2=1, min_state_1=0, max_state_1=1, min_state_2=0, max_state_2=2, cutoff=T.REACT_CUT, bond_list=hb, intramolecular=True, intraresidual=True)
    o.reaction_add(0, 1, rate=1e30, **common)
    r1 = o.reaction_add(2, 1, rate=0.0, **common)
    o.reactions_enable(True)
    o.run(4)
    o.reaction_set_rate(r1, 1e30)
    o.run(1)
    ev = [(int(e["step"]), int(e["id_a"]), int(e["id_b"])) for e in o.get_events()]
    assert sorted((a, b) for st, a, b in ev if st == 1) == s["r0"] and sorted((a, b) for st, a, b in ev if st == 5) == s["r1"]
    t3, s3, t4, s4 = T.spawned(s["bonds0"], ev, s["types"], T.REG3, T.REG4)
    canon = lambda rows: sorted(min(tuple(r), tuple(r[::-1])) for r in np.asarray(rows).tolist())
    assert canon(o.get_list(h[1])) == canon(t3) == canon(closed["t3"]) and canon(o.get_list(h[2])) == canon(t4) == canon(closed["t4"])
