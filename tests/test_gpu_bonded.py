"""Every bonded kind on the device against the independent fp64 autograd reference of tests/bonded_ref.py, on the molecule zoo
(tests/test_oracle_bonded.py runs the same zoo through the CPU restatement): the seam of the dihedral, bending angles near
straight and folded, nearly collinear dihedrals, the clamped ends of the tables, FENE close to rMax, the LJ pair at its cutoff,
tuples across faces, a corner and the ghost-layer boundaries of anisotropic boxes, a hub that owns dozens of CSR rows of mixed
arity, and typed lists of arity 2, 3 and 4 before and after type changes -- on every bonded kernel path, in both precisions.

The reference is evaluated at the positions the engine returns, so the quantisation of the fp32 position codec is not
counted as error.  Every tolerance is relative to the largest reference force component of the molecule itself.

Tolerances
  fp64, well-conditioned members   1e-10 on forces, rtol 1e-11 on list energies (the project's parity figures)
  fp64, near-degenerate members    10 x the oracle-to-reference figure recorded in bonded_ref.DEGENERATE, not below 1e-10
  fp32                             bonded geometry is fp64 in this build and the force of a particle is rounded to fp32 once,
                                   when it is added to the force array: 2^-24 = 6e-8 per component, 1e-6 with margin (no
                                   harmonic bond is evaluated inline by the fp32 pair kernel here: no context of this file has
                                   a single harmonic list); never below the fp64 rule; energies rtol 2e-4, atol 1e-3
"""
import numpy as np
import pytest

import bonded_ref as B
from conftest import rel_err

pytestmark = pytest.mark.gpu

# the zoo's box and what selects the kernel (as test_gpu_hybrid_bonds.PATHS does)
PATHS = {
    "default": dict(box="tiles"),                                          # work list, full kernel, fused rebuild
    "bonds_only": dict(box="tiles", kinds=B.BONDS_ONLY_KINDS),             # k_bonded_work<.., BONDS_ONLY>
    "unfused": dict(box="tiles", opts={"fused_rebuild": 0}),               # k_bonded_prep in a launch of its own
    "no_tiles": dict(box="tiles", opts={"tiles": 0}),                      # per-particle k_bonded
    "dd_self": dict(box="tiles", opts={"dd_self": 1}),                     # one slab that is its own neighbour
    "cells": dict(box="cells"),                                            # the smallest cell-path box
    "brute": dict(box="brute"),                                            # fewer than three cells on x
}
TOL_F = {64: 1e-10, 32: 1e-6}
TOL_E = {64: dict(rel=1e-11, abs=1e-11), 32: dict(rel=2e-4, abs=1e-3)}

_REF = {}


def reference(z, use, x, types):
    """The reference at positions x, computed once per distinct (box, lists, positions, types)."""
    key = (z["name"], tuple(use), x.tobytes(), types.tobytes())
    if key not in _REF:
        _REF[key] = B.reference(x, z["box"], types, [z["lists"][i] for i in use], z["mol"])
    return _REF[key]


def tolerance(name, prec):
    return max(TOL_F[prec], 10.0 * B.DEGENERATE.get(name, 0.0))


def engine(make_gpu, z, prec, opts, use, vel=None):
    g = make_gpu(prec)
    for k in sorted(opts, key=lambda k: k != "dd_self"):                   # (dd_self first: it picks the transport)
        g.set_option(k, opts[k])
    return g, B.build(g, z, use, vel=vel)


def compare(g, h, z, use, types, prec, label):
    g.run(0)
    f, x, obs = g.get_state("FORCE"), g.get_state("POS"), g.observe()
    ref = reference(z, use, x, types)
    assert np.isfinite(f).all() and np.isfinite(obs["epot_list"]).all(), label
    err = B.molecule_errors(f, ref["force"], z["mol"])
    bad, worst = [], (0.0, None)
    for u, m in enumerate(z["members"]):
        if m["finite_only"]:
            continue
        p = m["ids"] - 1
        fmax = ref["fmax"][u]
        rel = err[u] / fmax if fmax > 0 else err[u]
        if rel > worst[0] and m["name"] not in B.DEGENERATE:
            worst = (rel, m["name"] + "/" + m["order"])
        if m["name"] in B.DEGENERATE:
            print("%s fp%d %s/%s: %.2e (allowed %.2e)" % (label, prec, m["name"], m["order"], rel, tolerance(m["name"], prec)))
        if not err[u] <= tolerance(m["name"], prec) * fmax:
            bad.append((m["name"], m["order"], m["site"], rel))
        # the net force of a molecule is zero to rounding: every member of a tuple evaluates the same term (fp64: sums of a
        # few dozen terms; fp32: one rounding per particle when its force is stored)
        net = np.abs(f[p].sum(0)).max()
        assert net <= (1e-12 if prec == 64 else len(p) * 2.0 ** -23) * fmax, (label, m["name"], m["order"], net, fmax)
    print("%s fp%d: largest error of a well-conditioned member %.2e (%s)" % (label, prec, worst[0], worst[1]))
    assert not bad, (label, prec, bad)
    for k, i in enumerate(use):
        l = z["lists"][i]
        assert obs["list_size"][h[i]] == len(l["ids"]), (label, l["name"])
        if l["name"] not in B.FINITE_ONLY_LISTS:
            assert obs["epot_list"][h[i]] == pytest.approx(ref["energy"][k], **TOL_E[prec]), (label, l["name"])
    return f, ref


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("path", sorted(PATHS))
def test_every_member_on_every_path(make_gpu, path, prec):
    cfg = PATHS[path]
    z = B.zoo(cfg["box"])
    use = B.pick_lists(z, kinds=cfg.get("kinds"))
    assert len(use) == (len(z["lists"]) if "kinds" not in cfg else 8)
    g, h = engine(make_gpu, z, prec, cfg.get("opts", {}), use)
    types = z["types"].copy()
    f, ref = compare(g, h, z, use, types, prec, path)
    # a tuple whose types are not registered contributes nothing at all
    quiet = [m for m in z["members"] if m["name"] == "typed_unregistered"]
    assert len(quiet) == 3 and all(np.all(f[m["ids"] - 1] == 0.0) for m in quiet)
    e0 = ref["energy"].copy()
    # type changes: tuples come in, drop out and change slot
    for pid, ty in z["retype"]:
        g.modify_particle(pid, "type", ty)
        types[pid - 1] = ty
    f, ref = compare(g, h, z, use, types, prec, path + " retyped")
    assert all(np.abs(f[m["ids"] - 1]).max() > 1.0 for m in quiet)
    typed = [k for k, i in enumerate(use) if z["lists"][i].get("typed") and z["lists"][i]["name"] != "tbond_fenelj"]
    assert typed and all(abs(ref["energy"][k] - e0[k]) > 1e-3 for k in typed)


@pytest.mark.parametrize("prec", [64, 32])
def test_fene_lj_and_harmonic_dihedrals_through_the_stepping_launch(make_gpu, make_oracle, prec):
    """50 NVE steps of the zoo's FENE + LJ bonds and of its harmonic dihedrals around the seam against the oracle."""
    z = B.zoo("tiles", ("fene", "dih_seam", "dih_zero", "dih_+", "dih_-"))
    assert {"FENE_LJ", "DIH_HARMONIC"} <= {l["kind"] for l in z["lists"]}
    vel = np.random.default_rng(3).normal(0, 0.3, (z["n"], 3))
    g, h = engine(make_gpu, z, prec, {}, None, vel=vel)
    o = make_oracle()
    B.build(o, z, vel=vel)
    g.run(0); o.run(0)
    assert rel_err(g.get_state("FORCE"), o.get_state("FORCE")) < (1e-10 if prec == 64 else 5e-5)
    g.run(50); o.run(50)
    x, xo = g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")
    assert np.abs(xo - z["pos"]).max() > 0.01                              # (it moved)
    assert rel_err(x, xo) < (1e-9 if prec == 64 else 2e-4), prec
