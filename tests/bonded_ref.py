"""An independent reference of every bonded kind, and the molecule zoo the bonded tests evaluate it on.

Reference: plain torch fp64 on CPU tensors (GPU tests import this module: nothing here ever creates a device tensor).  Every
energy is written from the formulas in include/chem_mi355.h; forces are -autograd.grad of the summed energy, so no force
formula appears here at all.  Displacements take the minimum image per axis of an orthorhombic box.  The bending angle is
atan2(|r1 x r2|, r1 . r2), which keeps its digits where acos and sqrt(1 - c^2) lose them; the dihedral is the IUPAC atan2
form.  Tabulated kinds carry an e and an f column that are interpolated independently: the reference takes e(x) as the value
and -f(x) as the slope (a first-order surrogate around the evaluation point), so that autograd returns f(x) * dx/dpos.

Zoo: zoo(box_name) builds one system of small molecules ("members"), each at three id orders, packed into well-separated clusters
whose members exclude each other completely: the pair term is exactly zero and the reference needs none.
"""
import functools
import math

import numpy as np
import torch

ARITY = dict(HARMONIC=2, FENE=2, FENE_LJ=2, LJ_BOND=2, TABULATED=2, ANG_HARMONIC=3, ANG_COSINE=3, ANG_TABULATED=3,
             DIH_NCOS=4, DIH_RB=4, DIH_HARMONIC=4, DIH_TABULATED=4)
BONDS_ONLY_KINDS = ("HARMONIC", "FENE", "FENE_LJ", "LJ_BOND")

F64 = torch.float64


# ---- the reference ------------------------------------------------------------------------------------------------------------

def _mi(d, L):
    return d - L * torch.round(d / L)


def _table(x, tab):
    """Linear table (x0, dx, e, f) at x: value e(x), slope -f(x); the end rows hold beyond the grid."""
    x0, dx, e, f = tab
    e, f = torch.as_tensor(np.asarray(e), dtype=F64), torch.as_tensor(np.asarray(f), dtype=F64)
    n = e.shape[0]
    xv = x.detach()
    t = ((xv - x0) / dx).clamp(0.0, float(n - 1))
    k = t.floor().clamp(max=n - 2).long()
    w = t - k
    ev = e[k] + w * (e[k + 1] - e[k])
    fv = f[k] + w * (f[k + 1] - f[k])
    return ev - fv * (x - xv)


def _lj(r, eps, sig):
    s6 = (sig / r) ** 6
    return 4.0 * eps * (s6 * s6 - s6)


def _fene(r, K, r0, rmax):
    return -0.5 * K * rmax * rmax * torch.log(1.0 - ((r - r0) / rmax) ** 2)


def bend(x, L, idx):
    r1, r2 = _mi(x[idx[:, 0]] - x[idx[:, 1]], L), _mi(x[idx[:, 2]] - x[idx[:, 1]], L)
    return torch.atan2(torch.linalg.cross(r1, r2).norm(dim=1), (r1 * r2).sum(1))


def torsion(x, L, idx):
    b1, b2, b3 = _mi(x[idx[:, 1]] - x[idx[:, 0]], L), _mi(x[idx[:, 2]] - x[idx[:, 1]], L), _mi(x[idx[:, 3]] - x[idx[:, 2]], L)
    n1, n2 = torch.linalg.cross(b1, b2), torch.linalg.cross(b2, b3)
    return torch.atan2(b2.norm(dim=1) * (b1 * n2).sum(1), (n1 * n2).sum(1))


def _energy(kind, x, L, idx, P, tab):
    """Energy per tuple; P: (m, np) parameters per tuple."""
    if ARITY[kind] == 2:
        r = _mi(x[idx[:, 0]] - x[idx[:, 1]], L).norm(dim=1)
        if kind == "HARMONIC":
            return P[:, 0] * (r - P[:, 1]) ** 2
        if kind == "FENE":
            return _fene(r, P[:, 0], P[:, 1], P[:, 2])
        if kind == "FENE_LJ":            # (K, r0, rMax, sigma, epsilon)
            return _fene(r, P[:, 0], P[:, 1], P[:, 2]) + _lj(r, P[:, 4], P[:, 3])
        if kind == "LJ_BOND":            # (epsilon, sigma, cutoff): shifted to U(cutoff) = 0, nothing beyond the cutoff
            u = _lj(r, P[:, 0], P[:, 1]) - _lj(P[:, 2], P[:, 0], P[:, 1])
            return torch.where(r <= P[:, 2], u, torch.zeros_like(u))
        return _table(r, tab)
    if ARITY[kind] == 3:
        th = bend(x, L, idx)
        if kind == "ANG_HARMONIC":
            return P[:, 0] * (th - P[:, 1]) ** 2
        if kind == "ANG_COSINE":
            return P[:, 0] * (1.0 + torch.cos(th - P[:, 1]))
        return _table(th, tab)
    phi = torsion(x, L, idx)
    if kind == "DIH_NCOS":               # (K, phi0, n)
        return P[:, 0] * (1.0 + torch.cos(P[:, 2] * phi - P[:, 1]))
    if kind == "DIH_RB":
        c = torch.cos(phi - math.pi)
        return sum(P[:, k] * c ** k for k in range(6))
    if kind == "DIH_HARMONIC":           # the difference wrapped to (-pi, pi]
        d = phi - P[:, 1]
        d = torch.atan2(torch.sin(d), torch.cos(d))
        return 0.5 * P[:, 0] * d * d
    return _table(phi, tab)


def resolve(lst, types):
    """(tuples as 0-based indices, parameters per tuple) of a list under the particle types `types` (by id - 1).  A typed
    list takes, per tuple, the first registered type tuple that equals the tuple's current types read forwards or backwards;
    a tuple without one drops out."""
    ids = np.asarray(lst["ids"], dtype=np.int64).reshape(-1, lst["arity"])
    if lst.get("typed") is None:
        p = np.asarray(lst["params"] if lst.get("table") is None else [0.0], dtype=np.float64)
        return ids - 1, np.tile(p, (len(ids), 1))
    keep, prm = [], []
    for row in ids:
        tt = tuple(int(types[i - 1]) for i in row)
        for key, p in lst["typed"]:
            if tuple(key) == tt or tuple(key) == tt[::-1]:
                keep.append(row - 1)
                prm.append(p)
                break
    return np.asarray(keep, dtype=np.int64).reshape(-1, lst["arity"]), np.asarray(prm, dtype=np.float64).reshape(len(keep), -1)


def reference(pos, box, types, lists, mol=None):
    """force (n, 3) per particle, energy per list and -- with mol, the molecule index of every particle -- fmax, the largest
    |force component| of every molecule, which is what the comparisons scale by."""
    x = torch.tensor(np.asarray(pos, dtype=np.float64), dtype=F64, requires_grad=True)
    L = torch.tensor(np.asarray(box, dtype=np.float64), dtype=F64)
    total, energy = x.sum() * 0.0, []
    for lst in lists:
        idx, P = resolve(lst, types)
        if len(idx) == 0:
            energy.append(0.0)
            continue
        u = _energy(lst["kind"], x, L, torch.as_tensor(idx), torch.as_tensor(P, dtype=F64), lst.get("table")).sum()
        energy.append(float(u.detach()))
        total = total + u
    force = -torch.autograd.grad(total, x)[0].numpy()
    out = dict(force=force, energy=np.asarray(energy))
    if mol is not None:
        fmax = np.zeros(int(np.max(mol)) + 1)
        np.maximum.at(fmax, mol, np.abs(force).max(1))
        out["fmax"] = fmax
    return out


def molecule_errors(f, ref, mol):
    """Per molecule: max |f - ref| over its particles and components."""
    err = np.zeros(int(np.max(mol)) + 1)
    np.maximum.at(err, mol, np.abs(np.asarray(f) - np.asarray(ref)).max(1))
    return err


# ---- the conditioning of the near-degenerate members ---------------------------------------------------------------------------
# Oracle-to-reference force error of the near-degenerate members, relative to the member's own largest reference force
# component: the largest value over the member's three id orders and the three zoo boxes (tiles, cells, brute), measured on
# the CPU by tests/test_oracle_bonded.py, which prints every figure and asserts that the oracle stays within 2x of it.  The
# GPU tests allow 10x these figures (not below 1e-10).
#  - Bending angles: the oracle and the kernel compute theta = acos(c) and divide by sqrt(1 - c^2), so an error of one ulp in
#    the cosine becomes about 1e-16 / dev^2 in the force at a deviation dev from straight or folded.  Each member carries
#    harmonic (theta0 = 119 deg and theta0 = pi), cosine and tabulated bending terms.
#  - Dihedral with three members 1e-5 off collinear, at a generic orientation: the components of b1 x b2 are differences of
#    products of order 1 that leave 1e-5, an absolute rounding of 1e-16 each -- 1e-11 of the normal, in any formulation that
#    forms the cross product in fp64 (the reference included).  At 1e-3 and 1e-1 the member holds the bound of all others.
DEGENERATE = {
    "angle_straight_1e-2": 1.7e-12,   # measured 1.67e-12  (theta = pi - 1e-2)
    "angle_straight_1e-3": 1.4e-10,   # measured 1.37e-10  (theta = pi - 1e-3)
    "angle_straight_1e-4": 1.3e-8,    # measured 1.27e-8   (theta = pi - 1e-4)
    "angle_folded_1e-2": 1.5e-12,     # measured 1.48e-12  (theta = 1e-2)
    "angle_folded_1e-4": 2.1e-8,      # measured 2.08e-8   (theta = 1e-4)
    "dih_collinear_1e-5": 6.5e-12,    # measured 6.45e-12
}
# every other member: oracle against reference (largest seen 2.9e-14: angle_straight_1e-1)
WELL = 1e-12


# ---- the zoo ------------------------------------------------------------------------------------------------------------------

RC, SKIN = 24.6, 0.4
RL = RC + SKIN
# cell counts per axis (helpers.LADDER: the smallest tile-path box, the smallest cell-path box, a brute-force box) and the
# fraction of a cell on top: three different edges everywhere
BOXES = {"tiles": ((5, 5, 5), (0.2, 0.5, 0.9)), "cells": ((3, 3, 3), (0.5, 0.7, 0.9)), "brute": ((2, 7, 7), (0.5, 0.3, 0.7))}

_DPHI = 2.0 * math.pi / 720
_PHI = -math.pi + _DPHI * np.arange(721)
_PHI_SHORT = -3.0 + 0.01 * np.arange(601)                 # ends at +-3.0: phi = +-(pi - 0.1) lies beyond both ends
_TH = (math.pi / 180) * np.arange(181)                    # 0 .. pi: the near-straight and near-folded angles sit in the end intervals
_RB = 0.8 + 0.01 * np.arange(61)                          # 0.8 .. 1.4


def _lists():
    d2r = math.pi / 180
    L = [
        dict(name="harm", kind="HARMONIC", params=[30.0, 0.9]),
        dict(name="fene", kind="FENE", params=[30.0, 0.0, 1.5]),
        dict(name="fene_r0", kind="FENE", params=[30.0, 0.3, 1.5]),
        dict(name="fenelj", kind="FENE_LJ", params=[30.0, 0.0, 1.5, 1.0, 1.0]),
        dict(name="fenelj_r0", kind="FENE_LJ", params=[30.0, 0.3, 1.5, 1.05, 0.8]),
        dict(name="ljb", kind="LJ_BOND", params=[1.2, 1.0, 2.5]),
        dict(name="tabb", kind="TABULATED", table=(_RB[0], 0.01, 25.0 * (_RB - 0.95) ** 2 + 0.5 * np.sin(3.0 * _RB), -50.0 * (_RB - 0.95) - 1.5 * np.cos(3.0 * _RB))),
        dict(name="angh", kind="ANG_HARMONIC", params=[5.0, 119 * d2r]),
        dict(name="angh_pi", kind="ANG_HARMONIC", params=[5.0, math.pi]),
        dict(name="angc", kind="ANG_COSINE", params=[3.0, 130 * d2r]),
        dict(name="tabang", kind="ANG_TABULATED", table=(0.0, math.pi / 180, 4.0 * (_TH - 2.0) ** 2 + np.cos(2.0 * _TH), -8.0 * (_TH - 2.0) + 2.0 * np.sin(2.0 * _TH))),
        dict(name="ncos", kind="DIH_NCOS", params=[1.5, 20 * d2r, 3.0]),
        dict(name="rb", kind="DIH_RB", params=[0.5, -0.3, 0.2, 0.1, -0.1, 0.05]),
        dict(name="dihh_a", kind="DIH_HARMONIC", params=[4.0, 175 * d2r]),           # phi0 on either side of the seam
        dict(name="dihh_b", kind="DIH_HARMONIC", params=[4.0, -179 * d2r]),
        dict(name="tabdih", kind="DIH_TABULATED", table=(_PHI[0], _DPHI, 0.8 * (1 + np.cos(2 * _PHI - 0.3)), 1.6 * np.sin(2 * _PHI - 0.3))),
        dict(name="tabdih_short", kind="DIH_TABULATED", table=(-3.0, 0.01, 0.6 * (1 + np.cos(3 * _PHI_SHORT + 0.4)), 1.8 * np.sin(3 * _PHI_SHORT + 0.4))),
        dict(name="tbond", kind="HARMONIC", typed=[((1, 2), [30.0, 0.9]), ((2, 3), [25.0, 1.0]), ((3, 4), [20.0, 1.1]), ((2, 2), [35.0, 0.95])]),
        dict(name="tbond_fenelj", kind="FENE_LJ", typed=[((1, 2), [30.0, 0.0, 1.5, 1.0, 1.0]), ((4, 3), [25.0, 0.1, 1.6, 0.9, 0.7])]),
        dict(name="tang", kind="ANG_COSINE", typed=[((1, 2, 3), [3.0, 130 * d2r]), ((4, 3, 2), [2.0, 120 * d2r]), ((1, 2, 2), [2.5, 125 * d2r]), ((2, 1, 2), [1.5, 100 * d2r])]),
        dict(name="tdih", kind="DIH_HARMONIC", typed=[((1, 2, 3, 4), [4.0, 60 * d2r]), ((1, 2, 2, 1), [3.0, -100 * d2r]), ((1, 3, 2, 1), [2.0, 30 * d2r])]),
        # exactly degenerate geometries: the terms are only required to stay finite (the reference has no gradient there)
        dict(name="x_angc", kind="ANG_COSINE", params=[3.0, 130 * d2r]),
        dict(name="x_angh_pi", kind="ANG_HARMONIC", params=[5.0, math.pi]),
        dict(name="x_dih", kind="DIH_NCOS", params=[1.5, 20 * d2r, 3.0]),
    ]
    for l in L:
        l["arity"] = ARITY[l["kind"]]
    return L


FINITE_ONLY_LISTS = ("x_angc", "x_angh_pi", "x_dih")


def _place(a, b, c, bond, theta, phi):
    """The point at `bond` from c with bending angle theta at c and dihedral phi (IUPAC sign) about b-c."""
    bc = (c - b) / np.linalg.norm(c - b)
    n = np.cross(b - a, bc)
    n /= np.linalg.norm(n)
    m = np.cross(n, bc)
    return c + bond * (-math.cos(theta) * bc + math.sin(theta) * (math.cos(phi) * m + math.sin(phi) * n))


def _tetramer(bonds, cos_sin_1, theta2, phi):
    """Four points: bond lengths, (cos, sin) of the bending angle at point 1, the bending angle at point 2, the dihedral."""
    c1, s1 = cos_sin_1
    p0, p1 = np.zeros(3), np.array([bonds[0], 0.0, 0.0])
    p2 = p1 + bonds[1] * np.array([-c1, s1, 0.0])
    return np.stack([p0, p1, p2, _place(p0, p1, p2, bonds[2], theta2, phi)])


def _e(v):
    return "1e%d" % round(math.log10(v))


def _cs(deg):
    return math.cos(math.radians(deg)), math.sin(math.radians(deg))


def _members():
    """Every zoo member: name, local coordinates (chain order), types (chain order), terms [(list name, chain positions)],
    flags.  rotate = False keeps axis-aligned coordinates exact."""
    M = []

    def add(name, xyz, terms, types=None, rotate=True, finite_only=False, interleave=False):
        xyz = np.asarray(xyz, dtype=np.float64)
        M.append(dict(name=name, xyz=xyz, terms=terms, types=[0] * len(xyz) if types is None else list(types), rotate=rotate,
                      finite_only=finite_only, interleave=interleave))

    chain_bonds = [("harm", (0, 1)), ("harm", (1, 2)), ("harm", (2, 3))]
    chain_angles = [("angc", (0, 1, 2)), ("angc", (1, 2, 3))]
    every_dih = ["ncos", "rb", "dihh_a", "dihh_b", "tabdih", "tabdih_short"]
    # a generic tetramer with every family; two of the dihedral lists read the chain backwards
    add("generic", _tetramer((1.0, 0.95, 1.05), _cs(110), math.radians(125), math.radians(40)),
        chain_bonds + [("fene", (1, 0)), ("tabb", (2, 1)), ("fenelj", (3, 2)), ("ljb", (0, 3))] + chain_angles + [("angh", (2, 1, 0)), ("tabang", (1, 2, 3))] +
        [(n, (3, 2, 1, 0) if n in ("rb", "tabdih") else (0, 1, 2, 3)) for n in every_dih])
    # dihedrals at the seam of atan2, at 0 and at +-pi/2: every dihedral kind; the short table is evaluated beyond both ends
    # at +-(pi - 1e-1), the full one at its end rows
    for sgn in (+1, -1):
        for dev in (1e-1, 1e-3, 1e-6):
            add("dih_seam_%s%s" % ("+" if sgn > 0 else "-", _e(dev)), _tetramer((1.0, 1.0, 1.0), _cs(110), math.radians(115), sgn * (math.pi - dev)),
                chain_bonds + chain_angles + [(n, (0, 1, 2, 3)) for n in every_dih])
    for name, phi in (("dih_zero", 0.0), ("dih_+half_pi", 0.5 * math.pi), ("dih_-half_pi", -0.5 * math.pi)):
        add(name, _tetramer((1.0, 1.0, 1.0), _cs(110), math.radians(115), phi), chain_bonds + chain_angles + [(n, (0, 1, 2, 3)) for n in every_dih])
    # angles near straight and near folded: theta0 = pi and theta0 != pi, cosine, and the end intervals of the table
    ang = [("angh", (0, 1, 2)), ("angh_pi", (0, 1, 2)), ("angc", (2, 1, 0)), ("tabang", (0, 1, 2))]
    for dev in (1e-1, 1e-2, 1e-3, 1e-4):
        add("angle_straight_%s" % _e(dev), [[1.0, 0, 0], [0, 0, 0], [-1.1 * math.cos(dev), 1.1 * math.sin(dev), 0]], ang)
    for dev in (1e-2, 1e-4):
        add("angle_folded_%s" % _e(dev), [[1.0, 0, 0], [0, 0, 0], [1.1 * math.cos(dev), 1.1 * math.sin(dev), 0]], ang)
    # dihedrals whose first three members are nearly collinear (forces grow as 1 / offset)
    for off in (1e-1, 1e-3, 1e-5):
        add("dih_collinear_%s" % _e(off), _tetramer((1.0, 1.0, 1.0), (-math.cos(off), math.sin(off)), math.radians(115), math.radians(70)),
            chain_bonds + [(n, (0, 1, 2, 3)) for n in ("ncos", "rb", "dihh_a", "tabdih")])
    # FENE and FENE + LJ close to rMax, r0 = 0 and r0 != 0; the bond table below, inside and beyond its grid
    for ratio in (0.5, 0.9, 0.99):
        add("fene_%g" % ratio, [[0, 0, 0], [ratio * 1.5, 0, 0]], [("fene", (0, 1)), ("fenelj", (1, 0)), ("tabb", (0, 1))])
        add("fene_r0_%g" % ratio, [[0, 0, 0], [0.3 + ratio * 1.5, 0, 0]], [("fene_r0", (0, 1)), ("fenelj_r0", (1, 0))])
    # LJ pairs just inside, at and just outside the cutoff; along x with dyadic coordinates, so that r is |dx| exactly
    for name, r in (("ljb_inside", 2.5 * (1 - 1e-9)), ("ljb_at", 2.5), ("ljb_outside", 2.5 * (1 + 1e-9))):
        add(name, [[0, 0, 0], [r, 0, 0]], [("ljb", (0, 1))], rotate=False)
    # typed lists of arity 2, 3 and 4: forwards, backwards, palindromic, not registered, partly registered
    tet = _tetramer((0.95, 1.0, 1.05), _cs(112), math.radians(121), math.radians(-75))
    typed = [("tbond", (0, 1)), ("tbond", (1, 2)), ("tbond", (2, 3)), ("tbond_fenelj", (0, 1)), ("tbond_fenelj", (3, 2)),
             ("tang", (0, 1, 2)), ("tang", (1, 2, 3)), ("tdih", (0, 1, 2, 3))]
    for name, ty in (("typed_forwards", (1, 2, 3, 4)), ("typed_backwards", (4, 3, 2, 1)), ("typed_palindrome", (1, 2, 2, 1)),
                     ("typed_unregistered", (5, 6, 5, 6)), ("typed_partly", (1, 2, 3, 5))):
        add(name, tet, typed, types=ty)
    # a hub: 8 arms, bonds from three lists (one typed), all 28 arm-hub-arm angles over three lists, 7 dihedrals with the hub
    # in every role; one list_add call per tuple, so that the calls interleave across the lists
    rng = np.random.default_rng(5)
    while True:
        arms = rng.normal(size=(8, 3))
        arms /= np.linalg.norm(arms, axis=1)[:, None]
        c = arms @ arms.T
        if np.abs(c[np.triu_indices(8, 1)]).max() < 0.9:
            break
    arms *= rng.uniform(0.85, 1.15, 8)[:, None]
    bonds = [("harm", (0, 1)), ("fene", (0, 4)), ("tbond", (7, 0)), ("harm", (2, 0)), ("fene", (5, 0)), ("tbond", (0, 8)), ("harm", (0, 3)), ("fene", (0, 6))]
    angs = [(("angh", "angc", "tabang")[k % 3], (a, 0, b)) for k, (a, b) in enumerate((a, b) for a in range(1, 9) for b in range(a + 1, 9))]
    dihs = [("ncos", (1, 0, 2, 3)), ("rb", (4, 0, 5, 6)), ("dihh_a", (7, 0, 8, 1)), ("tabdih", (0, 2, 3, 4)), ("ncos", (0, 5, 6, 7)),
            ("dihh_b", (8, 7, 6, 0)), ("rb", (2, 3, 0, 4))]
    terms = []
    for k in range(len(angs)):
        terms.append(angs[k])
        if k < len(bonds):
            terms.append(bonds[k])
        if k % 4 == 0:
            terms.append(dihs[k // 4])
    add("hub", np.concatenate([np.zeros((1, 3)), arms]), terms, types=[2, 0, 0, 0, 0, 0, 0, 1, 1], interleave=True)
    # exactly straight, and exactly collinear: only finiteness is asserted
    add("exact_straight", [[1.0, 0, 0], [0, 0, 0], [-1.25, 0, 0]], [("x_angc", (0, 1, 2)), ("x_angh_pi", (0, 1, 2))], rotate=False, finite_only=True)
    add("exact_collinear", [[0, 0, 0], [0.75, 0, 0], [1.5, 0, 0], [2.5, 0, 0]], [("x_dih", (0, 1, 2, 3))], rotate=False, finite_only=True)
    return M


# type changes after the first comparison: (member, chain position, new type).  typed_unregistered comes in (1, 2, 3, 4);
# typed_forwards loses its last bond, angle and its dihedral (1, 2, 3, 5); typed_palindrome changes slot in all three lists
# (1, 2, 3, 1): bond (2, 2) -> (2, 3), angle (1, 2, 2) -> (1, 2, 3), dihedral (1, 2, 2, 1) -> (1, 3, 2, 1) read backwards
RETYPE = [("typed_unregistered", 0, 1), ("typed_unregistered", 1, 2), ("typed_unregistered", 2, 3), ("typed_unregistered", 3, 4),
          ("typed_forwards", 3, 5), ("typed_palindrome", 2, 3)]


def _order(k, which, rng):
    """id offset of every chain position."""
    if which == "ascending":
        return np.arange(k)
    if which == "descending":
        return np.arange(k)[::-1].copy()
    while True:
        p = rng.permutation(k)
        if k < 3 or (not np.array_equal(p, np.arange(k)) and not np.array_equal(p, np.arange(k)[::-1])):
            return p


def _rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


@functools.lru_cache(maxsize=None)
def _zoo(box_name, select):
    nc, frac = BOXES[box_name]
    box = (np.asarray(nc, dtype=np.float64) + np.asarray(frac)) * RL
    lists = _lists()
    members = [m for m in _members() if select is None or m["name"].startswith(select)]
    units = []                                      # (member, order)
    for m in members:
        for which in (("ascending", "descending", "shuffled") if len(m["xyz"]) > 2 else ("ascending", "descending")):
            units.append((m, which))
    # sites: a grid whose pitch leaves more than rc + skin between the clusters; site 0 of an axis sits on the face, and on z
    # the tiles box has one site per cell layer, so that the sites 1 and 4 sit on the ghost-layer boundaries of a slab
    extent = 4.0
    msite = np.floor(box / (RL + extent + 0.05)).astype(int)
    assert msite.min() >= 2
    pitch = box / msite
    sites = np.stack(np.meshgrid(*[np.arange(k) for k in msite], indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(17)
    n, pos, types, mol, cluster, mem = 0, [], [], [], [], []
    entries = []
    per_site = -(-len(units) // len(sites))
    for u, (m, which) in enumerate(units):
        site, slot = u % len(sites), u // len(sites)
        k = len(m["xyz"])
        xyz = m["xyz"] - 0.5 * (m["xyz"].min(0) + m["xyz"].max(0))
        rot = _rotation(rng)
        if m["rotate"]:
            xyz = xyz @ rot.T
        assert np.abs(xyz).max() < 0.5 * extent - 0.15 * per_site / 2 - 0.05, (m["name"], np.abs(xyz).max())
        anchor = sites[site] * pitch + (slot - 0.5 * (per_site - 1)) * np.array([0.15, 0.1, 0.05])
        anchor = np.round(anchor * 64.0) / 64.0
        order = _order(k, which, rng)
        ids = n + 1 + order                            # id of chain position j
        p = np.empty((k, 3))
        p[order] = xyz + anchor
        t = np.empty(k, np.int32)
        t[order] = m["types"]
        pos.append(p); types.append(t)
        mol += [u] * k; cluster += [site] * k
        mem.append(dict(name=m["name"], order=which, ids=ids, finite_only=m["finite_only"], site=tuple(sites[site])))
        run = []
        for (ln, cp) in m["terms"]:
            li = [l["name"] for l in lists].index(ln)
            run.append((li, tuple(int(ids[c]) for c in cp)))
        if not m["interleave"]:
            run.sort(key=lambda e: e[0])             # one call per list and member
        entries += run
        n += k
    pos = np.concatenate(pos); types = np.concatenate(types)
    mol, cluster = np.asarray(mol), np.asarray(cluster)
    for li, l in enumerate(lists):
        l["ids"] = np.asarray([e[1] for e in entries if e[0] == li], dtype=np.int64).reshape(-1, l["arity"])
    renumber = {li: k for k, li in enumerate(li for li, l in enumerate(lists) if len(l["ids"]))}
    lists = [l for l in lists if len(l["ids"])]
    entries = [(renumber[li], ids) for li, ids in entries]
    # everything inside a cluster is excluded; clusters are further apart than rc + skin
    excl = []
    for s in np.unique(cluster):
        i = np.nonzero(cluster == s)[0] + 1
        a, b = np.triu_indices(len(i), 1)
        excl.append(np.stack([i[a], i[b]], 1))
    excl = np.concatenate(excl)
    d = pos[:, None, :] - pos[None, :, :]
    d -= box * np.rint(d / box)
    r = np.sqrt((d * d).sum(2))
    r[cluster[:, None] == cluster[None, :]] = np.inf
    assert r.min() > RL + 0.05, r.min()
    retype = []
    for (name, cp, ty) in RETYPE:
        retype += [(int(u["ids"][cp]), ty) for u in mem if u["name"] == name]
    return dict(name=box_name, box=box, nc=nc, rc=RC, skin=SKIN, dt=0.002, n=n, ids=np.arange(1, n + 1), types=types, pos=pos, mass=np.ones(n),
                mol=mol, members=mem, lists=lists, entries=entries, exclusions=excl, retype=retype)


def zoo(box_name, select=None):
    """The zoo in one of BOXES (select: only the members whose name starts with it).  Read-only: shared between tests."""
    return _zoo(box_name, select)


def straddlers(spec):
    """Per axis, the units with particles on both sides of the face at 0; and the units across all three (the corner)."""
    out = {0: [], 1: [], 2: [], "corner": []}
    for u, m in enumerate(spec["members"]):
        p = spec["pos"][m["ids"] - 1]
        across = [(p[:, d].min() < 0 < p[:, d].max()) for d in range(3)]
        for d in range(3):
            if across[d]:
                out[d].append(u)
        if all(across):
            out["corner"].append(u)
    return out


def pick_lists(spec, kinds=None, names=None):
    """Indices of the spec's lists of the given kinds / names."""
    return [i for i, l in enumerate(spec["lists"]) if (kinds is None or l["kind"] in kinds) and (names is None or l["name"] in names)]


def build(eng, spec, use=None, vel=None):
    """Set the zoo up on an engine (oracle or HIP); use: indices of the lists to create (default all).  The tuples are added in
    the zoo's emission order, one call per run of tuples of one list.  Returns {list index in spec: handle}."""
    eng.set_box(spec["box"])
    eng.set_cutoff(spec["rc"], spec["skin"])
    eng.set_dt(spec["dt"])
    eng.set_particles(spec["ids"], spec["types"], spec["pos"], spec["mass"], vel=vel)
    ty = sorted(set(int(t) for t in spec["types"]) | set(t for _, t in spec["retype"]))
    for a in ty:                                        # a pair potential between all types: zero by construction of the zoo
        for b in ty:
            if a <= b:
                eng.nb_lj(a, b, 1.0, 1.0, spec["rc"], True)
    use = list(range(len(spec["lists"]))) if use is None else list(use)
    handles = {}
    for i in use:
        l = spec["lists"][i]
        h = eng.list_create(l["arity"], l["kind"], l.get("typed") is not None)
        if l.get("typed") is not None:
            for key, p in l["typed"]:
                eng.list_set_params(h, p, types=key)
        elif l.get("table") is not None:
            eng.list_set_params(h, [eng.table_create(*l["table"])])
        else:
            eng.list_set_params(h, l["params"])
        handles[i] = h
    run, cur = [], None
    for li, ids in spec["entries"] + [(None, None)]:
        if li != cur and run:
            eng.list_add(handles[cur], run)
            run = []
        cur = li
        if li in handles:
            run.append(ids)
    eng.set_exclusions(spec["exclusions"])
    return handles
