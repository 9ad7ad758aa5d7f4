"""The oracle against numpy on every system tests/test_gpu_geometry.py uses (CPU only).

The oracle bins particles into the same cells as the engine, so a mistake both make at a cell-count threshold would pass
every engine-against-oracle test.  helpers.brute_pairs and helpers.pair_reference know no cells: all pairs, minimum
image.  This file also shows, without a GPU, that the generators' preconditions hold (geometry_spec asserts them and
redraws) and that the dynamic legs do what their GPU tests need: rebuilds, image changes, a rank emptied and one filled.
"""
import numpy as np
import pytest

import helpers as H
from chemlab_amd import workloads as W


def _check_static(o, spec, ref):
    o.run(0)
    assert np.array_equal(H.canonical_pairs(o.get_verlet_pairs()), spec["pairs"])
    f, elj, _, vir = ref
    assert np.abs(o.get_state("FORCE") - f).max() <= 1e-12 * np.abs(f).max()
    obs = o.observe()
    assert obs["epot_lj"] == pytest.approx(elj, rel=1e-12, abs=1e-12 * spec["n"])
    assert obs["virial_nb"] == pytest.approx(vir, rel=1e-12, abs=1e-12 * spec["n"])


@pytest.mark.parametrize("fill", ["uniform", "corner_droplet"])
@pytest.mark.parametrize("frac", [0.5, 0.0])
@pytest.mark.parametrize("nc", H.LADDER_BOXES, ids=lambda nc: "%dx%dx%d" % nc)
def test_oracle_list_forces_and_energies_equal_numpy_on_the_ladder(make_oracle, nc, frac, fill):
    spec = H.ladder_spec(nc, frac, fill)
    assert spec["min_gap"] > 1e-9 and spec["n"] <= 7000
    o = make_oracle()
    W.apply(spec, o)
    _check_static(o, spec, H.geometry_reference("ladder", nc, frac, fill))
    if fill == "corner_droplet":                       # the dynamic leg of the GPU test: enough rebuilds, enough wrapped particles
        o.run(H.LADDER_STEPS)
        assert o.timers()["rebuilds"] >= 20
        assert int((o.get_state("IMAGE") != 0).any(1).sum()) >= 30


def _layers(spec, x):
    L = spec["box"][2]
    nzg = spec["nc"][2]
    z = x[:, 2] - np.floor(x[:, 2] / L) * L
    return z * nzg / L                                 # (fractional cell layer)


@pytest.mark.parametrize("name", sorted(H.SLAB_CASES))
def test_oracle_equals_numpy_on_the_slab_cases_and_the_films_travel(make_oracle, name):
    spec = H.slab_spec(name)
    o = make_oracle()
    W.apply(spec, o)
    _check_static(o, spec, H.geometry_reference("slab", name))
    P = H.SLAB_CASES[name][4][0]
    if P == 1:
        return
    caps = H.slab_capacities(spec, P)
    owners0 = [c["n_real"] > 0 for c in caps]
    o.run(H.LADDER_STEPS)
    lay = _layers(spec, o.get_state("POS"))
    # where the film is at the end, a quarter layer clear of every rank boundary so that the engine's ownership at its
    # last rebuild cannot differ from this
    if name.startswith("empty_rank"):
        assert owners0 == [True] + [False] * (P - 1)
        assert lay.min() > caps[1]["z0"] + 0.25 and lay.max() < caps[1]["z0"] + caps[1]["ncz"] - 0.25      # rank 0 emptied, rank 1 filled
    else:
        assert owners0[0] and owners0[-1] and not any(owners0[1:-1])
        assert lay.min() > 0.25 and lay.max() < caps[0]["ncz"] - 0.25                                      # all on rank 0 now
        assert (o.get_state("IMAGE")[:, 2] == 1).sum() >= 30                                               # through the periodic face
    final = dict(spec, pos=o.get_state("POS"))
    for c in H.slab_capacities(final, P):              # the arrivals fit as well
        assert c["n_real"] < c["cap"] - 2 * c["G"] and c["max_layer"] < c["G"]


def test_oracle_equals_numpy_on_the_cluster_in_the_big_box(make_oracle):
    spec = H.cluster_spec()
    assert 40 <= spec["n"] <= 80 and spec["nc"] == [38, 38, 38]
    o = make_oracle()
    W.apply(spec, o)
    _check_static(o, spec, H.geometry_reference("cluster"))
