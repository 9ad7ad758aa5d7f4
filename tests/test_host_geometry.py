"""CPU-only tests of the planning rules of chemlab_amd/csrc/chem_geom_host.hpp: cells, slab layout, list skin, row stride,
tile plan, growth after an overflow, tile order, segment shift, tile layers -- what CtxT (chem_api.hip) calls between its
allocations and launches.  Each is compared with a model written here or with the independent Python statements of the
same rule (helpers.slab_capacities, multigpu.slab_layers, multigpu.owner_of).  The harness is compiled with g++ from
tests/host/; tests/test_gpu_geometry.py pins on a device that CtxT runs this plan."""
import math
import struct

import numpy as np
import pytest

import helpers as H
from chemlab_amd import multigpu
from chemlab_amd import workloads as W

EINVAL, ENOSPC = "-1", "-2"
WIDE = 1 << 20          # Box::xs_nb when no tile is narrow


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return H.compile_geometry_harness(tmp_path_factory.mktemp("host"))


def ints(words):
    return [int(w) for w in words[1:]]


def ceil_div(a, b):
    return -(-a // b)


def check_xrange(harness, nx, nb, w):
    """tile_xrange covers 0..nx without gap or overlap; returns the tile widths."""
    out = H.run_harness(harness, ["xrange %d %d %d" % (nx, nb, w)])[0]
    ranges = [tuple(int(v) for v in t.split(":")) for t in out[2:]]
    assert len(ranges) == int(out[1])
    at = 0
    for cx0, hx in ranges:
        assert cx0 == at and hx > 0, (nx, nb, w, ranges)
        at += hx
    assert at == nx, (nx, nb, w, ranges)
    return [hx for _, hx in ranges]


# ---- the ladder of cell counts ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("frac", [0.5, 0.0])
@pytest.mark.parametrize("nc", H.LADDER_BOXES, ids=lambda nc: "%dx%dx%d" % nc)
def test_ladder_cells_and_tiles(harness, nc, frac):
    spec = H.ladder_spec(nc, frac, "uniform")
    rl = spec["rc"] + spec["skin"]
    cells, plan, plan0 = H.run_harness(harness, ["cells " + " ".join(H.dbits(v) for v in spec["box"] + [rl]), H.plan_line(spec), H.plan_line(spec, tiles=0)])
    assert ints(cells) == ([1] + spec["nc"] if min(nc) >= 3 else [0, 0, 0, 0])
    assert spec["nc"] == list(nc)
    ntiles, ncx, nwide, w, rows, cap, use, S, z0, ncz = ints(plan)
    assert (use, ntiles > 0) == ((1, True) if min(nc) >= 5 else (0, False))
    assert ncx == (nc[0] if min(nc) >= 3 else 0)
    if use:
        assert ntiles == ceil_div(nc[0], 3) * ceil_div(nc[1], 3) * ceil_div(nc[2], 3)
        assert (nwide, w, rows) == (ceil_div(nc[0], 3), 1, ceil_div(nc[1], 3) * ceil_div(nc[2], 3))
        assert cap == max(1024, (int(125 * (spec["n"] / (nc[0] * nc[1] * nc[2])) * 1.12) + 64 + 255) // 256 * 256)
        assert check_xrange(harness, nc[0], WIDE, 1) == [3] * (nc[0] // 3) + [nc[0] % 3] * (nc[0] % 3 > 0)
    else:
        assert (nwide, rows, cap) == (0, 0, 0)
    assert ints(plan0)[:6] == [0, ncx, 0, 1, 0, 0] and ints(plan0)[6] == 0       # tiles=0: no tiles


def test_narrow_tiles_of_the_12_cell_row(harness):
    spec = H.ladder_spec((12, 5, 5), 0.5, "uniform")
    ntiles, ncx, nwide, w, rows, cap = ints(H.run_harness(harness, [H.plan_line(spec, tile_split=11)])[0])[:6]
    assert (ncx, nwide, w, rows) == (12, 1, 1, 4) and ntiles == 4 * (1 + 9)
    assert check_xrange(harness, 12, 1, 1) == [3] + [1] * 9


@pytest.mark.parametrize("split", [11, 2, 21])
def test_narrow_tiles_of_the_7_cell_box(harness, split):
    """The relation tests/test_gpu_round3.py::test_narrow_tiles_change_nothing asserts of chem_debug_tiles."""
    spec = W.reactive_melt(n=8788, seed=61, interval=20)
    ntiles, nx, nwide, w, rows, cap = ints(H.run_harness(harness, [H.plan_line(spec, tile_split=split)])[0])[:6]
    assert nx == 7 and nwide == split // 10 and w == split % 10
    assert rows == 9 and ntiles == rows * (nwide + -(-(nx - 3 * nwide) // w))
    assert check_xrange(harness, nx, nwide, w) == [3] * nwide + [w] * ((nx - 3 * nwide) // w) + [(nx - 3 * nwide) % w] * ((nx - 3 * nwide) % w > 0)


# ---- slabs --------------------------------------------------------------------------------------------------------------------

def test_slab_partition_is_multigpu_slab_layers(harness):
    script, want = [], []
    for nzg in range(4, 41):
        for P in range(1, 9):
            try:
                layers = multigpu.slab_layers(nzg, P)
            except ValueError:
                layers = None
            for rk in range(P):
                script.append("slab %d %d %d" % (nzg, P, rk))
                want.append(None if layers is None else [layers[rk][1] - layers[rk][0], layers[rk][0], (rk - 1) % P, (rk + 1) % P])
    assert any(w is None for w in want) and any(w is not None and w[0] == 2 for w in want)
    for line, out, w in zip(script, H.run_harness(harness, script), want):
        if w is None:
            assert out[:2] == ["error", EINVAL] and "fewer than 2 cell layers" in " ".join(out), (line, out)
        else:
            assert out[0] == "slab" and ints(out) == w, (line, out, w)


def test_slab_needs_cells_on_every_axis(harness):
    spec = dict(H.ladder_spec((2, 7, 7), 0.5, "uniform"))
    out = H.run_harness(harness, [H.plan_line(spec, dd=1)])[0]
    assert out[:2] == ["error", EINVAL] and "at least 3 cells" in " ".join(out)


@pytest.mark.parametrize("name", sorted(H.SLAB_CASES))
def test_slab_capacities_are_helpers_slab_capacities(harness, name):
    spec = H.slab_spec(name)
    nzg = spec["nc"][2]
    for P in H.SLAB_CASES[name][4]:
        caps = H.slab_capacities(spec, P)
        plans = H.run_harness(harness, [H.plan_line(spec, dd=1, P=P, rk=rk) for rk in range(P)])
        for rk in range(P):
            z0, ncz = ints(plans[rk])[8:10]
            assert (z0, ncz) == (caps[rk]["z0"], caps[rk]["ncz"])
            G, mcap, cap = ints(H.run_harness(harness, ["caps %d %d %d" % (spec["n"], nzg, ncz)])[0])
            assert (G, mcap, cap) == (caps[rk]["G"], caps[rk]["mcap"], caps[rk]["cap"])


@pytest.mark.parametrize("nz,P", [(23, 1), (23, 2), (23, 3), (40, 8), (7, 3)])
def test_layer_of_a_coordinate_is_multigpu_owner_of(harness, nz, P):
    rc, skin = 2.0, 0.3
    Lz = (nz + 0.5) * (rc + skin)
    rng = np.random.default_rng(900 + nz + P)
    z = np.concatenate([rng.uniform(-2 * Lz, 3 * Lz, 600), [0.0, Lz, -Lz, 2 * Lz, -0.0, np.nextafter(Lz, 0.0), 0.5 * Lz]])
    assert (z < 0).any() and (z >= Lz).any()
    layer = np.array(ints(H.run_harness(harness, ["layer %s %d %d " % (H.dbits(Lz), nz, len(z)) + " ".join(H.dbits(v) for v in z)])[0]))
    zf = z - np.floor(z / Lz) * Lz                           # (helpers.slab_capacities' statement of the fold)
    assert np.array_equal(layer, np.clip(np.floor(zf * nz / Lz).astype(int), 0, nz - 1))
    bounds = np.array([a for a, _ in multigpu.slab_layers(nz, P)] + [nz])
    assert np.array_equal(np.searchsorted(bounds, layer, side="right") - 1, multigpu.owner_of(z, Lz, rc, skin, P))


# ---- list skin ------------------------------------------------------------------------------------------------------------------

def model_list_skin(L, rc, skin, opt, criterion, tiles, fused, dd, P, npart):
    if opt == 0.0 or criterion != 0 or not tiles or (not dd and not fused):
        return 0.0
    edge = 1e300
    for d in range(3):
        nc = math.floor(L[d] / (rc + opt if opt > 0 else rc + skin))
        if opt < 0:
            if npart < 100000:
                return 0.0
            nc -= 2
        if nc < 5 or (dd and d == 2 and nc // P < 2):
            return 0.0
        edge = min(edge, L[d] / nc)
    s = edge * (1.0 - 1e-9) - rc
    return s if s > skin else 0.0


BENCH_L = (1e6 / 0.8) ** (1.0 / 3.0)      # the benchmark: 10^6 particles at density 0.8
SKIN_CASES = {
    #                 L                              opt  criterion tiles fused dd P npart
    "option_0": ([BENCH_L] * 3, 0.0, 0, 1, 1, 0, 1, 1000000),
    "explicit": ([BENCH_L] * 3, 0.45, 0, 1, 1, 0, 1, 5000),
    "explicit_below_the_skin": ([BENCH_L] * 3, 0.2, 0, 1, 1, 0, 1, 5000),
    "automatic_small_system": ([30.0] * 3, -1.0, 0, 1, 1, 0, 1, 99999),
    "automatic_benchmark": ([BENCH_L] * 3, -1.0, 0, 1, 1, 0, 1, 1000000),
    "displacement_criterion": ([BENCH_L] * 3, -1.0, 1, 1, 1, 0, 1, 1000000),
    "unfused_single_domain": ([BENCH_L] * 3, -1.0, 0, 1, 0, 0, 1, 1000000),
    "unfused_slab": ([BENCH_L] * 3, -1.0, 0, 1, 0, 1, 2, 1000000),
    "slab_with_two_layers_left": ([BENCH_L, BENCH_L, 9.5 * 2.8], -1.0, 0, 1, 1, 1, 3, 1000000),
    "slab_wider_skin_leaves_one_layer": ([BENCH_L, BENCH_L, 9.5 * 2.8], -1.0, 0, 1, 1, 1, 4, 1000000),
}


@pytest.mark.parametrize("case", sorted(SKIN_CASES))
def test_list_skin(harness, case):
    rc, skin = 2.5, 0.3
    L, opt, crit, tiles, fused, dd, P, npart = SKIN_CASES[case]
    out = H.run_harness(harness, ["skin " + " ".join(H.dbits(v) for v in L + [rc, skin, opt]) + " %d %d %d %d %d %d" % (crit, tiles, fused, dd, P, npart)])[0]
    got = struct.unpack("<d", struct.pack("<Q", int(out[1])))[0]
    assert got == model_list_skin(L, rc, skin, opt, crit, tiles, fused, dd, P, npart)
    zero = case in ("option_0", "explicit_below_the_skin", "automatic_small_system", "displacement_criterion", "unfused_single_domain",
                    "slab_wider_skin_leaves_one_layer")
    assert (got == 0.0) == zero, (case, got)
    if case == "automatic_benchmark":      # 38 cells of 2.8 per axis -> 36 cells, the whole edge of one is the list cutoff
        assert math.floor(BENCH_L / (rc + skin)) == 38 and got == pytest.approx(BENCH_L / 36 - rc, rel=1e-8)
        assert ints(H.run_harness(harness, ["cells " + " ".join(H.dbits(v) for v in L + [rc + got])])[0]) == [1, 36, 36, 36]


# ---- row stride and growth ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("npart,user", [(1000000, 0), (8788, 0), (8788, 100), (8788, 97), (10, 0), (10, 500), (1, 0), (2, 0)])
def test_row_stride(harness, npart, user):
    L, rl = [BENCH_L, 0.5 * BENCH_L, 2 * BENCH_L], 2.8
    S = ints(H.run_harness(harness, ["stride " + " ".join(H.dbits(v) for v in L + [rl]) + " %d %d" % (npart, user)])[0])[0]
    expect = 4.0 / 3.0 * math.pi * rl * rl * rl * npart / (L[0] * L[1] * L[2])
    ncap = min(user if user > 0 else int(expect * 1.6 + 48), max(npart - 1, 1))
    assert S == (ncap + 15) // 16 * 16 and S % 16 == 0 and S >= 16
    if user > 0 and user <= npart - 1:
        assert user <= S < user + 16           # the user's capacity honoured
    assert S < max(npart - 1, 1) + 16          # never more rows than other particles (rounded up)


@pytest.mark.parametrize("nmax", [1000000, 1000])
@pytest.mark.parametrize("ov", [1, 255, 256, 1537, 5000])
def test_growth_after_overflow(harness, ov, nmax):
    cap, S = ints(H.run_harness(harness, ["grow %d %d" % (ov, nmax)])[0])
    assert cap == (ov + ov // 8 + 255) // 256 * 256 and cap % 256 == 0 and cap > ov
    clamp = max((nmax + 15) // 16 * 16, 16)
    assert S == min((int(ov * 1.25) + 31) // 16 * 16, clamp) and S % 16 == 0
    assert S > ov or S == clamp
    assert (S == clamp) == (nmax == 1000 and ov >= 1537)


# ---- LDS fit, with a linear byte model ------------------------------------------------------------------------------------------

def test_lds_fit(harness):
    box = [5.5 * 2.3] * 3                                    # 5 cells per axis: one stencil = the whole box
    thin = dict(box=box, rc=2.0, skin=0.3, n=1000, rebuild_criterion=1)
    dense = dict(thin, n=8000)                               # 64 per cell: (int)(125 * 64 * 1.12) + 64 = 9024 -> 9216 slots
    budget = 150 * 1024
    fit, off, slab_fit, slab_off = H.run_harness(harness, [H.plan_line(thin, bytes_per_slot=22, budget=budget), H.plan_line(dense, bytes_per_slot=22, budget=budget),
                                                           H.plan_line(thin, dd=1, bytes_per_slot=22, budget=budget), H.plan_line(dense, dd=1, bytes_per_slot=22, budget=budget)])
    assert 1280 * 22 < budget < 9216 * 22
    assert ints(fit)[:7] == [8, 5, 2, 1, 4, 1280, 1]
    assert ints(off)[:7] == [0, 5, 0, 1, 0, 9216, 0]        # single domain: the per-cell kernels take over
    assert ints(slab_fit)[:7] == [8, 5, 2, 1, 4, 1280, 1]
    assert slab_off[:2] == ["error", ENOSPC] and "does not fit the LDS" in " ".join(slab_off)
    # the other errors of a slab: too few cells along x or y, tiles=0
    narrow = dict(thin, box=[4.5 * 2.3, 5.5 * 2.3, 5.5 * 2.3])
    few, no_tiles = H.run_harness(harness, [H.plan_line(narrow, dd=1), H.plan_line(thin, dd=1, tiles=0)])
    assert few[:2] == ["error", EINVAL] and ">= 5 cells along x and y" in " ".join(few)
    assert no_tiles[:2] == ["error", EINVAL] and "tiles=0 is a single-domain switch" in " ".join(no_tiles)


# ---- tile order -----------------------------------------------------------------------------------------------------------------

def model_home_cells(nc, nb_opt, w, tile):
    nb = ceil_div(nc[0], 3) if nb_opt * 3 >= nc[0] else nb_opt
    ntx = nb if nb * 3 >= nc[0] else nb + ceil_div(nc[0] - nb * 3, w)
    nty = ceil_div(nc[1], 3)
    tx, ty, tz = tile % ntx, (tile // ntx) % nty, tile // (ntx * nty)
    cx0, hx = (3 * tx, 3) if tx < nb else (nb * 3 + (tx - nb) * w, w)
    return min(hx, nc[0] - cx0) * min(3, nc[1] - 3 * ty) * min(3, nc[2] - 3 * tz), ntx * nty * ceil_div(nc[2], 3)


@pytest.mark.parametrize("nc,nb,w", [((5, 6, 7), WIDE, 1), ((5, 5, 23), WIDE, 1), ((12, 5, 5), 1, 1), ((12, 5, 5), 2, 2)])
def test_tile_order(harness, nc, nb, w):
    ntiles = model_home_cells(nc, nb, w, 0)[1]
    out = ints(H.run_harness(harness, ["order %d %d %d %d %d %d" % (nc + (nb, w, ntiles))])[0])
    assert out[0] == ntiles and len(out) == 1 + 2 * ntiles
    ord_, pos = out[1:1 + ntiles], out[1 + ntiles:]
    assert sorted(ord_) == list(range(ntiles))
    assert [pos[t] for t in ord_] == list(range(ntiles))
    home = [model_home_cells(nc, nb, w, t)[0] for t in range(ntiles)]
    assert len(set(home)) > 1
    off = 0
    for x in range(8):
        cnt = ntiles // 8 + (1 if x < ntiles % 8 else 0)
        part = ord_[off:off + cnt]
        assert sorted(part) == list(range(off, off + cnt))                                      # a range keeps its tiles
        assert part == sorted(part, key=lambda t: (-home[t], t))                                # most home cells first, stable
        off += cnt


def test_tile_order_needs_eight_tiles(harness):
    few, eight = H.run_harness(harness, ["order 5 5 3 %d 1 4" % WIDE, "order 5 5 5 %d 1 8" % WIDE])
    assert ints(few) == [0] and ints(eight)[0] == 8


# ---- segment shift, tile layers -----------------------------------------------------------------------------------------------

def test_segment_shift(harness):
    cases = [(n, lo, 1024) for lo in (6, 0) for n in (0, 1, 63, 64, 1023, 1024, 1025, 65536, 65537, 46656, 54872, 1 << 20, (1 << 20) + 1, 3000000)]
    for (n, lo, mx), out in zip(cases, H.run_harness(harness, ["shift %d %d %d" % c for c in cases])):
        sh = lo
        while ceil_div(n, 1 << sh) > mx:
            sh += 1
        assert ints(out) == [sh], (n, lo)


def test_tile_layers_and_overlap(harness):
    cases = [(ntiles, ntxy) for ntxy in (4, 144) for ntiles in (ntxy, 2 * ntxy, 3 * ntxy, 8 * ntxy, 60 * ntxy)]
    out = H.run_harness(harness, ["layers %d %d %d" % (c + (which,)) for c in cases for which in (0, 1, 2)])
    for k, (ntiles, ntxy) in enumerate(cases):
        allt, interior, boundary = (ints(l) for l in out[3 * k:3 * k + 3])
        assert allt == [0, ntiles, 0, ntiles]
        assert interior == [ntxy, ntiles - 2 * ntxy, 0, ntiles - 2 * ntxy]                      # every layer but the lowest and the highest
        assert boundary == [0, ntxy, ntiles - ntxy, 2 * ntxy]
    script, want = [], []
    for opt in (-1, 0, 1):
        for use in (0, 1):
            for ntiles, ntxy in cases:
                for polls in (0, 1):
                    script.append("overlap %d %d %d %d %d" % (opt, use, ntiles, ntxy, polls))
                    want.append(int((opt > 0 or (opt < 0 and ntiles >= 8192)) and use == 1 and ntiles > 2 * ntxy and polls == 1))
    assert [ints(l)[0] for l in H.run_harness(harness, script)] == want and 0 < sum(want) < len(want)
