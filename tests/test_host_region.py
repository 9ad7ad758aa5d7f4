"""Region rules, host side: chemlab_amd/csrc/chem_region_host.hpp (box test, firing rule, selection over the compacted
records, validation, the quota the device decides by) against tests/region_ref.py on seeded random sets.  Nothing here needs a
GPU.  The harness is compiled with g++ from tests/host/, once more with -fsanitize=address,undefined as a stand-alone program."""
import os
import subprocess

import numpy as np
import pytest

import region_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def build(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include")] + flags +
                          [os.path.join(ROOT, "tests", "host", "region_harness.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if request.param == "plain":
        return build(tmp_path_factory.mktemp("host"), "region_harness", ["-O1"])
    return build(tmp_path_factory.mktemp("host_san"), "region_harness_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def drive(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    return [x for x in out.stdout.split("\n") if x]


def rule_line(r):
    return "rule %s %s %d %d %d %d %r %d %d %d" % (" ".join(repr(float(v)) for v in r["lo"]), " ".join(repr(float(v)) for v in r["hi"]),
                                                    r["target_type"], r["new_type"], r["interval"], r["mode"], float(r["value"]), r["num"],
                                                    r["seed"], 1 if r["enabled"] else 0)


def fire_lines(step, box, tags, types, pos):
    return ["fire %d %r %r %r %d" % (step, box[0], box[1], box[2], len(tags))] + \
           ["%d %d %r %r %r" % (t, ty, float(p[0]), float(p[1]), float(p[2])) for t, ty, p in zip(tags, types, pos)]


def parse_fire(out, k):
    n = int(out[k].split()[1]); chg = [tuple(int(v) for v in out[k + 1 + j].split()) for j in range(n)]; k += 1 + n
    m = int(out[k].split()[1]); st = [tuple(int(v) for v in out[k + 1 + j].split()) for j in range(m)]; k += 1 + m
    types = [int(v) for v in out[k].split()[1:]]
    return chg, st, types, k + 1


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_firing_against_the_reference(harness, seed):
    rng = np.random.default_rng(seed)
    box = [6.0, 4.5, 7.5]
    w = 0.75
    rules = []
    for d in range(3):      # six slabs at the box edges, modes mixed, plus a whole-box rule by count that feeds on an earlier one
        for side in (0, 1):
            lo, hi = [0.0, 0.0, 0.0], list(box)
            if side == 0:
                hi[d] = w
            else:
                lo[d] = box[d] - w
            mode = int(rng.integers(0, 4))
            rules.append(G.rule(lo, hi, 1, 4 + d, interval=int(rng.integers(1, 4)), mode=mode, value=float(rng.choice([0.0, 0.3, 0.5, 0.999, 1.0])),
                                num=int(rng.integers(0, 6)), seed=int(rng.integers(0, 2 ** 63)), enabled=bool(rng.random() < 0.85)))
    rules.append(G.rule([0, 0, 0], box, 4, 1, interval=2, mode=G.MODE_NUM, num=2, seed=5))
    n = 150
    tags = rng.permutation(400)[:n]      # arbitrary order, as the device's records come
    types = rng.choice([0, 1, 1, 1, 4], n)
    lines = [rule_line(r) for r in rules]
    want = []
    cur = np.zeros(400, np.int64); cur[tags] = types
    for step in range(0, 7):
        pos = rng.uniform(-3.0, 10.0, (n, 3))
        pos[:6] = [[0.75, 1, 1], [0.0, 1, 1], [6.0, 1, 1], [5.25, 1, 1], [np.nextafter(0.75, 0), 2, 2], [12.0, 4.5, 15.0]]      # on the faces
        lines += fire_lines(step, box, tags, cur[tags], pos)
        full = np.full((400, 3), 3.0); full[tags] = G.fold(pos, np.array(box))
        present = np.zeros(400, bool); present[tags] = True
        ty = np.where(present, cur, -1)
        ch, st = G.fire(rules, step, full, ty)
        cur = np.where(present, ty, cur)
        want.append((ch, st, cur[tags].tolist()))
    out = drive(harness, lines)
    assert [o.split()[1] for o in out[:len(rules)]] == [str(k) for k in range(len(rules))]
    k = len(rules)
    total = 0
    for ch, st, ty in want:
        gch, gst, gty, k = parse_fire(out, k)
        assert gch == ch and gst == st and gty == ty
        total += len(ch)
    assert total > 10      # guard: the cases did change something


def test_validation(harness):
    good = G.rule([0, 0, 0], [1, 1, 1], 1, 2)
    bad = []
    for key, val in (("target_type", -1), ("target_type", 16), ("new_type", 16), ("new_type", -1), ("interval", 0), ("mode", 4), ("mode", -1)):
        r = dict(good); r[key] = val; bad.append(r)
    r = dict(good); r["lo"] = np.array([2.0, 0, 0]); bad.append(r)
    r = dict(good); r["hi"] = np.array([1.0, np.inf, 1]); bad.append(r)
    r = dict(good); r["lo"] = np.array([np.nan, 0, 0]); bad.append(r)
    for mode in (G.MODE_PROB, G.MODE_FRACTION):
        for v in (-0.1, 1.5):
            r = dict(good); r["mode"] = mode; r["value"] = v; bad.append(r)
    r = dict(good); r["mode"] = G.MODE_NUM; r["num"] = -1; bad.append(r)
    ok = [dict(good, lo=np.array([1.0, 1, 1])), dict(good, mode=G.MODE_NUM, num=0), dict(good, mode=G.MODE_ALL, value=7.0)]
    out = drive(harness, [rule_line(r) for r in bad + ok])
    assert [o.split()[1] for o in out] == [str(EINVAL)] * len(bad) + ["0", "1", "2"]


def test_binding_structs_match_the_header(tmp_path):
    import ctypes as C
    from chemlab_amd import _capi
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "chem_mi355.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %d\\n", sizeof(chem_region_desc), offsetof(chem_region_desc, new_mass), offsetof(chem_region_desc, value),\n'
                   '         offsetof(chem_region_desc, seed), sizeof(chem_region_change), sizeof(chem_region_stats), CHEM_MAX_REGIONS);\n  return 0;\n}\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    D = _capi.RegionDesc
    assert got == [C.sizeof(D), D.new_mass.offset, D.value.offset, D.seed.offset, C.sizeof(_capi.RegionChange), C.sizeof(_capi.RegionStats), _capi.CHEM_MAX_REGIONS]
    api = _capi.load()
    assert all(hasattr(api, n) for n in ("region_add", "region_enable", "region_get_changes", "region_get_stats", "region_counters"))


def test_quota_is_the_reference_count(harness):
    cases = [(0, 0.0, 0, 5, 0, 5), (1, 0.5, 0, 9, 4, 4), (2, 0.0, 3, 2, 0, 2), (2, 0.0, 3, 8, 0, 3), (2, 0.0, 0, 8, 0, 0),
             (3, 0.999, 0, 3, 0, 2), (3, 0.33, 0, 3, 0, 0), (3, 1.0, 0, 7, 0, 7), (3, 0.0, 0, 7, 0, 0)]
    out = drive(harness, ["quota %d %r %d %d %d" % c[:5] for c in cases])
    assert [int(o.split()[1]) for o in out] == [c[5] for c in cases]
    for mode, value, num, nc, na, q in cases:
        if mode >= 2:
            assert G.quota(dict(mode=mode, value=value, num=num), nc) == q
