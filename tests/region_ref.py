"""Region rules (include/chem_mi355.h, chem_region_add ff.; FreezeRegion, ChangeParticleType) restated in numpy / plain Python:
the box test on folded positions, the firing rule, the order of rules, the four selection modes and the draw (region_draw of
include/chem_philox.h, restated with philox_py as react_ref.atrp_draw is).  The positions are given per step (the engine's
own, read back with CHEM_STATE_POS); what comes out are the changes, the stats and the types."""
import math

import numpy as np

from test_philox import philox_py

MODE_ALL, MODE_PROB, MODE_NUM, MODE_FRACTION = 0, 1, 2, 3
M32 = 0xffffffff


def region_draw(seed, step, tag, rule):
    ctr = (tag & M32, step & M32, (step >> 32) & M32, (0x5245474E ^ (rule << 8)) & M32)
    key = ((seed & M32) ^ 0x52474E53, (seed >> 32) & M32)
    return tuple(philox_py(ctr, key))


def u01(x):
    return (float(x) + 0.5) * (1.0 / 4294967296.0)


def rule(lo, hi, target_type, new_type, interval=1, mode=MODE_ALL, value=0.0, num=0, seed=0, enabled=True):
    return dict(lo=np.asarray(lo, float), hi=np.asarray(hi, float), target_type=target_type, new_type=new_type, interval=interval,
                mode=mode, value=value, num=num, seed=seed, enabled=enabled)


def fold(pos, box):
    """what chem_get_state(CHEM_STATE_POS) does to a decoded coordinate"""
    pos, box = np.asarray(pos, float), np.asarray(box, float)
    x = pos - np.floor(pos / box) * box
    return np.where(x >= box, x - box, x)


def inside(r, pos):
    return np.all((r["lo"] <= pos) & (pos < r["hi"]), axis=-1)


def due(r, step):
    return r["enabled"] and step > 0 and step % r["interval"] == 0


def quota(r, ncand):
    if r["mode"] == MODE_NUM:
        return min(r["num"], ncand)
    return int(math.floor(r["value"] * float(ncand)))


def pick(r, k, step, cand):
    """the tags of `cand` that rule r (index k) changes at `step`, ascending"""
    cand = sorted(int(t) for t in cand)
    if r["mode"] == MODE_ALL:
        return cand
    draws = {t: region_draw(r["seed"], step, t, k) for t in cand}
    if r["mode"] == MODE_PROB:
        return [t for t in cand if u01(draws[t][1]) < r["value"]]
    order = sorted(cand, key=lambda t: (draws[t][0], t))
    return sorted(order[:quota(r, len(cand))])


def fire(rules, step, pos, types):
    """One step: `pos` folded (n, 3), `types` (n,) is updated in place.  Returns (changes [(step, tag, rule)], stats
    [(step, rule, candidates, changed)]); rules in insertion order, a later rule sees the types an earlier one left."""
    changes, stats = [], []
    for k, r in enumerate(rules):
        if not due(r, step):
            continue
        cand = np.nonzero((types == r["target_type"]) & inside(r, pos))[0]
        if len(cand) == 0:
            continue
        hit = pick(r, k, step, cand)
        if not hit:
            continue
        types[hit] = r["new_type"]
        changes += [(step, t, k) for t in hit]
        stats.append((step, k, len(cand), len(hit)))
    return changes, stats


def run(rules, pos_by_step, types, box):
    """pos_by_step: {step: positions as read back}.  Returns (changes, stats, final types)."""
    types = np.array(types, dtype=np.int64)
    changes, stats = [], []
    for step in sorted(pos_by_step):
        c, s = fire(rules, step, fold(pos_by_step[step], box), types)
        changes += c
        stats += s
    return changes, stats, types
