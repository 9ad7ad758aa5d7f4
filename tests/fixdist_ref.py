"""Fixed distances / by-product release (include/chem_mi355.h, chem_fix_create ff.): the rule set restated in plain numpy and
plain Python.  Imports nothing from the product.

Per step, behind the drift, for every live entry (a, t, d):
    u = minimum image of x_t - x_a;  u = (1, 0, 0) if |u| = 0 else u / |u|;  x_t <- x_a + d u (same periodic image as before);
    v_t <- v_a (the anchor's half-step velocity).
Sets keep their entries in insertion order; a release removes entries, keeps the order of the others and logs
(step, set, anchor, target, cause); the records of one step are ordered by (set, insertion index)."""
import numpy as np

CAUSE_REACTION, CAUSE_TYPE = 1, 2
MAX_SETS = 8


def min_image(d, box):
    box = np.asarray(box, dtype=np.float64)
    return d - box * np.rint(d / box)


def constrain(xa, xt, d, box):
    """new unfolded position of the target: at distance d from the anchor along the minimum-image direction, on the periodic
    image it was on"""
    box = np.asarray(box, dtype=np.float64)
    sep = xt - xa
    shift = box * np.rint(sep / box)
    r = sep - shift
    nrm = np.sqrt((r * r).sum(-1, keepdims=True))
    e1 = np.zeros_like(r)
    e1[..., 0] = 1.0
    u = np.where(nrm > 0, r / np.where(nrm > 0, nrm, 1.0), e1)
    return xa + np.asarray(d)[..., None] * u + shift


def step_model(x, v, f, m, dt, entries, box):
    """One velocity-Verlet step as far as the read-backs before the call decide it: x (unfolded), v, f (the forces current
    at the step), m.  entries: rows (anchor index, target index, d).  Returns (x after the drift and the constraint, the
    half-step velocities after the constraint); the caller adds the second half kick with the forces read after the call."""
    vh = v + 0.5 * dt * f / m[:, None]
    xn = x + dt * vh
    if len(entries):
        a = np.array([e[0] for e in entries]); t = np.array([e[1] for e in entries]); d = np.array([e[2] for e in entries], dtype=np.float64)
        xn[t] = constrain(xn[a], xn[t], d, box)
        vh[t] = vh[a]
    return xn, vh


def distances(x, entries, box):
    a = np.array([e[0] for e in entries]); t = np.array([e[1] for e in entries])
    r = min_image(x[t] - x[a], box)
    return np.sqrt((r * r).sum(-1))


class Sets:
    """The host bookkeeping: sets, entries (anchor, target, dist, seq), release rules, the log."""

    def __init__(self, nparticles):
        self.n = nparticles
        self.sets = []          # dict(anchor_type, target_type, ent=[[a, t, d, seq]], next_seq)
        self.rules = []         # (reaction, role, set, count)
        self.log = []           # (step, set, a, t, cause, seq)

    def create(self, anchor_type=-1, target_type=-1):
        if len(self.sets) >= MAX_SETS:
            return None
        self.sets.append(dict(anchor_type=anchor_type, target_type=target_type, ent=[], next_seq=0))
        return len(self.sets) - 1

    def _targets(self):
        return {e[1] for s in self.sets for e in s["ent"]}

    def _anchors(self):
        return {e[0] for s in self.sets for e in s["ent"]}

    def add(self, h, pairs, dist):
        """True if accepted; all or nothing"""
        if not (0 <= h < len(self.sets)) or not (dist > 0.0) or not np.isfinite(dist):
            return False
        targets, anchors = self._targets(), self._anchors()
        for a, t in pairs:
            if not (0 <= a < self.n and 0 <= t < self.n) or a == t:
                return False
            if t in targets or t in anchors or a in targets:
                return False
            targets.add(t); anchors.add(a)
        s = self.sets[h]
        for a, t in pairs:
            s["ent"].append([a, t, dist, s["next_seq"]]); s["next_seq"] += 1
        return True

    def _release(self, picked, step, cause):
        """picked: set of (set, seq)"""
        recs = []
        for h, s in enumerate(self.sets):
            keep = []
            for e in s["ent"]:
                if (h, e[3]) in picked:
                    recs.append((step, h, e[0], e[1], cause, e[3]))
                else:
                    keep.append(e)
            s["ent"] = keep
        self.log.extend(recs)
        self.log.sort(key=lambda r: (r[0], r[1], r[5]))
        return [r[:5] for r in recs]

    def release_by_reaction(self, reactants, step):
        """reactants: (reaction, role, particle) in the order the releases are taken"""
        picked = set()
        for reaction, role, p in reactants:
            for rr, ro, h, count in self.rules:
                if rr != reaction or ro != role:
                    continue
                left = count
                for e in self.sets[h]["ent"]:
                    if left > 0 and e[0] == p and (h, e[3]) not in picked:
                        picked.add((h, e[3])); left -= 1
        return self._release(picked, step, CAUSE_REACTION)

    def release_by_type(self, types, step):
        picked = set()
        for h, s in enumerate(self.sets):
            at, tt = s["anchor_type"], s["target_type"]
            if at < 0 and tt < 0:
                continue
            for e in s["ent"]:
                if (at >= 0 and types[e[0]] != at) or (tt >= 0 and types[e[1]] != tt):
                    picked.add((h, e[3]))
        return self._release(picked, step, CAUSE_TYPE)

    def entries(self, h):
        return [tuple(e) for e in self.sets[h]["ent"]]

    def records(self):
        return [r[:5] for r in self.log]
