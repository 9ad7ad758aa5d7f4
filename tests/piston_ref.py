"""The Langevin piston barostat restated in fp64 (include/chem_mi355.h chem_barostat_langevin): the reference of
tests/test_piston_ref.py, tests/test_host_piston.py (CPU) and tests/test_gpu_piston.py (device).  No engine in here.

State between steps: x, v, L, the forces f at (x, L) and the piston momentum pe (a half-step quantity).  One step, with
eps_dot = pe / W, c = 1 + 3 / N_f (N_f = 3 n), sv = exp(-c eps_dot dt / 2), mu = exp(eps_dot dt):

    v <- sv v;  v <- v + dt f / 2m            x <- mu (x + dt v / sqrt(mu));  L <- mu L
    f <- forces at (x, L) (+ the thermostat's share, from the velocities of this point)
    v <- v + dt f / 2m;  v <- sv v
    P = (sum m v^2 + W_vir) / 3V
    G = 3V (P - P0) + (3 / N_f) sum m v^2 - gammaP pe + sqrt(24 gammaP W kT / dt) (u - 1/2);   pe <- pe + dt G

u = u01(barostat_draw(seed, step)[0]), `step` the number of the step that has just been counted.

With gammaP = 0 and no thermostat, H = sum m v^2 / 2 + U + P0 V + (pe + dt G / 2)^2 / 2W, evaluated behind the step with that
step's G (the momentum at the full step), is conserved to O(dt^2)."""
import numpy as np

import aged_ref
from test_philox import philox_py


def u01(x):
    return (float(x) + 0.5) * (1.0 / 4294967296.0)


def barostat_draw(seed, step):
    """chem_philox::barostat_draw: a counter domain and a key constant of its own, one draw per step."""
    seed, step = int(seed) & 0xffffffffffffffff, int(step) & 0xffffffffffffffff
    ctr = (0, step & 0xffffffff, (step >> 32) & 0xffffffff, 0x50495354)
    key = ((seed & 0xffffffff) ^ 0x4241524F, (seed >> 32) & 0xffffffff)
    return philox_py(ctr, key)


def piston_sv(pe, W, nf, dt):
    return float(np.exp(-0.5 * (1.0 + 3.0 / nf) * (pe / W) * dt))


def piston_mu(pe, W, dt):
    return float(np.exp((pe / W) * dt))


def piston_force(volume, p, p0, nf, mv2, gammaP, pe, W, kT, dt, u):
    return 3.0 * volume * (p - p0) + (3.0 / nf) * mv2 - gammaP * pe + float(np.sqrt(24.0 * gammaP * W * kT / dt)) * (u - 0.5)


def piston_ok(pe, mu, sv):
    return bool(np.isfinite(pe) and np.isfinite(mu) and np.isfinite(sv) and mu > 0.0)


def energy_force_fn(spec):
    """force_fn of piston_step for a spec with non-bonded LJ terms only: (forces, W_vir, U) from aged_ref.exact_pairs."""
    def fn(x, L):
        r = aged_ref.exact_pairs(dict(spec, box=L), x)
        return r["f"], r["virial_nb"], r["epot_lj"] + r["epot_tab"]
    return fn


def piston_step(spec, x, v, f, L, pe, force_fn, dt, p0, W, gammaP, kT, seed, step, thermo_fn=None):
    """One step.  x unfolded, f the forces the step starts with (thermostat share included), `step` the number the step has
    when it is finished.  force_fn(x, L) -> (forces, W_vir[, U]); thermo_fn(v) -> the thermostat's force at the velocities
    between the two half kicks (None: no thermostat).  Returns a dict: x, v, f, L, pe (the new state), P, G, mv2, virial, volume,
    epot (None without U), sv, mu (the factors this step used), u."""
    m = np.asarray(spec["mass"], np.float64)[:, None]
    nf = 3.0 * len(m)
    with np.errstate(over="ignore", invalid="ignore"):
        sv, mu = piston_sv(pe, W, nf, dt), piston_mu(pe, W, dt)
    if not piston_ok(pe, mu, sv):
        raise ArithmeticError("Langevin barostat: pe = %g, mu = %g, sv = %g" % (pe, mu, sv))
    v = sv * np.asarray(v, np.float64)
    v = v + 0.5 * dt * np.asarray(f, np.float64) / m
    x = mu * (np.asarray(x, np.float64) + dt * v / np.sqrt(mu))
    L = mu * np.asarray(L, np.float64)
    r = force_fn(x, L)
    f, w = r[0], r[1]
    epot = r[2] if len(r) > 2 else None
    if thermo_fn is not None:
        f = f + thermo_fn(v)
    v = v + 0.5 * dt * f / m
    v = sv * v
    k = float((m * v * v).sum())
    vol = float(np.prod(L))
    p = (k + w) / (3.0 * vol)
    u = u01(barostat_draw(seed, step)[0])
    g = piston_force(vol, p, p0, nf, k, gammaP, pe, W, kT, dt, u)
    return dict(x=x, v=v, f=f, L=L, pe=pe + dt * g, P=p, G=g, mv2=k, virial=w, volume=vol, epot=epot, sv=sv, mu=mu, u=u)


def conserved(out, pe_before, dt, p0, W):
    """H behind a step: `out` is what piston_step returned (or the same quantities read from an engine), pe_before the
    momentum the step started with."""
    pe_full = pe_before + 0.5 * dt * out["G"]
    return 0.5 * out["mv2"] + out["epot"] + p0 * out["volume"] + pe_full * pe_full / (2.0 * W)
