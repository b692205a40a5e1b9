"""The plane of scale index x deviation on which the rate kernels are checked symbol by symbol, and the float64
references that stand behind that check.  TEST INFRASTRUCTURE (see oracle/__init__.py).

-log2 [Phi((v + .5)/s) - Phi((v - .5)/s)] changes regime along both axes: the log_ndtr pair switches at (v +- .5)/s = -10
(asymptotic series) and at 0, the survival pair takes over right of the median, the scale index saturates at 63, and the
scan's own formulation (csrc/entropy.hip normal_bits_fast) has its a == 0 / a >= 1 forms and subtracts two erfcx values at
large s.  ``cells()`` lists (v, raw) pairs that walk all of it, out to |v| = 5000 (|v|/s = 45 000 at s = 0.11); every value
is a float32 so that the kernels and the references read the same numbers.

    python -m oracle.rate_plane          prints the float32 floor of the reference formulation (FLOAT32_FLOOR in
                                         tests/test_hip_rate_plane.py) and the sizes of the plane
"""
from __future__ import annotations

import math

import numpy as np
import scipy.special as sp
import torch

from . import ops_np as O
from . import train_ref

F32, F64 = np.float32, np.float64
LN2 = math.log(2.0)
C0, C1 = train_ref.LOG_SCALE_MIN, train_ref.SCALE_FACTOR
LN63 = F32(math.log(63.0))                 # exp() of it is 62.99999166: two float32 steps inside the bound
SATURATED = (4.2, 4.5, 4.9)
FAR = (100.0, 200.0, 300.0, 1000.0, 2000.0, 5000.0)
SWITCH_INDEXES = (0.0, 5.0, 20.0, 40.0, 63.0)
SWITCH_ULPS = (1, 4, 64)


def raws():
    """raw = ln(idx) for 96 indexes in (0, 63], index 0 (raw = -50), float32(ln 63) and its two neighbours (the last
    unsaturated / first saturated values around it) and three saturated values."""
    idx = np.concatenate([[0.01, 0.1], np.linspace(0.5, 63.0, 94)])
    edge = [LN63, np.nextafter(LN63, F32(0)), np.nextafter(LN63, F32(9))]
    return np.unique(np.concatenate([np.log(idx).astype(F32), [F32(-50.0)], edge, np.asarray(SATURATED, F32)]))


def integer_deviations():
    far = np.asarray(FAR)
    return np.unique(np.concatenate([np.arange(-70.0, 71.0), far, -far])).astype(F32)


def real_deviations(seed=0):
    """+-0.5 exactly, 100 values in (-1.5, 1.5), 300 in (-70, 70), 100 in (-5000, 5000): stratified, so no stretch is empty."""
    rng = np.random.default_rng(seed)

    def strata(lo, hi, k):
        edges = np.linspace(lo, hi, k + 1)
        return rng.uniform(edges[:-1], edges[1:])

    return np.unique(np.concatenate([[-0.5, 0.5], strata(-1.5, 1.5, 100), strata(-70.0, 70.0, 300),
                                     strata(-5000.0, 5000.0, 100)]).astype(F32))


def sigma_of(raw):
    return np.exp(C0 + C1 * np.clip(np.exp(np.asarray(raw, F64)), 0.0, 63.0))


def _steps(x, k):
    x = F32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F32(np.inf if k > 0 else -np.inf))
    return x


def switch_cells():
    """(v, raw) pairs with (v +- .5)/s a few float32 steps on either side of -10 and of 0 -- and, mirrored, of +10, where the
    survival pair meets the same switch -- for five scales."""
    v, r = [], []
    for idx in SWITCH_INDEXES:
        raw = F32(-50.0) if idx == 0 else F32(math.log(idx))
        s = float(sigma_of(raw))
        for centre in (-10 * s - 0.5, -10 * s + 0.5, 10 * s - 0.5, 10 * s + 0.5, -0.5, 0.5):
            for k in SWITCH_ULPS:
                for sign in (-1, 1):
                    v.append(_steps(centre, sign * k))
                    r.append(raw)
    return np.asarray(v, F32), np.asarray(r, F32)


def _grid(dev, raw):
    return np.repeat(dev, raw.size), np.tile(raw, dev.size)


def cells(kind):
    """-> (v, raw), float32 [cells].  "integer": the integer deviations x raws (what the rounding scan and a pinned SGA sample
    can reach); "real": the non-integer deviations x raws plus the switch cells; "all": both."""
    if kind == "integer":
        return _grid(integer_deviations(), raws())
    if kind == "real":
        v, r = _grid(real_deviations(), raws())
        sv, sr = switch_cells()
        return np.concatenate([v, sv]), np.concatenate([r, sr])
    if kind == "all":
        a, b = cells("integer"), cells("real")
        return np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])
    raise ValueError(kind)


def factorized_deviations(kind, seed=1):
    """Deep-factorized prior: the integers -60 .. 60 / 200 stratified non-integers in (-60, 60) and +-0.5."""
    if kind == "integer":
        return np.arange(-60.0, 61.0).astype(F32)
    rng = np.random.default_rng(seed)
    edges = np.linspace(-60.0, 60.0, 201)
    return np.unique(np.concatenate([[-0.5, 0.5], rng.uniform(edges[:-1], edges[1:])]).astype(F32))


# ---- float64 references ---------------------------------------------------------------------------
def ref_bits(v, raw):
    """Per-symbol bits: oracle.ops_np.noisy_normal_logprob (SciPy log_ndtr pair, survival pair right of the median)."""
    return -O.noisy_normal_logprob(np.asarray(v, F64), sigma_of(raw)) / LN2


def ref_autograd(v, raw):
    """-> (bits, d bits/d v, d bits/d raw) of train_ref.noisy_normal_bits by float64 autograd (identity_if_towards at the bound)."""
    vt = torch.from_numpy(np.asarray(v, F64)).requires_grad_(True)
    rt = torch.from_numpy(np.asarray(raw, F64)).requires_grad_(True)
    bits = train_ref.noisy_normal_bits(vt, rt)
    bits.sum().backward()
    return bits.detach().numpy(), vt.grad.numpy(), rt.grad.numpy()


def ref_analytic(v, raw):
    """The same derivatives written out, phi/P in the log domain:
        d bits/d v = -(r_hi - r_lo) / (s ln 2),  d bits/d s = (r_hi hi - r_lo lo) / (s ln 2),  r_x = phi(x) / P,
        d s/d raw = s c1 e^raw where the index is inside the bound or descent would move it back (d bits/d s > 0).
    -> dict(bits, dv, dr, S_v, S): S_v and S are the sizes of the two terms whose difference dv and dr are."""
    v, raw = np.asarray(v, F64), np.asarray(raw, F64)
    s = sigma_of(raw)
    e = np.exp(raw)
    hi, lo = (v + 0.5) / s, (v - 0.5) / s
    logp = O.noisy_normal_logprob(v, s)
    half_ln_2pi = 0.5 * math.log(2.0 * math.pi)
    r_hi = np.exp(-0.5 * hi * hi - half_ln_2pi - logp)
    r_lo = np.exp(-0.5 * lo * lo - half_ln_2pi - logp)
    dbits_ds = (r_hi * hi - r_lo * lo) / (s * LN2)
    gate = (e <= 63.0) | (dbits_ds > 0.0)
    return dict(bits=-logp / LN2, dv=-(r_hi - r_lo) / (s * LN2), dr=np.where(gate, dbits_ds * s * C1 * e, 0.0),
                S_v=(r_hi + r_lo) / (s * LN2), S=(np.abs(r_hi * hi) + np.abs(r_lo * lo)) * C1 * e / LN2)


# ---- the reference formulation at float32 -----------------------------------------------------------
def float32_restatement_bits(v, raw):
    """What oracle.ops_np.noisy_normal_logprob does, with every intermediate rounded to float32 and every elementary
    function correctly rounded (evaluated in float64, then rounded): the least error a float32 evaluation of that
    formulation can have, whatever its exp / log / erfc implementations."""
    def f(x):
        return np.asarray(x, F64).astype(F32)

    v, raw = f(v), f(raw)
    idx = np.minimum(f(np.exp(raw.astype(F64))), F32(63.0))
    s = f(np.exp((F32(C0) + f(F32(C1) * idx)).astype(F64)))
    hi, lo = f((v + F32(0.5)) / s), f((v - F32(0.5)) / s)
    right = hi > 0
    big = f(sp.log_ndtr(np.where(right, -lo, hi).astype(F64)))
    small = f(sp.log_ndtr(np.where(right, -hi, lo).astype(F64)))
    ratio = f(np.exp((small - big).astype(F64)))
    logp = big + f(np.log1p(-ratio.astype(F64)))
    return -f(logp.astype(F64) / LN2)


def min_abs_rel(got, ref):
    err = np.abs(np.asarray(got, F64) - ref)
    return np.minimum(err, err / np.maximum(np.abs(ref), 1e-300))


def float32_floor():
    v, raw = cells("all")
    return float(min_abs_rel(float32_restatement_bits(v, raw), ref_bits(v, raw)).max())


if __name__ == "__main__":
    for kind in ("integer", "real", "all"):
        print(f"{kind}: {cells(kind)[0].size} cells ({raws().size} raws)")
    print(f"float32 floor of the reference formulation, max of min(abs, rel) error in bits: {float32_floor():.3e}")
