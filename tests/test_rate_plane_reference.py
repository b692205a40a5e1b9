"""The float64 references behind tests/test_hip_rate_plane.py, checked on the same plane (CPU, no GPU needed): the GPU tests
judge the kernels out to |v|/sigma = 45 000, so the references have to be right there too."""
import numpy as np

from oracle import rate_plane as P

EPS = np.finfo(np.float64).eps


def test_plane_covers_what_it_claims():
    raw, ints, reals = P.raws(), P.integer_deviations(), P.real_deviations()
    e = np.exp(raw.astype(np.float64))
    assert ((e > 0) & (e <= 63)).sum() >= 64 + 2 and (raw == np.float32(-50)).any() and (raw == P.LN63).any()
    assert (e > 63).sum() >= 4 and e[e <= 63].max() > 62.9999                     # both sides of the bound, next to it
    assert set(np.arange(-70, 71)) | {s * f for s in (-1, 1) for f in P.FAR} == set(ints.tolist())
    assert {-0.5, 0.5} <= set(reals.tolist()) and np.abs(reals).max() <= 5000
    assert (np.abs(reals) < 1.5).sum() >= 100 and (np.abs(reals) < 70).sum() >= 400 and (np.abs(reals) > 70).sum() >= 90
    v, r = P.switch_cells()
    s = P.sigma_of(r)
    for x in ((v + 0.5) / s, (v - 0.5) / s):                                     # float32 neighbours on both sides of each switch
        for at in (-10.0, 0.0, 10.0):
            near = np.abs(x - at) < 1e-4
            assert (x[near] > at).sum() >= 5 and (x[near] < at).sum() >= 5
    assert P.cells("all")[0].size == P.cells("integer")[0].size + P.cells("real")[0].size


def test_references_are_finite_and_agree_on_the_plane():
    """SciPy's log_ndtr pair (ops_np) and torch's under autograd (train_ref) give the same bits; autograd's derivatives equal
    the analytic ones (phi / P in the log domain) to 1e-6 relative.  Each derivative is a difference of two terms of sizes
    S_v / S, and float64 resolves it to ~1e-16 of those: 1e-12 of them is allowed next to the relative bar."""
    v, raw = P.cells("all")
    bits, dv, dr = P.ref_autograd(v, raw)
    a = P.ref_analytic(v, raw)
    for x in (bits, dv, dr, P.ref_bits(v, raw), a["dv"], a["dr"], a["S"], a["S_v"]):
        assert np.isfinite(x).all()
    assert (bits > 0).all() and bits.max() > 1e9                                   # the far tail really is in the plane
    np.testing.assert_allclose(bits, P.ref_bits(v, raw), rtol=1e-12, atol=1e-15)
    assert (np.abs(dv - a["dv"]) <= 1e-6 * np.abs(a["dv"]) + 1e-12 * a["S_v"]).all()
    assert (np.abs(dr - a["dr"]) <= 1e-6 * np.abs(a["dr"]) + 1e-12 * a["S"]).all()
    sat = np.exp(raw.astype(np.float64)) > 63                                      # identity_if_towards at the bound
    assert (dr[sat] >= 0).all() and (dr[sat] > 0).any() and (dr[sat] == 0).any()


def test_central_differences_at_moderate_cells():
    """Where float64 differences can resolve them (both bin edges within 4 sigma, index inside the bound) central differences
    of ref_bits reproduce the derivatives.  Steps h = 1e-4 sigma in v and 1e-6 in raw; the truncation h^2 f''' / 6 is below
    1e-7 S_v (f''' <~ 65 S_v / sigma^2 at |x| <= 4) and (c1 e^raw)^3 x^6 h^2 / 6 <= 3e-7 of S; the roundoff is eps bits / h."""
    v, raw = (a.astype(np.float64) for a in P.cells("all"))
    s = P.sigma_of(raw)
    ok = (np.abs(v) + 0.5 <= 4 * s) & (np.exp(raw) < 62.9)
    assert ok.sum() > 10000
    v, raw, s = v[ok], raw[ok], s[ok]
    a = P.ref_analytic(v, raw)
    round_off = 4 * EPS * np.maximum(a["bits"], 1.0)
    h = 1e-4 * s
    fd = (P.ref_bits(v + h, raw) - P.ref_bits(v - h, raw)) / (2 * h)
    assert (np.abs(fd - a["dv"]) <= 1e-5 * np.abs(a["dv"]) + 1e-6 * a["S_v"] + round_off / h).all()
    h = 1e-6
    fd = (P.ref_bits(v, raw + h) - P.ref_bits(v, raw - h)) / (2 * h)
    assert (np.abs(fd - a["dr"]) <= 1e-5 * np.abs(a["dr"]) + 1e-6 * a["S"] + round_off / h).all()


def test_float32_floor_constant_is_the_one_the_reference_gives():
    """FLOAT32_FLOOR of the GPU test is derived from the reference formulation alone; recompute it."""
    import test_hip_rate_plane as G
    floor = P.float32_floor()
    assert abs(G.FLOAT32_FLOOR - floor) <= 1e-3 * floor, (G.FLOAT32_FLOOR, floor)
    assert G.KERNEL_FACTOR == 4.0
