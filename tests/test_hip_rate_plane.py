"""The rate kernels and their gradients SYMBOL BY SYMBOL on the plane of scale index x deviation (oracle/rate_plane.py), out to
|v| = 5000, against float64: csrc/entropy.hip (both scans, both deep-factorized kernels) and the rate / rate-gradient kernels
of csrc/sga.hip.  The other tests compare per-image sums of bits, and per-element gradients at a few hundred random points
with |v|/sigma below ~60; this file walks the regimes of the formulas: the a == 0 / a >= 1 forms and the ln(1 - e) series of
normal_bits_fast, its two erfcx values at large sigma, the x > 0 / x > -10 / asymptotic switch of log_ndtr_f, the median
switch and the saturated scale index.

The kernels return per-image sums; a symbol is read alone by giving every cell its own image (n = cells, h = w = 1, c = 4, the
same (v, raw) in the four channels; the sum over 4) -- the trick of test_hip_ops.py::test_entropy_known_answers.

Bars
  bits        |got - ref| <= 2e-4 max(ref, 1e-3) (test_entropy_known_answers') AND min(abs, rel) error <= KERNEL_FACTOR x
              FLOAT32_FLOOR, the error of the reference's own formulation evaluated at float32 (derived on the CPU from the
              reference, not from a kernel: tests/test_rate_plane_reference.py recomputes it)
  gradients   |got - ref| <= 2e-6 + 1e-3 |ref| (test_hip_train.py's per-element bar); for d bits / d raw |ref| is replaced by
              max(|ref|, 1e-3 S), S = (|r_hi hi| + |r_lo lo|) c1 e^raw / ln 2 the size of the two terms whose difference the
              derivative is: near |v| ~ sigma it crosses zero and no float32 evaluation resolves it below a few roundings of
              S (1e-6 S is ~17 ulp).  A conditioning floor, not a skip: every cell is judged.
  everything  finite.

The derivatives written as exp(-x^2/2 - c - log P), as they were before this file existed, leave the gradient bar from
|v|/sigma ~ 180 on in a float32 emulation (DESIGN.md 4.5 has the table); every check prints its measured figure as a
"PLANE ..." line (pytest -s).
"""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import model_np
from oracle import ops_np as O
from oracle import rate_plane as P
from oracle import train_ref

pytestmark = pytest.mark.gpu

# python -m oracle.rate_plane
#   "float32 floor of the reference formulation, max of min(abs, rel) error in bits: 5.962e-06"
FLOAT32_FLOOR = 5.962e-6
# x2: the scan's fast path subtracts two erfcx values that agree to three digits at large sigma; x2: exp / log implementations
KERNEL_FACTOR = 4.0
IMAGES_PER_LAUNCH = 8192
LN2 = math.log(2.0)


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


@functools.lru_cache(maxsize=None)
def reference(kind):
    """Computed once per kind of cell and shared (read-only) by the tests."""
    v, raw = P.cells(kind)
    bits, dv, dr = P.ref_autograd(v, raw)
    ref = dict(v=v, raw=raw, bits=P.ref_bits(v, raw), bits_train=bits, dv=dv, dr=dr, S=P.ref_analytic(v, raw)["S"])
    for a in ref.values():
        assert np.isfinite(a).all()
        a.setflags(write=False)
    return ref


def per_image(fn, v, raw, dev):
    """fn(y [n,1,1,4], hyper [n,1,1,8]) -> (bits[n], per-element tensors...) run over the cells, one cell per image.
    -> (per-symbol bits, channel 0 of every per-element output)."""
    outs = []
    for s in range(0, v.size, IMAGES_PER_LAUNCH):
        vv, rr = v[s:s + IMAGES_PER_LAUNCH], raw[s:s + IMAGES_PER_LAUNCH]
        y = np.repeat(vv, 4).reshape(-1, 1, 1, 4)
        hyper = np.concatenate([np.zeros_like(y), np.repeat(rr, 4).reshape(-1, 1, 1, 4)], -1)
        got = fn(t(y, dev), t(hyper, dev))
        outs.append([got[0].cpu().numpy() / 4] + [g.cpu().numpy()[:, 0, 0, 0].astype(np.float64) for g in got[1:]])
    return [np.concatenate(c) for c in zip(*outs)]


def worst(score, ref, got, **where):
    k = int(np.nanargmax(np.where(np.isfinite(score), score, np.inf)))
    at = ", ".join(f"{n} {a[k]:.9g}" for n, a in where.items())
    return f"worst {score[k]:.3g} of the bar at {at}: got {got[k]:.9g}, float64 {ref[k]:.9g}"


def check_bits(name, got, ref, **where):
    assert np.isfinite(got).all(), f"{name}: {np.count_nonzero(~np.isfinite(got))} non-finite bits"
    err = np.abs(got - ref)
    hard = err / (2e-4 * np.maximum(ref, 1e-3))
    tight = np.minimum(err, err / np.maximum(ref, 1e-300)) / (KERNEL_FACTOR * FLOAT32_FLOOR)
    print(f"PLANE {name} bits: {ref.size} symbols, max min(abs, rel) error {tight.max() * KERNEL_FACTOR * FLOAT32_FLOOR:.3e} "
          f"(float32 floor {FLOAT32_FLOOR:.3e}), {hard.max():.3g} of the 2e-4 bar")
    assert (hard <= 1).all(), f"{name} bits, 2e-4 max(ref, 1e-3): {worst(hard, ref, got, **where)}"
    assert (tight <= 1).all(), f"{name} bits, {KERNEL_FACTOR:g} x float32 floor: {worst(tight, ref, got, **where)}"


def check_gradient(name, got, ref, size=None, **where):
    assert np.isfinite(got).all(), f"{name}: {np.count_nonzero(~np.isfinite(got))} non-finite gradients"
    scale = np.abs(ref) if size is None else np.maximum(np.abs(ref), 1e-3 * size)
    score = np.abs(got - ref) / (2e-6 + 1e-3 * scale)
    sig = P.sigma_of(where["raw"]) if "raw" in where else None
    far = "" if sig is None or (score <= 1).all() else \
        f"; {np.mean(score > 1):.2%} of the cells over the bar, from |v|/sigma = {(np.abs(where['v']) / sig)[score > 1].min():.4g}"
    print(f"PLANE {name}: {ref.size} elements, worst {score.max():.3g} of the bar{far}")
    assert (score <= 1).all(), f"{name}: {worst(score, ref, got, **where)}{far}"


# ---- scale-indexed normal -------------------------------------------------------------------------
def test_scan_bits_per_symbol_rounding_mode(dev):
    """ops.entropy_scale_normal on the integer deviations: normal_bits_fast."""
    from shallow_ntc_amd import ops
    ref = reference("integer")

    def run(y, hyper):
        y_hat, bits, _ = ops.entropy_scale_normal(y, hyper)
        assert torch.equal(y_hat, y)                                        # integers round to themselves
        return (bits,)

    (got,) = per_image(run, ref["v"], ref["raw"], dev)
    check_bits("entropy_scale_normal(round)", got, ref["bits"], v=ref["v"], raw=ref["raw"])


def test_scan_bits_per_symbol_explicit_samples(dev):
    """ops.entropy_scale_normal(values_only=True) on the non-integer deviations and the switch cells: normal_bits / log_ndtr_f."""
    from shallow_ntc_amd import ops
    ref = reference("real")
    (got,) = per_image(lambda y, hyper: (ops.entropy_scale_normal(y, hyper, values_only=True)[1],), ref["v"], ref["raw"], dev)
    check_bits("entropy_scale_normal(values)", got, ref["bits"], v=ref["v"], raw=ref["raw"])


@pytest.mark.parametrize("kind", ["integer", "real"])
def test_noisy_normal_per_symbol(kind, dev):
    """ops.noisy_normal, one cell per image: per-symbol bits, and both derivatives in this layout."""
    from shallow_ntc_amd import ops
    ref = reference(kind)
    bits, dv, dr = per_image(ops.noisy_normal, ref["v"], ref["raw"], dev)
    where = dict(v=ref["v"], raw=ref["raw"])
    check_bits(f"noisy_normal[{kind}]", bits, ref["bits"], **where)
    check_gradient(f"noisy_normal[{kind}] d bits/d v", dv, ref["dv"], **where)
    check_gradient(f"noisy_normal[{kind}] d bits/d raw", dr, ref["dr"], size=ref["S"], **where)


def test_noisy_normal_gradients_whole_plane_one_launch(dev):
    """dv, dr of ops.noisy_normal over every cell of the plane in ONE launch, the cells laid out along h w c of one image
    (several grid-stride steps per thread, channels next to each other holding different cells)."""
    from shallow_ntc_amd import ops
    ref = reference("all")
    c, w = 8, 33
    cells = ref["v"].size
    h = -(-cells // (c * w))
    v, raw = np.zeros(h * w * c, np.float32), np.zeros(h * w * c, np.float32)
    v[:cells], raw[:cells] = ref["v"], ref["raw"]
    v, raw = v.reshape(1, h, w, c), raw.reshape(1, h, w, c)
    bits, dv, dr = ops.noisy_normal(t(v, dev), t(np.concatenate([np.zeros_like(v), raw], -1), dev))
    assert np.isfinite(bits.cpu().numpy()).all()
    where = dict(v=ref["v"], raw=ref["raw"])
    check_gradient("noisy_normal[plane] d bits/d v", dv.cpu().numpy().ravel()[:cells].astype(np.float64), ref["dv"], **where)
    check_gradient("noisy_normal[plane] d bits/d raw", dr.cpu().numpy().ravel()[:cells].astype(np.float64), ref["dr"],
                   size=ref["S"], **where)


def test_sga_normal_fwd_per_symbol(dev):
    """ops.sga_normal_fwd on the integer deviations: y_loc - mu integer-valued makes floor == ceil, the sample is that
    integer whatever the noise; bits per symbol and both derivatives at it."""
    from shallow_ntc_amd import ops
    ref = reference("integer")

    def run(y, hyper):
        noise = torch.zeros(tuple(y.shape) + (2,), dtype=torch.float32, device=y.device)
        yt, sp, dv, dr, bits = ops.sga_normal_fwd(y, hyper, 0.5, noise=noise)
        assert torch.equal(yt, y)
        return bits, dv, dr

    bits, dv, dr = per_image(run, ref["v"], ref["raw"], dev)
    where = dict(v=ref["v"], raw=ref["raw"])
    check_bits("sga_normal_fwd", bits, ref["bits"], **where)
    check_gradient("sga_normal_fwd d bits/d v", dv, ref["dv"], **where)
    check_gradient("sga_normal_fwd d bits/d raw", dr, ref["dr"], size=ref["S"], **where)


# ---- deep-factorized prior --------------------------------------------------------------------------
PRIORS = [((3, 3), 260),          # factorized_fast_kernel, channels across a 256-thread block
          ((2,), 8), ((4, 4, 4, 4), 8)]   # factorized_kernel
BASE = 0.0                        # the deviation of every channel but the one under test


@functools.lru_cache(maxsize=None)
def prior_lists(num_filters, c):
    rng = np.random.default_rng(100 * len(num_filters) + c)
    p = model_np.init_deep_factorized(c, rng, num_filters)
    for k in p:                                   # off the initial values so the tanh factors matter (as test_entropy_factorized)
        p[k] = (p[k] + 0.3 * rng.standard_normal(p[k].shape)).astype(np.float32)
    return model_np._prior_lists(p)


def factorized_reference(lists, v):
    """v [D, c] float64 -> per-symbol bits (ops_np) and d bits/d v (train_ref under float64 autograd)."""
    ms, bs, fs = lists
    bits = -O.deep_factorized_logprob(v, ms, bs, fs) / LN2
    vt = torch.from_numpy(v).requires_grad_(True)
    bt = train_ref.noisy_deep_factorized_bits(vt, *[[torch.from_numpy(a.astype(np.float64)) for a in arrs] for arrs in lists])
    bt.sum().backward()
    assert np.isfinite(bits).all() and np.isfinite(vt.grad.numpy()).all()
    np.testing.assert_allclose(bt.detach().numpy(), bits, rtol=1e-9, atol=1e-12)
    return bits, vt.grad.numpy()


def isolated(fn, devs, c, dev):
    """One symbol per image: image d * c + ch holds devs[d] in channel ch and BASE in the others, the last image BASE
    everywhere; fn(z [n,1,1,c]) -> (bits[n], per-element tensors...).  The per-image sums are double sums of the same float32
    terms but one, so  bits[image] - bits[last]  is  bits_ch(devs[d]) - bits_ch(BASE)  of the kernel to 1e-13.
    -> (that difference [D, c], the per-element outputs at the symbol under test [D, c] ...)."""
    D = devs.size
    z = np.full((D * c + 1, c), BASE, np.float32)
    img = np.arange(D * c)
    z[img, img % c] = np.repeat(devs, c)
    cols = []
    for s in range(0, z.shape[0], IMAGES_PER_LAUNCH):
        zz = z[s:s + IMAGES_PER_LAUNCH]
        got = fn(t(zz.reshape(-1, 1, 1, c), dev))
        rows = np.arange(zz.shape[0])
        ch = (s + rows) % c                                             # (the last image: any channel, dropped below)
        cols.append([got[0].cpu().numpy()] + [g.cpu().numpy().reshape(-1, c)[rows, ch].astype(np.float64) for g in got[1:]])
    bits, *elems = [np.concatenate(col) for col in zip(*cols)]
    return [(bits[:-1] - bits[-1]).reshape(D, c)] + [e[:-1].reshape(D, c) for e in elems]


def check_factorized(name, lists, c, v, dbits, grad=None):
    """v [D, c]: the samples the kernel evaluated.  dbits: bits(v) - bits(BASE) per symbol."""
    ref, ref_dz = factorized_reference(lists, v.astype(np.float64))
    ref0, _ = factorized_reference(lists, np.full((1, c), BASE))
    assert np.isfinite(dbits).all()
    # two symbols' errors in the difference: each at the project's per-symbol bar
    bar = 2e-4 * (np.maximum(ref, 1e-3) + np.maximum(ref0, 1e-3))
    score = np.abs(dbits - (ref - ref0)) / bar
    ch = np.broadcast_to(np.arange(c, dtype=np.float64), v.shape)
    print(f"PLANE {name} bits: {ref.size} symbols of up to {ref.max():.4g} bits, worst {score.max():.3g} of the 2e-4 bar, "
          f"max min(abs, rel) error {P.min_abs_rel(dbits + ref0, ref).max():.3e}")
    assert (score <= 1).all(), f"{name} bits: {worst(score.ravel(), (ref - ref0).ravel(), dbits.ravel(), v=v.ravel(), channel=ch.ravel())}"
    if grad is not None:
        check_gradient(f"{name} d bits/d z", grad.ravel(), ref_dz.ravel(), v=v.ravel(), channel=ch.ravel())


@pytest.mark.parametrize("num_filters,c", PRIORS)
def test_factorized_scan_per_symbol(num_filters, c, dev):
    """DeepFactorizedPrior.__call__: the rounding mode on the integers, explicit samples on the non-integers."""
    from shallow_ntc_amd import ops
    lists = prior_lists(num_filters, c)
    prior = ops.DeepFactorizedPrior(*lists)
    ints, reals = P.factorized_deviations("integer"), P.factorized_deviations("real")

    def rounding(z):
        z_hat, bits = prior(z)
        assert torch.equal(z_hat, z)
        return (bits,)

    (d,) = isolated(rounding, ints, c, dev)
    check_factorized(f"DeepFactorizedPrior{num_filters}(round)", lists, c, np.repeat(ints[:, None], c, 1), d)
    (d,) = isolated(lambda z: (prior(z, values_only=True)[1],), reals, c, dev)
    check_factorized(f"DeepFactorizedPrior{num_filters}(values)", lists, c, np.repeat(reals[:, None], c, 1), d)


@pytest.mark.parametrize("num_filters,c", PRIORS)
def test_noisy_factorized_per_symbol(num_filters, c, dev):
    """ops.noisy_factorized: per-symbol bits and per-element d bits/d z on the integers and the non-integers."""
    from shallow_ntc_amd import ops
    lists = prior_lists(num_filters, c)
    prior = ops.DeepFactorizedPrior(*lists)
    devs = np.concatenate([P.factorized_deviations("integer"), P.factorized_deviations("real")])
    d, g = isolated(lambda z: ops.noisy_factorized(prior, z), devs, c, dev)
    check_factorized(f"noisy_factorized{num_filters}", lists, c, np.repeat(devs[:, None], c, 1), d, g)


@pytest.mark.parametrize("num_filters,c", PRIORS)
def test_sga_factorized_fwd_per_symbol(num_filters, c, dev):
    """ops.sga_factorized_fwd under zero Gumbel noise: integer locations are sampled as themselves, non-integer ones
    somewhere between floor and ceil; bits and d bits/d z at the sample the kernel returns."""
    from shallow_ntc_amd import ops
    lists = prior_lists(num_filters, c)
    prior = ops.DeepFactorizedPrior(*lists)
    devs = np.concatenate([P.factorized_deviations("integer"), P.factorized_deviations("real")])

    def run(z):
        noise = torch.zeros(tuple(z.shape) + (2,), dtype=torch.float32, device=z.device)
        zt, sp, db, bits = ops.sga_factorized_fwd(prior, z, 0.5, noise=noise)
        whole = z == torch.round(z)
        assert torch.equal(zt[whole], z[whole])
        return bits, db, zt

    d, g, v = isolated(run, devs, c, dev)
    assert (v >= np.floor(devs)[:, None]).all() and (v <= np.ceil(devs)[:, None]).all()
    check_factorized(f"sga_factorized_fwd{num_filters}", lists, c, v, d, g)
