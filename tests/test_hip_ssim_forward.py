"""The SSIM / MS-SSIM forward on the GPU (-m gpu; csrc/msssim.hip and the input / finish kernels of csrc/msssim_grad.hip), one
entry point at a time against the float64 references and bars of tests/ssim_cases.py: single map elements, tile edges and
masks, exact invariants, the pool, the two pixel-value kernels, the finish, and -- as 1 - q, the form in which msssim_db, the
R-D ladder and the SGA loss read it -- what ``ops.image_quality`` and ``ops.msssim_distortion_grad`` return.

Figures of an MI355X are in DESIGN.md 4.6."""
import numpy as np
import pytest
import torch

import ssim_cases as S
from oracle import ops_np as O

pytestmark = pytest.mark.gpu


def t(x, dev):
    return torch.from_numpy(np.array(x)).to(dev)


def scale_sums(a, b, dev):
    """sntc_ssim_scale -> (ssim_sum[n, c], cs_sum[n, c]) float64."""
    from shallow_ntc_amd import ops
    n, c = a.shape[0], a.shape[3]
    out = torch.full((2, n, c), 7.0, dtype=torch.float64, device=dev)         # the launch zeroes its sums
    count = ops._ssim_scale(t(a, dev), t(b, dev), 255.0, out)
    assert count == (a.shape[1] - 10) * (a.shape[2] - 10)
    out = out.cpu().numpy()
    return out[0], out[1]


def model_range(a):
    """0-255 floats -> the model's [-0.5, 0.5] floats and the float32 pixel values msssim_inputs rebuilds from them."""
    x = (a / np.float32(255) - np.float32(0.5)).astype(np.float32)
    return x, S.pixel_values_f32(x)


# ---- B1: sntc_ssim_scale, one map element per sum ----------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("family", S.FAMILIES)
def test_every_map_element(family, c, dev):
    a, b = S.pair(family, 64, 11, 11, c)
    st = S.family_stats(family, 64, 11, 11, c)
    ssim, cs = scale_sums(a, b, dev)
    worst_cs = S.worst_ratio(cs, st["cs"][:, 0, 0], st["bar_cs"][:, 0, 0])
    worst_ssim = S.worst_ratio(ssim, st["ssim"][:, 0, 0], st["bar_ssim"][:, 0, 0])
    print(f"{family} c={c}: worst error / bar = {worst_cs:.3f} (cs) {worst_ssim:.3f} (ssim)")
    assert worst_cs <= 1 and worst_ssim <= 1, (worst_cs, worst_ssim)


# ---- B2: tiles, masks, batch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("h,w", S.TILE_SHAPES)
@pytest.mark.parametrize("family", ["smooth", "bright"])
def test_tiles_masks_and_batch(family, h, w, c, dev):
    """The mean of the per-element bars is loose for precision and tight for structure: one unmasked or dropped element moves
    a mean by about 1 / count."""
    a, b = S.pair(family, 3, h, w, c)
    ref_ssim, ref_cs, bar_ssim, bar_cs = S.mean_stats(S.family_stats(family, 3, h, w, c))
    count = (h - 10) * (w - 10)
    ssim, cs = scale_sums(a, b, dev)
    worst = max(S.worst_ratio(cs / count, ref_cs, bar_cs), S.worst_ratio(ssim / count, ref_ssim, bar_ssim))
    print(f"{family} 3x{h}x{w}x{c}: worst error of a mean / bar = {worst:.3f}; 1 / count = {1 / count:.1e}, widest bar = "
          f"{max(bar_cs.max(), bar_ssim.max()):.1e}")
    assert worst <= 1, worst
    for i in (0, 2):                                        # the same image launched alone: double atomics, only the order differs
        ssim1, cs1 = scale_sums(a[i:i + 1], b[i:i + 1], dev)
        np.testing.assert_allclose(ssim1[0], ssim[i], rtol=1e-12)
        np.testing.assert_allclose(cs1[0], cs[i], rtol=1e-12)


# ---- B3: exact invariants ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["smooth", "bright", "sga_range"])
def test_identical_images_are_exactly_one(family, dev):
    """2 exy == esq and 2 m0 m1 == m0^2 + m1^2 bit for bit, centred or not: every element is exactly 1.0f."""
    from shallow_ntc_amd import ops
    for h, w in S.TILE_SHAPES + ((161, 161),):
        for c in (1, 3):
            a, _ = S.pair(family, 2, h, w, c)
            ssim, cs = scale_sums(a, a, dev)
            assert (ssim == (h - 10) * (w - 10)).all() and (cs == (h - 10) * (w - 10)).all(), (h, w, c)
            assert (ops.image_quality(t(a, dev), t(a, dev)) == 1.0).all(), (h, w, c)
    a, _ = S.pair(family, 2, 161, 161, 3)
    sums, counts, single = ops.image_quality_launch(t(a, dev), t(a, dev))
    assert not single and (sums.cpu().numpy() == np.asarray(counts).reshape(5, 1, 1, 1)).all()


@pytest.mark.parametrize("p,r", S.CONSTANT_PAIRS)
def test_constant_images(p, r, dev):
    from shallow_ntc_amd import ops
    for c in (1, 3):
        a, b = S.constant_pair(p, r, 2, 26, 26, c)
        ref_ssim, ref_cs, bar_ssim, bar_cs = S.mean_stats(S.element_stats(a, b))
        ssim, cs = scale_sums(a, b, dev)
        assert (np.abs(cs / 256 - 1.0) <= bar_cs).all(), (cs / 256 - 1.0, bar_cs)
        assert (np.abs(ssim / 256 - S.lum_closed_form(p, r)) <= bar_ssim).all()
        q = ops.image_quality(t(a, dev), t(b, dev))
        assert (np.abs(q - S.lum_closed_form(p, r)) <= bar_ssim.mean(axis=-1)).all()
    a, b = S.constant_pair(p, r, 1, 161, 161, 3)
    q_ref, bar = S.quality_with_bar(a, b)
    np.testing.assert_allclose(q_ref, S.lum_closed_form(p, r) ** S.WEIGHTS[-1], rtol=1e-13)
    q = ops.image_quality(t(a, dev), t(b, dev))
    assert (np.abs(q - S.lum_closed_form(p, r) ** S.WEIGHTS[-1]) <= bar).all(), (q, q_ref, bar)


# ---- B4: sntc_avgpool2_symmetric ----------------------------------------------------------------------------------------------
POOL_LONG = (1, 1451, 1451, 1)     # 726 x 726 outputs: past one trip of the grid-stride loop, and an odd size
assert 726 * 726 > S.GRID_CAP


@pytest.mark.parametrize("shape", [(2, 1, 1, 3), (2, 1, 2, 1), (2, 2, 1, 3), (2, 9, 13, 3), (2, 8, 12, 1), (2, 33, 2, 3), POOL_LONG])
def test_pool(shape, dev):
    """4 float32 roundings (three additions, the product) against sum |terms| / 4; integer-valued inputs are exact."""
    from shallow_ntc_amd import ops
    rng = np.random.default_rng(shape[1] * 1000 + shape[2])
    x = (100.0 * rng.standard_normal(shape)).astype(np.float32)
    got = ops._avgpool2(t(x, dev)).cpu().numpy()
    ref, mag = O._avg_pool2_symmetric(x.astype(np.float64)), O._avg_pool2_symmetric(np.abs(x.astype(np.float64)))
    assert got.shape == ref.shape
    assert (np.abs(got - ref) <= 4 * S.U * mag).all(), float((np.abs(got - ref) / (4 * S.U * mag)).max())
    np.testing.assert_array_equal(got, S.emulate_pool(x))
    xi = rng.integers(0, 256, shape).astype(np.float32)
    np.testing.assert_array_equal(ops._avgpool2(t(xi, dev)).cpu().numpy().astype(np.float64), O._avg_pool2_symmetric(xi.astype(np.float64)))


# ---- B5: sntc_pixels_float -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 3])
def test_pixels_float_bits(c, dev):
    from shallow_ntc_amd import ops
    rng = np.random.default_rng(c)
    half = np.float32(0.5)
    ends = np.float32([-0.5, 0.5, np.nextafter(-half, np.float32(-1)), np.nextafter(-half, np.float32(1)), np.nextafter(half, np.float32(1)),
                       np.nextafter(half, np.float32(-1)), -0.502, 0.502, -3.0, 3.0, 0.0, -0.0, 1e30, -1e30])
    vals = np.concatenate([S.pixel_ties(), ends, rng.uniform(-0.6, 0.6, 200).astype(np.float32)])
    n, h, w, hs, ws = 2, 19, 27, 23, 30
    assert n * h * w * c >= vals.size
    xh = np.full((n, hs, ws, c), 1e30, np.float32)
    inner = np.resize(vals, (n, h, w, c))
    xh[:, :h, :w] = inner
    got = ops.pixels_float(t(xh, dev), h, w).cpu().numpy()
    np.testing.assert_array_equal(got, S.pixels_float_f32(inner))
    np.testing.assert_array_equal(got, O.floats_to_pixels(np.clip(inner, -1, 1), False).astype(np.float32))


def test_pixels_float_past_one_grid_trip(dev):
    from shallow_ntc_amd import ops
    shape = (1, 419, 419, 3)
    assert np.prod(shape) > S.GRID_CAP
    x = np.random.default_rng(0).uniform(-0.6, 0.6, shape).astype(np.float32)
    np.testing.assert_array_equal(ops.pixels_float(t(x, dev), 419, 419).cpu().numpy(), S.pixels_float_f32(x))


# ---- B6: sntc_msssim_inputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w,c,pad", [(3, 5, 7, 3, (2, 3)), (1, 11, 40, 1, (0, 0)), (2, 37, 52, 3, (0, 0)), (2, 37, 52, 3, (3, 4))])
def test_msssim_inputs(n, h, w, c, pad, dev):
    """a and b bit for bit; the margin (1e30) reaches nothing; sse at 5 u of its sum of squares (d = x_hat - x, 255 d and the
    square round once each, and the square doubles what came before it: 2 (u + u) + u) and equal to sntc_distortion_grad's."""
    from shallow_ntc_amd import ops
    rng = np.random.default_rng(n * h * w)
    x = rng.uniform(-0.5, 0.5, (n, h, w, c)).astype(np.float32)
    xh = (x + 0.05 * rng.standard_normal(x.shape)).astype(np.float32)
    xh_pad = np.pad(xh, ((0, 0), (0, pad[0]), (0, pad[1]), (0, 0)), constant_values=1e30)
    a, b, sse = ops.msssim_inputs(t(x, dev), t(xh_pad, dev))
    np.testing.assert_array_equal(a.cpu().numpy(), S.pixel_values_f32(x))
    np.testing.assert_array_equal(b.cpu().numpy(), S.pixel_values_f32(xh))
    ref = ((255.0 * (xh.astype(np.float64) - x.astype(np.float64))) ** 2).sum(axis=(1, 2, 3))
    sse = sse.cpu().numpy()
    assert (np.abs(sse - ref) <= 5 * S.U * ref).all(), np.abs(sse - ref) / (5 * S.U * ref)
    _, sse_mse = ops.distortion_grad(t(x, dev), t(xh_pad, dev), 1.0)
    np.testing.assert_allclose(sse, sse_mse.cpu().numpy(), rtol=1e-13)


# ---- B7: sntc_msssim_finish ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("n", [1, 64, 65])
@pytest.mark.parametrize("scales", [1, 5])
def test_finish(scales, n, c, dev):
    """Synthetic sums, no SSIM kernel.  Of every 13 (image, channel) products: five with a negative factor at positions 0 .. 4,
    five with a factor of exactly 0 there, three untouched.  Single-scale takes no clamp: the negative sums go straight in."""
    from shallow_ntc_amd import ops
    rng = np.random.default_rng(scales * 100 + n * 3 + c)
    single, weight = scales == 1, -37.5 / n
    counts = [float(v) for v in rng.integers(1, 40000, scales)]
    sums = rng.uniform(0.05, 1.0, (scales, 2, n, c)) * np.asarray(counts).reshape(-1, 1, 1, 1)
    clamped = np.zeros((n, c), bool)
    if n > 1:
        for j in range(n * c):
            i, ch, kind = j // c, j % c, j % 13
            if kind < 10:
                k = kind % 5 if not single else 0
                sums[k, 0 if (single or k == scales - 1) else 1, i, ch] = -0.3 * counts[k] if kind < 5 else 0.0
                clamped[i, ch] = not single
    q, coef = ops.msssim_finish(t(sums, dev), counts, single, weight)
    assert q.dtype == torch.float64 and coef.dtype == torch.float32 and coef.shape == (scales, n, c)
    q, coef = q.cpu().numpy(), coef.cpu().numpy()
    q_ref, coef_ref = S.finish_reference(sums, counts, single, weight)
    np.testing.assert_allclose(q_ref, ops.image_quality_finish(sums, counts, single), rtol=1e-13)
    bar = S.finish_q_bar(np.abs(sums[0, 0] / counts[0]).mean(axis=-1) if single else q_ref, scales, c)
    assert (np.abs(q - q_ref) <= bar).all(), float((np.abs(q - q_ref) / np.maximum(bar, 1e-300)).max())
    assert (np.abs(coef - coef_ref) <= S.finish_coef_bar(coef_ref, scales)).all()
    assert (coef[:, clamped] == 0).all() and (coef[:, ~clamped] != 0).all()           # a clamped product: exactly 0
    if clamped.any():
        assert clamped.all(axis=-1).any() and (q[clamped.all(axis=-1)] == 0).all()


# ---- B8: what the consumers read --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", S.CONSUMER_SHAPES)
@pytest.mark.parametrize("family", ["smooth", "bright", "bright_rounded", "flat_bright"])
def test_quality_as_the_consumers_read_it(family, h, w, dev):
    """ops.image_quality and the q of ops.msssim_distortion_grad within the first-order propagation of the element bars (and of
    the pool's) through prod f_k^{w_k}; 1 - q and dB are printed, no tolerance is set on them."""
    from shallow_ntc_amd import ops
    a0, b0 = S.pair(family, 1, h, w, 3)
    x, a = model_range(a0)
    xh, b = model_range(b0)
    q_ref, bar = S.quality_with_bar(a, b)
    np.testing.assert_allclose(q_ref, O.image_quality(a, b)[0], rtol=1e-12)
    q_eval = ops.image_quality(t(a, dev), t(b, dev))
    _, _, q_sga = ops.msssim_distortion_grad(t(x, dev), t(xh, dev), 10.0)
    q_sga = q_sga.cpu().numpy()
    for name, q in (("image_quality", q_eval), ("msssim_distortion_grad", q_sga)):
        print(f"{family} {h}x{w} {name}: 1 - q = {float(1 - q_ref[0]):.3e}, rel. err. of 1 - q = "
              f"{float(abs(q - q_ref)[0] / (1 - q_ref[0])):.2e}, dB err. = {float(abs(S.db(q) - S.db(q_ref))[0]):.2e}, err / bar = "
              f"{float((abs(q - q_ref) / bar)[0]):.3f}")
    np.testing.assert_allclose(q_sga, q_eval, rtol=1e-12)
    assert (np.abs(q_eval - q_ref) <= bar).all() and (np.abs(q_sga - q_ref) <= bar).all()
