"""The SSIM / MS-SSIM forward, the parts that need no GPU: the cases, references and bars of tests/ssim_cases.py are what
tests/test_hip_ssim_forward.py holds the kernels to, so this file checks them -- the references against the oracle, that the
hard cases are hard, that the bars are attainable by float32 (the emulation of the tile-centred kernel is within all of them)
and that they notice the defect they were written for (the emulation of the plain form E[x^2] - mu^2 on raw values is not)."""
import re
from pathlib import Path

import numpy as np
import pytest

import ssim_cases as S
from oracle import ops_np as O

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ("sntc_ssim_scale", "sntc_avgpool2_symmetric", "sntc_pixels_float", "sntc_msssim_inputs", "sntc_msssim_finish")
PATCH = (64, 11, 11)               # 64 images of one filter output each


def test_entry_points_declared_bound_and_exported():
    from shallow_ntc_amd import _capi
    header = (ROOT / "include" / "sntc.h").read_text()
    lib = _capi.load()
    for name in ENTRY_POINTS:
        assert re.search(rf"\bint {name}\(", header), f"{name} is not declared in include/sntc.h"
        assert name in _capi.SIGNATURES, f"{name} is missing from the _capi signature table"
        assert hasattr(lib, name), f"libsntc_hip.so does not export {name}"
        assert _capi.SIGNATURES[name][1][-1] is _capi.C.c_void_p                      # every entry point takes a stream
    assert "msssim.hip" in (ROOT / "shallow-ntc_amd" / "csrc" / "Makefile").read_text()


def test_case_module_restates_the_kernel():
    src = (ROOT / "shallow-ntc_amd" / "csrc" / "msssim.hip").read_text()
    assert re.search(r"kWin = 11;", src) and re.search(r"kTile = 16;", src)
    assert "cy = min(oy0 + kIn / 2, h - 1), cx = min(ox0 + kIn / 2, w - 1)" in src           # S.TILE_CENTRE
    assert "b > 2048 ? 2048 : b" in src                                                       # S.GRID_CAP
    assert (S.WIN, S.TILE, S.TILE_IN, S.TILE_CENTRE, S.GRID_CAP) == (11, 16, 26, 13, 2048 * 256)
    outputs = sorted({s - 10 for hw in S.TILE_SHAPES for s in hw})
    assert outputs == [1, 16, 17, 33, 49]                   # one, an exact tile, one past it, two tiles and one, three and one
    assert S.tiles(27, 43) == [(0, 0, 16, 16, 13, 13), (0, 16, 16, 16, 13, 29), (0, 32, 16, 1, 13, 42),
                               (16, 0, 1, 16, 26, 13), (16, 16, 1, 16, 26, 29), (16, 32, 1, 1, 26, 42)]


@pytest.mark.parametrize("family", S.FAMILIES)
@pytest.mark.parametrize("c", [1, 3])
def test_references_equal_the_oracle_and_are_not_degenerate(family, c):
    for n, h, w in (PATCH, (2, 27, 43)):
        a, b = S.pair(family, n, h, w, c)
        assert a.dtype == np.float32 and a.shape == (n, h, w, c) and not np.array_equal(a, b)
        st = S.family_stats(family, n, h, w, c)
        ssim, cs, bar_ssim, bar_cs = S.mean_stats(st)
        ref_ssim, ref_cs = O.ssim_per_channel(a, b)
        np.testing.assert_allclose(ssim, ref_ssim, rtol=1e-11, atol=1e-13)       # the shift leaves cs alone; lum takes it back
        np.testing.assert_allclose(cs, ref_cs, rtol=1e-11, atol=1e-13)
        # positive and not vacuous: the widest is a flat 0 patch of "blocks" whose tile constant is 255 (S ~ 255^2 over D = c2)
        assert (bar_cs > 0).all() and (bar_ssim > 0).all() and max(bar_cs.max(), bar_ssim.max()) < (0.05 if family == "blocks" else 1e-3)
        q = O.image_quality(a, b)[0]
        assert (1.0 - q > 0).all()
        if family == "checker":
            assert (st["cs"] < 0).all()
        if family in ("bright", "flat_bright"):
            assert (1.0 - q).mean() < 5e-3, (1.0 - q).mean()           # over the batch: one 11 x 11 patch is a noisy sample
    if family == "sga_range":
        a, b = S.pair(family, 2, 27, 43, c)
        assert a.min() < -10 and a.max() > 265 and a.min() >= -20 and b.max() <= 280
    if family == "blocks":
        a, _ = S.pair(family, 2, 27, 43, c)
        assert set(np.unique(a)) == {0.0, 255.0}


@pytest.mark.parametrize("family", S.HIGH_QUALITY)
def test_high_quality_families_are_in_the_regime_where_the_plain_form_fails(family):
    """1 - q < 5e-3 on the five-scale shapes for all three; the rounded variant's single-scale SSIM (sigma 1 after rounding) is
    1.8e-2 and is not asked to be."""
    for h, w in S.CONSUMER_SHAPES:
        if family == "bright_rounded" and h < 160:
            continue
        q, bar = S.family_quality(family, 1, h, w, 3)
        np.testing.assert_allclose(q, O.image_quality(*S.pair(family, 1, h, w, 3))[0], rtol=1e-12)
        assert (0 < 1.0 - q).all() and (1.0 - q < 5e-3).all(), (family, h, w, 1.0 - q)
        assert (bar < 0.2 * (1.0 - q)).all(), (family, h, w, bar, 1.0 - q)        # the bar still resolves 1 - q


def test_identical_pair_is_exactly_one():
    for family in ("smooth", "bright", "sga_range"):
        a, _ = S.pair(family, 1, 43, 59, 3)
        assert (O.image_quality(a, a)[0] == 1.0).all()
        for centred in (False, True):                       # 2 exy == esq and 2 m0 m1 == m0^2 + m1^2 bit for bit in both forms
            ssim, cs = S.emulate(a, a, centred)
            assert (ssim == 1.0).all() and (cs == 1.0).all()
    a, _ = S.pair("bright", 1, 161, 161, 3)
    assert (O.image_quality(a, a)[0] == 1.0).all() and (S.emulate_quality(a, a, True) == 1.0).all()


@pytest.mark.parametrize("family", S.FAMILIES)
@pytest.mark.parametrize("c", [1, 3])
def test_centred_emulation_is_within_every_element_bar(family, c):
    for n, h, w in (PATCH, (2, 27, 43)):
        a, b = S.pair(family, n, h, w, c)
        st = S.family_stats(family, n, h, w, c)
        ssim, cs = S.emulate(a, b, centred=True)
        worst = max(S.worst_ratio(cs, st["cs"], st["bar_cs"]), S.worst_ratio(ssim, st["ssim"], st["bar_ssim"]))
        print(f"{family} c={c} {n}x{h}x{w}: centred float32 emulation, worst error / bar = {worst:.3f}")
        assert worst <= 0.25, worst                        # not merely inside: the bar is no knife edge for a correct kernel


@pytest.mark.parametrize("family", S.HIGH_QUALITY)
@pytest.mark.parametrize("c", [1, 3])
def test_plain_emulation_exceeds_the_element_bar(family, c):
    a, b = S.pair(family, *PATCH, c)
    st = S.family_stats(family, *PATCH, c)
    ssim, cs = S.emulate(a, b, centred=False)
    worst_cs, worst_ssim = S.worst_ratio(cs, st["cs"], st["bar_cs"]), S.worst_ratio(ssim, st["ssim"], st["bar_ssim"])
    print(f"{family} c={c}: plain float32 emulation, worst error / bar = {worst_cs:.1f} (cs) {worst_ssim:.1f} (ssim)")
    assert worst_cs > 10 and worst_ssim > 10


def test_emulated_quality_against_the_consumer_bar():
    """What the consumers read: the centred emulation is within the propagated bar at every shape; the figures of 1 - q."""
    for family, (h, w) in (("smooth", (176, 200)), ("bright_rounded", (176, 200)), ("bright", (161, 187)), ("flat_bright", (161, 161)),
                           ("bright", (43, 59))):
        a, b = S.pair(family, 1, h, w, 3)
        q, bar = S.family_quality(family, 1, h, w, 3)
        for centred in (False, True):
            got = S.emulate_quality(a, b, centred)
            print(f"{family} {h}x{w} {'centred' if centred else 'plain'}: 1 - q = {float(1 - q[0]):.3e}, rel. err. of 1 - q = "
                  f"{float(abs(got - q)[0] / (1 - q[0])):.2e}, dB err. = {float(abs(S.db(got) - S.db(q))[0]):.2e}, err / bar = "
                  f"{float((abs(got - q) / bar)[0]):.3f}")
            if centred:
                assert (np.abs(got - q) <= bar).all()
            else:                                           # the one assertion the suite had passes on the plain form
                np.testing.assert_allclose(got, q, rtol=3e-5)


def test_small_kernel_restatements():
    ties = S.pixel_ties()
    assert ties.size == 3 * 255
    exact = np.rint((ties.astype(np.float64) + 0.5) * 255.0)
    got = S.pixels_float_f32(ties)
    assert got.min() == 0 and got.max() >= 254 and (np.abs(got - exact) <= 1).all()
    assert (S.pixels_float_f32(np.float32([-0.6, -0.5, -0.0, 0.0, 0.5, 0.6])) == [0, 0, 128, 128, 255, 255]).all()
    x = np.arange(2 * 3 * 5 * 1, dtype=np.float32).reshape(2, 3, 5, 1)
    np.testing.assert_array_equal(S.emulate_pool(x), O._avg_pool2_symmetric(x.astype(np.float64)))


def test_finish_reference_equals_the_host_finish():
    from shallow_ntc_amd import ops
    rng = np.random.default_rng(5)
    for scales, n, c in ((1, 3, 3), (5, 4, 1), (5, 2, 3)):
        counts = [float(k) for k in rng.integers(1, 900, scales)]
        sums = rng.uniform(0.2, 1.0, (scales, 2, n, c)) * np.asarray(counts).reshape(-1, 1, 1, 1)
        q, coef = S.finish_reference(sums, counts, scales == 1, -7.5)
        np.testing.assert_allclose(q, ops.image_quality_finish(sums, counts, scales == 1), rtol=1e-13)
        eps = 1e-6                                          # coef = d (weight q_i) / d sum_k, by central differences
        k, i, ch = scales - 1, n - 1, c - 1
        which = 0 if k == scales - 1 else 1
        hi, lo = sums.copy(), sums.copy()
        hi[k, which, i, ch] += eps
        lo[k, which, i, ch] -= eps
        fd = -7.5 * (S.finish_reference(hi, counts, scales == 1, 1.0)[0][i] - S.finish_reference(lo, counts, scales == 1, 1.0)[0][i]) / (2 * eps)
        np.testing.assert_allclose(coef[k, i, ch], fd, rtol=1e-5)
    sums = np.ones((5, 2, 2, 3))
    sums[2, 1, 0, 1] = -0.5
    sums[4, 0, 1, 2] = 0.0
    q, coef = S.finish_reference(sums, [1.0] * 5, False, 1.0)
    assert (coef[:, 0, 1] == 0).all() and (coef[:, 1, 2] == 0).all() and (coef[:, 0, 0] != 0).all()
    np.testing.assert_allclose(q, [2 / 3, 2 / 3], rtol=1e-15)
