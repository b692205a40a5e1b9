"""(MS-)SSIM as a differentiable distortion, the parts that need no GPU: the ABI of csrc/msssim_grad.hip, and a float64
PyTorch restatement of the loss of DESIGN.md 4.6 -- the function tests/test_hip_msssim_grad.py differentiates -- pinned to the
oracle's ``image_quality``."""
import re
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ops_np as O

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ("sntc_msssim_inputs", "sntc_msssim_finish", "sntc_ssim_scale_grad", "sntc_avgpool2_symmetric_grad")
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


# ---- the restatement -----------------------------------------------------------------------------------------------
def _window():
    c = torch.arange(11, dtype=torch.float64) - 5.0
    g = torch.exp(-0.5 * c * c / (1.5 * 1.5))
    return g / g.sum()


def _filter(x):
    """Depthwise 11-tap sigma 1.5 Gaussian, VALID, over H then W of an NCHW tensor."""
    c = x.shape[1]
    win = _window().to(x)
    x = F.conv2d(x, win.reshape(1, 1, 11, 1).repeat(c, 1, 1, 1), groups=c)
    return F.conv2d(x, win.reshape(1, 1, 1, 11).repeat(c, 1, 1, 1), groups=c)


def _maps(a, b, max_val=255.0):
    """-> (mean ssim[n, c], mean cs[n, c]) of one scale."""
    c1, c2 = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
    m0, m1 = _filter(a), _filter(b)
    num0, den0 = 2.0 * m0 * m1, m0 * m0 + m1 * m1
    lum = (num0 + c1) / (den0 + c1)
    cs = (2.0 * _filter(a * b) - num0 + c2) / (_filter(a * a + b * b) - den0 + c2)
    return (lum * cs).mean(dim=(2, 3)), cs.mean(dim=(2, 3))


def _pool(x):
    """2 x 2 average pool after repeating the last row / column of an odd size (tf.pad SYMMETRIC by one)."""
    h, w = x.shape[2], x.shape[3]
    if h % 2 or w % 2:
        x = F.pad(x, (0, w % 2, 0, h % 2), mode="replicate")
    return F.avg_pool2d(x, 2)


def quality(a, b):
    """Per-image q_i of DESIGN.md 4.6 for float64 NHWC tensors of 0-255 pixel values: single-scale SSIM when both sides
    are < 160, five-scale MS-SSIM otherwise.  A factor clamped at 0 gives its (image, channel) product the value 0 and a zero
    gradient (no 0 / 0)."""
    h, w = a.shape[1], a.shape[2]
    a, b = a.permute(0, 3, 1, 2), b.permute(0, 3, 1, 2)
    if h < 160 and w < 160:
        return _maps(a, b)[0].mean(dim=-1)
    factors = []
    for k in range(len(WEIGHTS)):
        if k > 0:
            a, b = _pool(a), _pool(b)
        s, cs = _maps(a, b)
        factors.append(s if k == len(WEIGHTS) - 1 else cs)
    f = torch.stack(factors, dim=-1)                                       # [n, c, scales]
    positive = (f > 0).all(dim=-1)
    safe = torch.where(f > 0, f, torch.ones_like(f))
    prod = torch.prod(safe ** torch.tensor(WEIGHTS, dtype=f.dtype), dim=-1)
    return torch.where(positive, prod, torch.zeros_like(prod)).mean(dim=-1)


def distortion(a, b):
    """D = 1 - mean_B q_i."""
    return 1.0 - quality(a, b).mean()


def smooth_pair(n, h, w, c=3, rounded=False, seed=None):
    """The images of test_hip_ops.py::test_ms_ssim (a smooth pattern with noise); unrounded unless asked."""
    rng = np.random.default_rng(h + w if seed is None else seed)
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([128 + 70 * np.sin(xx / 11 + k) * np.cos(yy / 6 - k) for k in range(c)], -1)[None] + rng.normal(0, 6, size=(n, h, w, c))
    b = a + rng.normal(0, 9, size=a.shape)
    if rounded:
        a, b = np.rint(a), np.rint(b)
    return np.clip(a, 0, 255).astype(np.float32), np.clip(b, 0, 255).astype(np.float32)


def clamp_pair(n=2, h=176, w=192):
    """A pair whose channel 1 of image 0 has a NEGATIVE mean cs on scale 0 only: a pixel checkerboard of opposite sign in a and
    b (anti-correlated at full resolution, removed by the first 2 x 2 pool)."""
    a, b = smooth_pair(n, h, w, seed=77)
    yy, xx = np.mgrid[0:h, 0:w]
    checker = (40.0 * (1 - 2 * ((yy + xx) % 2))).astype(np.float32)
    base = np.clip(a[0, :, :, 1], 45, 210)
    a[0, :, :, 1] = base + checker
    b[0, :, :, 1] = base - checker
    return a, b


# ---- tests ---------------------------------------------------------------------------------------------------------
def test_entry_points_declared_bound_and_exported():
    from shallow_ntc_amd import _capi
    header = (ROOT / "include" / "sntc.h").read_text()
    lib = _capi.load()
    for name in ENTRY_POINTS:
        assert re.search(rf"\bint {name}\(", header), f"{name} is not declared in include/sntc.h"
        assert name in _capi.SIGNATURES, f"{name} is missing from the _capi signature table"
        assert hasattr(lib, name), f"libsntc_hip.so does not export {name}"
        assert _capi.SIGNATURES[name][1][-1] is _capi.C.c_void_p                      # every entry point takes a stream
    assert "msssim_grad.hip" in (ROOT / "shallow-ntc_amd" / "csrc" / "Makefile").read_text()


def test_scale_rule_and_refusals():
    import pytest
    from shallow_ntc_amd import ops
    assert ops.msssim_scale_sizes(100, 120) == [(100, 120)]
    assert ops.msssim_scale_sizes(161, 187) == [(161, 187), (81, 94), (41, 47), (21, 24), (11, 12)]
    assert len(ops.msssim_scale_sizes(11, 40)) == 1
    for h, w in ((10, 300), (300, 10), (159, 160), (160, 400)):            # a side < 11; fifth scale below the window
        with pytest.raises(ValueError):
            ops.msssim_scale_sizes(h, w)


def test_restatement_equals_the_oracle():
    for n, h, w in ((2, 176, 200), (1, 161, 187), (2, 100, 120), (1, 11, 40)):
        for rounded in (True, False):
            a, b = smooth_pair(n, h, w, rounded=rounded)
            ref, _ = O.image_quality(a, b)
            got = quality(torch.from_numpy(a).double(), torch.from_numpy(b).double()).numpy()
            np.testing.assert_allclose(got, ref, rtol=1e-12)
    a, b = smooth_pair(1, 176, 200, c=1)
    np.testing.assert_allclose(quality(torch.from_numpy(a).double(), torch.from_numpy(b).double()).numpy(), O.image_quality(a, b)[0],
                               rtol=1e-12)


def test_clamped_factor_has_a_finite_zero_gradient():
    a, b = clamp_pair()
    at = torch.from_numpy(a).double()
    bt = torch.from_numpy(b).double().requires_grad_(True)
    _, cs = _maps(at.permute(0, 3, 1, 2), bt.permute(0, 3, 1, 2))
    assert float(cs.detach()[0, 1]) < 0 and (cs.detach().numpy().ravel()[[0, 2, 3, 4, 5]] > 0).all()
    q = quality(at, bt)
    np.testing.assert_allclose(q.detach().numpy(), O.image_quality(a, b)[0], rtol=1e-12)
    (g,) = torch.autograd.grad(1.0 - q.mean(), bt)
    g = g.numpy()
    assert np.isfinite(g).all()
    assert (g[0, :, :, 1] == 0).all()
    assert np.abs(g[0, :, :, 0]).max() > 0 and np.abs(g[1]).max() > 0
