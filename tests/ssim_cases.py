"""Input families, float64 references, per-element bars and a float32 emulation of the SSIM / MS-SSIM forward
(csrc/msssim.hip, and the input / finish kernels of csrc/msssim_grad.hip).  Shared by tests/test_hip_ssim_forward.py (the kernels
on the device) and tests/test_ssim_forward_host.py (the references, the bars and the emulation, on the CPU).

Every reference is float64 NumPy and every builder is cached: a reference is computed once per process and never written to.

The bar of one map element.  The library is built with -ffp-contract=off, so the kernel is a fixed sequence of IEEE float32
operations and  |got - ref| <= R 2^-24 S  holds to first order, S the float64 sum of the absolute values of the terms that enter
the element and R the float32 roundings on its longest path.  With a~ = a - s, b~ = b - s (s: the kernel's tile constant, below),
W the 11 x 11 window, N and D the numerator and denominator of cs:

    S_N = 2 sum W|a~ b~| + 2 (sum W|a~|)(sum W|b~|) + c2         S_D = sum W(a~^2 + b~^2) + (sum W|a~|)^2 + (sum W|b~|)^2 + c2
    bar_cs = R u (S_N + |cs| S_D) / D

the luminance factor the same way from the terms of ITS numerator and denominator, the true means |s| + sum W|a~|, and
lum * cs by the product rule plus the product's own rounding.  S is deliberately that of the CENTRED evaluation: the S of the
plain form E[x^2] - mu^2 on raw 0-255 values is 10^3 larger on bright data and would bless the cancellation.

R = 30, counted on the kernel: x x, + y y (2); an 11-term row pass and an 11-term column pass (12 each by the K + 1 convention of
tests/train_kernel_cases.py); - (mu_a^2 + mu_b^2), + c2, the division (3): 29 for cs, and lum * cs makes 30.  The window
weights are float32 roundings of the float64 window, two more relative perturbations of every term; the first addition of each
pass is to 0.0f and exact, two fewer: still 30."""
import functools

import numpy as np

from oracle import ops_np as O

U = 2.0 ** -24                     # unit roundoff of float32
U64 = 2.0 ** -53
R = 30                             # float32 roundings on the longest path of one ssim map element (module docstring)
WIN, TILE = 11, 16                 # csrc/msssim.hip kWin, kTile
TILE_IN = TILE + WIN - 1           # kIn = 26: the side of the staged input tile
# csrc/msssim.hip ssim_scale_kernel: `cy = min(oy0 + kIn / 2, h - 1), cx = min(ox0 + kIn / 2, w - 1)` -- the tile constant of the
# tile of filter outputs at (oy0, ox0) is a[cy, cx, ch], the a value at the centre of its staged inputs, clamped into the image
TILE_CENTRE = TILE_IN // 2
# csrc/msssim.hip blocks_for(): `b > 2048 ? 2048 : b` blocks of 256 threads -- one trip of the pool's and pixels_float's grid-stride loop
GRID_CAP = 2048 * 256
C1, C2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2
WEIGHTS = O.MSSSIM_WEIGHTS

FAMILIES = ("smooth", "bright", "bright_rounded", "flat_bright", "dark", "blocks", "sga_range", "checker")
HIGH_QUALITY = ("bright", "bright_rounded", "flat_bright")          # 1 - q < 5e-3: where the plain form loses its digits
TILE_SHAPES = ((11, 27), (26, 26), (27, 26), (27, 43), (43, 59), (11, 59))       # 1, 16, 17, 33, 49 filter outputs per side
CONSUMER_SHAPES = ((161, 161), (161, 187), (176, 200), (43, 59))                 # the smallest five-scale shapes, one single-scale
CONSTANT_PAIRS = ((255.0, 250.0), (0.0, 5.0), (128.0, 128.5))


def f64(a):
    return np.asarray(a, dtype=np.float64)


def window():
    return O._gauss_window(WIN, 1.5)


def window_f32():
    """The window as the launch hands it to the kernel: the float64 window rounded to float32."""
    return window().astype(np.float32)


# ---- inputs --------------------------------------------------------------------------------------------------------------
def _pattern(h, w, c, amp, base):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([base + amp * np.sin(xx / 11 + k) * np.cos(yy / 6 - k) for k in range(c)], -1)[None]


@functools.lru_cache(maxsize=None)
def pair(family, n, h, w, c):
    """-> (a, b) float32 [n, h, w, c], read-only."""
    rng = np.random.default_rng([FAMILIES.index(family), n, h, w, c])
    shape = (n, h, w, c)
    lo, hi = 0.0, 255.0
    if family == "smooth":                       # smooth_pair of tests/test_msssim_grad_host.py, unrounded
        a = _pattern(h, w, c, 70, 128) + rng.normal(0, 6, shape)
        b = a + rng.normal(0, 9, shape)
    elif family in ("bright", "bright_rounded"):
        a = _pattern(h, w, c, 10, 240) + rng.normal(0, 1, shape)
        b = a + rng.normal(0, 1.0 if family == "bright_rounded" else 0.5, shape)
        if family == "bright_rounded":
            a, b = np.rint(a), np.rint(b)
    elif family == "flat_bright":
        a = 250 + rng.uniform(-0.3, 0.3, shape)
        b = 250 + rng.uniform(-0.3, 0.3, shape)
    elif family == "dark":
        a = np.rint(_pattern(h, w, c, 6, 12) + rng.normal(0, 1, shape))
        b = np.rint(a + rng.normal(0, 1, shape))
    elif family == "blocks":                     # 0 / 255 blocks of 7 x 5 pixels
        cells = 255.0 * rng.integers(0, 2, (n, -(-h // 7), -(-w // 5), c))
        a = np.repeat(np.repeat(cells, 7, axis=1), 5, axis=2)[:, :h, :w]
        b = np.rint(a + rng.normal(0, 20, shape))
    elif family == "sga_range":                  # what the SGA step hands over: unrounded, unclamped, past both ends of 0-255
        lo, hi = -20.0, 280.0
        a = _pattern(h, w, c, 150, 130) + rng.normal(0, 6, shape)
        b = a + rng.normal(0, 9, shape)
    elif family == "checker":                    # clamp_pair of tests/test_msssim_grad_host.py: anti-correlated, cs < 0
        yy, xx = np.mgrid[0:h, 0:w]
        checker = (40.0 * (1 - 2 * ((yy + xx) % 2)))[None, :, :, None]
        base = np.clip(_pattern(h, w, c, 70, 128) + rng.normal(0, 6, shape), 45, 210)
        a, b = base + checker, base - checker
    else:
        raise KeyError(family)
    a, b = np.clip(a, lo, hi).astype(np.float32), np.clip(b, lo, hi).astype(np.float32)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def constant_pair(p, r, n, h, w, c):
    a, b = np.full((n, h, w, c), p, np.float32), np.full((n, h, w, c), r, np.float32)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def lum_closed_form(p, r):
    return (2.0 * p * r + C1) / (p * p + r * r + C1)


# ---- tiles ---------------------------------------------------------------------------------------------------------------
def tiles(h, w):
    """-> [(oy0, ox0, rows, cols, cy, cx)]: every tile of filter outputs, its valid extent and the pixel of its constant."""
    ho, wo = h - WIN + 1, w - WIN + 1
    return [(oy0, ox0, min(TILE, ho - oy0), min(TILE, wo - ox0), min(oy0 + TILE_CENTRE, h - 1), min(ox0 + TILE_CENTRE, w - 1))
            for oy0 in range(0, ho, TILE) for ox0 in range(0, wo, TILE)]


def _filter64(x, win):
    """VALID separable filter over axes 1, 2 of [n, h, w, c], float64."""
    k = len(win)
    h, w = x.shape[1], x.shape[2]
    t = sum(win[j] * x[:, :, j:j + w - k + 1] for j in range(k))
    return sum(win[i] * t[:, i:i + h - k + 1] for i in range(k))


# ---- the float64 reference of every map element and its bar ----------------------------------------------------------------
def element_stats(a, b):
    """-> dict of float64 [n, ho, wo, c] arrays: cs, lum, ssim (= lum cs) and bar_cs, bar_lum, bar_ssim."""
    a, b = f64(a), f64(b)
    n, h, w, c = a.shape
    win = window()
    out = {k: np.zeros((n, h - WIN + 1, w - WIN + 1, c)) for k in ("cs", "lum", "ssim", "bar_cs", "bar_lum", "bar_ssim")}
    for oy0, ox0, rows, cols, cy, cx in tiles(h, w):
        s = a[:, cy, cx, :][:, None, None, :]
        ta = a[:, oy0:oy0 + rows + WIN - 1, ox0:ox0 + cols + WIN - 1] - s
        tb = b[:, oy0:oy0 + rows + WIN - 1, ox0:ox0 + cols + WIN - 1] - s
        m0, m1, exy, esq = _filter64(ta, win), _filter64(tb, win), _filter64(ta * tb, win), _filter64(ta * ta + tb * tb, win)
        fa, fb, fab = _filter64(np.abs(ta), win), _filter64(np.abs(tb), win), _filter64(np.abs(ta * tb), win)
        num, den = 2.0 * exy - 2.0 * m0 * m1 + C2, esq - m0 * m0 - m1 * m1 + C2
        cs = num / den
        bar_cs = R * U * ((2.0 * fab + 2.0 * fa * fb + C2) + np.abs(cs) * (esq + fa * fa + fb * fb + C2)) / den
        ma, mb = m0 + s, m1 + s                                    # the true means
        sa, sb = np.abs(s) + fa, np.abs(s) + fb
        den0 = ma * ma + mb * mb + C1
        lum = (2.0 * ma * mb + C1) / den0
        bar_lum = R * U * ((2.0 * sa * sb + C1) + np.abs(lum) * (sa * sa + sb * sb + C1)) / den0
        ssim = lum * cs
        bar_ssim = np.abs(lum) * bar_cs + np.abs(cs) * bar_lum + U * np.abs(ssim)
        sl = (slice(None), slice(oy0, oy0 + rows), slice(ox0, ox0 + cols))
        for k, v in (("cs", cs), ("lum", lum), ("ssim", ssim), ("bar_cs", bar_cs), ("bar_lum", bar_lum), ("bar_ssim", bar_ssim)):
            out[k][sl] = v
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def family_stats(family, n, h, w, c):
    return element_stats(*pair(family, n, h, w, c))


def mean_stats(st):
    """element_stats -> (ssim[n, c], cs[n, c], bar_ssim[n, c], bar_cs[n, c]): the spatial means and the means of the bars."""
    return tuple(st[k].mean(axis=(1, 2)) for k in ("ssim", "cs", "bar_ssim", "bar_cs"))


def worst_ratio(got, ref, bar):
    """max |got - ref| / bar; <= 1 passes."""
    return float((np.abs(f64(got) - f64(ref)) / bar).max())


# ---- the quality the consumers read, and the bar of it -----------------------------------------------------------------------
def pool64(x):
    return O._avg_pool2_symmetric(f64(x))


def quality_with_bar(a, b):
    """-> (q[n], bar[n]) of ops.image_quality: single-scale SSIM below 160 x 160, five-scale MS-SSIM otherwise.

    First-order propagation through q = mean_c prod_k f_k^{w_k}:  dq <= mean_c sum_k w_k (prod / f_k) df_k, with df_k the mean of
    the per-element bars of scale k plus, on the scales below the first, what the float32 pyramid adds: every pool level rounds
    4 times against the magnitude of its inputs (the bar of the pool kernel), so the inputs of scale k are off by at most
    4 k u A_k (A_k: the largest magnitude at that scale), which moves cs by at most 2 (1 + |cs|)(sigma_a + sigma_b) / D of it
    (d N / d b(r) = 2 W(r) (a(r) - mu_a), sum W |a - mu_a| <= sigma_a, and alike for D) and lum by at most
    2 (|mu_a| + |mu_b|)(1 + lum) / D_lum of it."""
    a, b = f64(a), f64(b)
    h, w = a.shape[1], a.shape[2]
    if h < 160 and w < 160:
        ssim, _, bar_ssim, _ = mean_stats(element_stats(a, b))
        return ssim.mean(axis=-1), bar_ssim.mean(axis=-1)
    win = window()
    factors, bars = [], []
    for k in range(len(WEIGHTS)):
        if k > 0:
            a, b = pool64(a), pool64(b)
        st = element_stats(a, b)
        ssim, cs, bar_ssim, bar_cs = mean_stats(st)
        last = k == len(WEIGHTS) - 1
        f, bar = (ssim, bar_ssim) if last else (cs, bar_cs)
        if k > 0:
            delta = 4 * k * U * max(np.abs(a).max(), np.abs(b).max())
            m0, m1 = _filter64(a, win), _filter64(b, win)
            va, vb = np.maximum(_filter64(a * a, win) - m0 * m0, 0.0), np.maximum(_filter64(b * b, win) - m1 * m1, 0.0)
            moved = 2.0 * (1.0 + np.abs(st["cs"])) * (np.sqrt(va) + np.sqrt(vb)) / (va + vb + C2) * delta
            if last:
                moved = st["lum"] * moved + np.abs(st["cs"]) * 2.0 * (np.abs(m0) + np.abs(m1)) * (1.0 + st["lum"]) / (m0 * m0 + m1 * m1 + C1) * delta
            bar = bar + moved.mean(axis=(1, 2))
        factors.append(np.maximum(f, 0.0))
        bars.append(bar)
    f, bar = np.stack(factors, -1), np.stack(bars, -1)                      # [n, c, scales]
    wts = np.asarray(WEIGHTS)
    prod = np.prod(f ** wts, axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        dq = np.where(f > 0, wts * prod[..., None] / f * bar, 0.0).sum(axis=-1)
    return prod.mean(axis=-1), dq.mean(axis=-1)


@functools.lru_cache(maxsize=None)
def family_quality(family, n, h, w, c):
    return quality_with_bar(*pair(family, n, h, w, c))


def db(q):
    with np.errstate(divide="ignore"):
        return -10.0 * np.log10(1.0 - f64(q))


# ---- the float32 emulation of ssim_scale_kernel (tests/test_ssim_forward_host.py only) ---------------------------------------
def emulate(a, b, centred):
    """The kernel's float32 operations in the kernel's order: per tile, staging (minus the tile constant when ``centred``), the
    11-tap row pass in j order, the column pass in i order, the same formulas.  ``centred=False`` is the plain form on raw
    values.  -> (ssim, cs) float32 maps [n, ho, wo, c]; the kernel adds them up in float64."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    n, h, w, c = a.shape
    win = window_f32()
    c1 = np.float32(np.float32(0.01) * np.float32(255)) * np.float32(np.float32(0.01) * np.float32(255))
    c2 = np.float32(np.float32(0.03) * np.float32(255)) * np.float32(np.float32(0.03) * np.float32(255))
    two = np.float32(2)
    ssim, cs_map = (np.zeros((n, h - WIN + 1, w - WIN + 1, c), np.float32) for _ in range(2))
    for oy0, ox0, rows, cols, cy, cx in tiles(h, w):
        s = a[:, cy, cx, :][:, None, None, :] if centred else np.float32(0)
        x = a[:, oy0:oy0 + rows + WIN - 1, ox0:ox0 + cols + WIN - 1] - s
        y = b[:, oy0:oy0 + rows + WIN - 1, ox0:ox0 + cols + WIN - 1] - s
        xy, sq = x * y, x * x + y * y
        r = [np.zeros((n, rows + WIN - 1, cols, c), np.float32) for _ in range(4)]
        for j in range(WIN):
            for acc, v in zip(r, (x, y, xy, sq)):
                acc += win[j] * v[:, :, j:j + cols]
        m = [np.zeros((n, rows, cols, c), np.float32) for _ in range(4)]
        for i in range(WIN):
            for acc, v in zip(m, r):
                acc += win[i] * v[:, i:i + rows]
        m0, m1, exy, esq = m
        cs = (two * exy - two * m0 * m1 + c2) / (esq - (m0 * m0 + m1 * m1) + c2)
        t0, t1 = m0 + s, m1 + s
        lum = (two * t0 * t1 + c1) / (t0 * t0 + t1 * t1 + c1)
        sl = (slice(None), slice(oy0, oy0 + rows), slice(ox0, ox0 + cols))
        ssim[sl], cs_map[sl] = lum * cs, cs
    assert ssim.dtype == np.float32 and cs_map.dtype == np.float32
    return ssim, cs_map


def emulate_pool(x):
    """avgpool2_kernel in float32: 0.25f * (((p00 + p01) + p10) + p11), an odd size extended by its last row / column."""
    x = np.asarray(x, np.float32)
    h, w = x.shape[1], x.shape[2]
    y0, y1 = np.arange(0, h, 2), np.minimum(np.arange(0, h, 2) + 1, h - 1)
    x0, x1 = np.arange(0, w, 2), np.minimum(np.arange(0, w, 2) + 1, w - 1)
    g = lambda ys, xs: x[:, ys][:, :, xs]
    return np.float32(0.25) * (((g(y0, x0) + g(y0, x1)) + g(y1, x0)) + g(y1, x1))


def emulate_quality(a, b, centred):
    """ops.image_quality on the emulated kernels (float32 pyramid, float64 sums, the host finish)."""
    h, w = a.shape[1], a.shape[2]
    if h < 160 and w < 160:
        return f64(emulate(a, b, centred)[0]).mean(axis=(1, 2)).mean(axis=-1)
    factors = []
    for k in range(len(WEIGHTS)):
        if k > 0:
            a, b = emulate_pool(a), emulate_pool(b)
        ssim, cs = emulate(a, b, centred)
        factors.append(np.maximum(f64(ssim if k == len(WEIGHTS) - 1 else cs).mean(axis=(1, 2)), 0.0))
    return np.prod(np.stack(factors, -1) ** np.asarray(WEIGHTS), axis=-1).mean(axis=-1)


# ---- float32 restatements of the small kernels ------------------------------------------------------------------------------
def pixels_float_f32(v):
    """pixels_float_kernel: rint((v + .5f) 255f) clamped to 0-255, every operation in float32."""
    v = np.asarray(v, np.float32)
    return np.clip(np.rint((v + np.float32(0.5)) * np.float32(255)), np.float32(0), np.float32(255)).astype(np.float32)


def pixel_values_f32(v):
    """msssim_inputs_kernel: (v + .5f) 255f in float32, unrounded and unclamped."""
    return ((np.asarray(v, np.float32) + np.float32(0.5)) * np.float32(255)).astype(np.float32)


def pixel_ties():
    """Every v with (v + .5) 255 at k + .5 for k = 0 .. 254, as float32, and its float32 neighbours."""
    t = ((np.arange(255) + 0.5) / 255.0 - 0.5).astype(np.float32)
    return np.concatenate([t, np.nextafter(t, np.float32(1)), np.nextafter(t, np.float32(-1))])


# ---- sntc_msssim_finish ---------------------------------------------------------------------------------------------------
def finish_reference(sums, counts, single, weight):
    """float64 restatement of DESIGN.md 4.6: sums [scales, 2, n, c] -> (q[n], coef[scales, n, c])."""
    sums = f64(sums)
    scales, _, n, c = sums.shape
    if single:
        return (sums[0, 0] / counts[0]).mean(axis=-1), np.full((1, n, c), weight / c / counts[0])
    wts = np.asarray(WEIGHTS[:scales])
    means = np.stack([sums[k, 0 if k == scales - 1 else 1] / counts[k] for k in range(scales)], -1)      # [n, c, scales]
    f = np.maximum(means, 0.0)
    positive = (f > 0).all(axis=-1)
    prod = np.where(positive, np.prod(np.where(f > 0, f, 1.0) ** wts, axis=-1), 0.0)
    coef = np.where(positive[..., None], weight / c * prod[..., None] * wts / np.where(f > 0, f, 1.0) / np.asarray(counts), 0.0)
    return prod.mean(axis=-1), np.moveaxis(coef, -1, 0)


def finish_q_bar(q_ref, scales, c):
    """Per (image, channel) the kernel rounds in float64: a division, ``pow`` (within 2 ulp; an error e of its argument moves it
    by w e <= e) and a multiplication per scale, then c additions and the division by c: 4 scales + c + 1 roundings of 2^-53,
    all terms non-negative so relative to q.  The NumPy reference rounds as often: twice that."""
    return 2.0 * (4 * scales + c + 1) * U64 * np.abs(q_ref)


def finish_coef_bar(coef_ref, scales):
    """One float32 rounding of a float64 value that itself carries the roundings of ``finish_q_bar`` and four more operations."""
    return (U + 2.0 * (4 * scales + 4) * U64) * np.abs(coef_ref)
