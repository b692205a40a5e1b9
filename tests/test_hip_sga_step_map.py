"""SGA iterative inference on a step map (-m gpu): the map sample / rate kernels against the per-image
kernels (bit for bit on a constant map) and against a float64 restatement with a step per latent position, the weighted
distortion gradient, the per-block integer SSE, the whole model's loss and gradients on a map, and
``compress(x, itinf=dict(step_offsets=...))`` end to end."""
import numpy as np
import pytest
import torch

from oracle import model_np
from oracle import ops_np as O
from test_hip_itinf_bitstream import ITINF, flushed_bits, hyper_model, images, payload_bits, slack_bar  # noqa: F401
from test_hip_sga import gumbel, make_model, t
from test_hip_sga_step import LN2, SKIP_CAP, TAU, bits_of, close, quant_of, scale_at

pytestmark = pytest.mark.gpu

N = 3


def d8(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.int8)).to(dev)


def lut_of(dev):
    from shallow_ntc_amd import entropy_coding as ec
    return ec.step_lut(dev)


def position_steps(K):
    """(step, inv_step) of every position as the kernels read them from the table: float32-rounded, float64 [n, h, w, 1]."""
    from shallow_ntc_amd import entropy_coding as ec
    table = np.array([[ec.step_size(k), ec.step_size(-k)] for k in range(ec.STEP_MIN, ec.STEP_MAX + 1)])
    at = table[np.asarray(K, np.int64) - ec.STEP_MIN]
    return at[..., 0:1], at[..., 1:2]


def map_of(kind, n, h, w):
    """mod3: position p -> (-32, 0, 32)[p mod 3]; random: seeded, uniform over the ladder; halves: -6 on the first half of the
    positions, +12 on the second.  The same map for every image but the random one."""
    hw = h * w
    p = np.arange(hw)
    if kind == "mod3":
        K = np.tile(np.array([-32, 0, 32])[p % 3], (n, 1))
    elif kind == "random":
        K = np.random.default_rng([11, h, w]).integers(-32, 33, size=(n, hw))
    else:
        K = np.tile(np.where(p < hw // 2, -6, 12), (n, 1))
    return K.reshape(n, h, w).astype(np.int8)


# ---- the float64 restatement: test_hip_sga_step.restate's formulas with step, inverse step and k per position ------------
def restate_map(y, mu, raw, g, tau, K):
    step, inv = position_steps(K)
    k = np.asarray(K, np.float64)[..., None]
    y, mu, raw, g = (np.asarray(a, np.float64) for a in (y, mu, raw, g))
    u = (y - mu) * inv
    v = O.sga_round(u, tau, g)
    h = 1e-6
    sp = (O.sga_round(u + h, tau, g) - O.sga_round(u - h, tau, g)) / (2 * h)
    sigma, e, j = scale_at(raw, k)
    bits = bits_of(v, sigma)
    hv = 1e-5
    dv = (bits_of(v + hv, sigma) - bits_of(v - hv, sigma)) / (2 * hv)
    dsig = (bits_of(v, sigma * (1 + hv)) - bits_of(v, sigma * (1 - hv))) / (2 * hv * sigma)
    inner = (e <= 63.0) | (dsig > 0.0)                        # identity-if-towards on the reference's clamp
    outer = (j >= 0.0) & (j <= 63.0)                          # the plain clamp gradient on this project's own
    dr = dsig * sigma * O.SCALE_FACTOR * e * inner * outer
    skip = (np.abs(u - np.rint(u)) < 1e-2) | (np.abs(j) < 1e-3) | (np.abs(j - 63.0) < 1e-3) | (np.abs(e - 63.0) < 1e-3)
    return dict(u=u, v=v, yt=step * v + mu, sp=sp, bits=bits, dv=dv, dr=dr, j=j, skip=skip)


def plant_integers(y, mu, K, rng, share=0.005):
    """test_hip_sga_step.plant_integers with a step per position: move a few y (and, where that fails, their mu to 0) so that
    the KERNEL's float32 u = (y - mu) * inv_step(K_p) is an exact integer.  Returns how many were placed."""
    step, inv = position_steps(K)
    placed = 0
    per = y[0].size
    for i in range(y.shape[0]):
        for fi in rng.choice(per, size=min(40, max(2, int(share * per))), replace=False):
            idx = (i,) + np.unravel_index(fi, y.shape[1:])
            st, inv32 = step[idx[:3] + (0,)], np.float32(inv[idx[:3] + (0,)])
            s = np.float32(rng.choice([-7, -3, -1, 0, 1, 2, 3, 5, 6, 11]))
            for m in (mu[idx], np.float32(0.0)):
                lo = hi = np.float32(np.float64(m) + np.float64(s) * st)
                for _ in range(33):
                    hit = [c for c in (lo, hi) if np.float32(np.float32(c - m) * inv32) == s]
                    if hit:
                        break
                    lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
                if hit:
                    y[idx], mu[idx] = hit[0], m
                    placed += 1
                    break
    return placed


def draw(rng, n, h, w, c, K):
    mu = rng.standard_normal((n, h, w, c)).astype(np.float32)
    raw = rng.uniform(-2.5, 4.5, size=mu.shape).astype(np.float32)
    y = (mu + position_steps(K)[0] * rng.laplace(0, 2, size=mu.shape)).astype(np.float32)
    return y, mu, raw, gumbel(rng, mu.shape)


def make_inputs(n, h, w, c, K, code, plant=True):
    """test_hip_sga_step.make_inputs on a map: y = mu + step(K_p) Laplace(0, 2); the seed is the first whose float64 restatement
    skips at most SKIP_CAP of the elements."""
    for seed in range(64):
        rng = np.random.default_rng([seed, n, h, w, c, code])
        y, mu, raw, g = draw(rng, n, h, w, c, K)
        planted = plant_integers(y, mu, K, rng) if plant and mu[0].size >= 400 else 0
        ref = restate_map(y, mu, raw, g, TAU, K)
        if ref["skip"].mean() <= SKIP_CAP and np.abs(ref["u"]).max() <= 60.0:
            return dict(y=y, mu=mu, raw=raw, g=g, hyper=np.concatenate([mu, raw], -1), ref=ref, planted=planted, seed=seed)
    raise AssertionError("no seed keeps the restatement's skipped share under the cap")


# ---- 1. a constant map is the per-image kernel pair, bit for bit ------------------------------------------------------------
@pytest.mark.parametrize("h,w,c", [(3, 5, 8), (7, 37, 5)], ids=["c8-vector", "c5-scalar"])
def test_constant_map_is_the_per_image_kernels(h, w, c, dev):
    from shallow_ntc_amd import ops
    ks = [-32, 5, 32]
    K = np.array(ks, np.int8).reshape(N, 1, 1) * np.ones((N, h, w), np.int8)
    y, mu, raw, g = draw(np.random.default_rng(h * w), N, h, w, c, K)
    yd, hd, gd, kd, lut = t(y, dev), t(np.concatenate([mu, raw], -1), dev), t(g, dev), d8(K, dev), lut_of(dev)
    quant = quant_of(ks, dev)                                    # dweight = 1
    for noise, seed, step in ((gd, 0, 0), (None, 7, 3)):         # supplied noise; the generator with the same (seed, step)
        old = ops.sga_normal_step_fwd(yd, hd, TAU, quant, noise, seed, step)
        new = ops.sga_normal_step_map_fwd(yd, hd, TAU, kd, lut, noise, seed, step)
        for name, a, b in zip(("y_tilde", "sprime", "dbits_dv", "dbits_draw"), old, new):
            assert torch.equal(a, b), (name, "noise" if noise is not None else "generator")
        np.testing.assert_allclose(new[4].cpu().numpy(), old[4].cpu().numpy(), rtol=1e-12)
    g_yt = t(np.random.default_rng(c).standard_normal(y.shape), dev)
    got = ops.sga_normal_step_map_bwd(g_yt, new[1], new[2], new[3], 1.0 / (N * 64 * 64), kd, lut)
    want = ops.sga_normal_step_bwd(g_yt, old[1], old[2], old[3], 1.0 / (N * 64 * 64), quant)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---- 2. the map kernels against float64 --------------------------------------------------------------------------------------
# units per image as in test_hip_sga_step: 1; 255 / 256 / 257 around one workgroup; several workgroups, the last partly idle;
# c = 5: the element-wise path; 131 200 units: every workgroup loops (one map only: its float64 restatement takes seconds)
SHAPES = [(1, 1, 4), (15, 17, 4), (8, 16, 8), (1, 257, 4), (23, 29, 8), (7, 37, 5)]
MAPS = ["mod3", "random", "halves"]
CASES = [(h, w, c, m) for m in MAPS for h, w, c in SHAPES] + [(1, 131200, 4, "mod3")]


@pytest.mark.parametrize("h,w,c,kind", CASES, ids=[f"{h}x{w}x{c}-{m}" for h, w, c, m in CASES])
def test_map_kernels_against_float64(h, w, c, kind, dev):
    from shallow_ntc_amd import entropy_coding as ec
    from shallow_ntc_amd import ops
    K = map_of(kind, N, h, w)
    case = make_inputs(N, h, w, c, K, MAPS.index(kind))
    ref = case["ref"]
    ok = ~ref["skip"]
    share = float(ref["skip"].mean())
    print(f"\n{h}x{w}x{c} {kind}: seed {case['seed']}, skipped {share:.4f}, planted integer u {case['planted']}, max |u| {np.abs(ref['u']).max():.1f}")
    assert share <= SKIP_CAP
    yd, hd, gd, kd, lut = t(case["y"], dev), t(case["hyper"], dev), t(case["g"], dev), d8(K, dev), lut_of(dev)
    yt, sp, dv, dr, bits = (a.cpu().numpy() for a in ops.sga_normal_step_map_fwd(yd, hd, TAU, kd, lut, gd))
    step, inv = position_steps(K)
    mu64 = case["mu"].astype(np.float64)
    close((yt.astype(np.float64) - mu64) / step, ref["v"], ok, 0.0, 3e-5, "sample v")
    np.testing.assert_allclose(bits, ref["bits"].sum(axis=(1, 2, 3)), rtol=2e-5)
    for got, name in ((sp, "sp"), (dv, "dv"), (dr, "dr")):
        close(got.astype(np.float64), ref[name], ok, 3e-3, 1e-3, name)
    # the plain clamp gradient of the outer clamp: exactly zero off the ladder's ends
    off = (ref["j"] < -1e-3) | (ref["j"] > 63.0 + 1e-3)
    assert (dr[off] == 0.0).all()
    if kind == "mod3" and h * w >= 3:
        assert off.any() and (dr[~off] != 0.0).any()               # the ends are reached, and the middle is live
    # where the kernel's own u is an integer, y~ is the coder's value of the coder's symbol (the map kernels of the coder)
    u32 = (case["y"] - case["mu"]) * inv.astype(np.float32)
    assert u32.dtype == np.float32
    exact = u32 == np.rint(u32)
    if c % 4 == 0 and case["planted"]:
        assert all(exact[i].sum() >= 2 for i in range(N))
        sym, _ = ops.step_map_symbols(yd, hd, ec.scale_table_ids(hd), kd, lut)
        coder = ops.dequant_step_map(sym, hd, kd, lut).cpu().numpy()
        np.testing.assert_array_equal(sym.cpu().numpy()[exact], u32[exact].astype(np.int32))
        np.testing.assert_array_equal(yt[exact].view(np.uint32), coder[exact].view(np.uint32))
    # backward: the three formulas in float64 on the forward outputs; no dweight
    rng = np.random.default_rng(h * w)
    g_yt = rng.standard_normal(yt.shape).astype(np.float32)
    wgt = 0.37
    g_y, g_h = (a.cpu().numpy().astype(np.float64)
                for a in ops.sga_normal_step_map_bwd(t(g_yt, dev), t(sp, dev), t(dv, dev), t(dr, dev), wgt, kd, lut))
    a = sp.astype(np.float64) * inv
    dvw = np.float64(np.float32(wgt)) * dv
    g = g_yt.astype(np.float64)
    every = np.ones(yt.shape, bool)
    close(g_y, (g * step + dvw) * a, every, 3e-3, 1e-3, "g_yloc")
    close(g_h[..., :c], g * (1.0 - step * a) - dvw * a, every, 3e-3, 1e-3, "g_mu")
    close(g_h[..., c:], np.float64(np.float32(wgt)) * dr, every, 3e-3, 1e-3, "g_raw")


def test_unaligned_view_and_stray_map_bytes(dev):
    """A y_loc that starts 4 bytes into its allocation takes the element-wise path: the same element-wise outputs.  Map bytes of
    +-64 are clamped in the kernel before they index the table: the result of the map clipped on the host."""
    from shallow_ntc_amd import ops
    h, w, c = 8, 16, 8
    K = map_of("random", N, h, w)
    y, mu, raw, g = draw(np.random.default_rng(1), N, h, w, c, K)
    yd, hd, gd, kd, lut = t(y, dev), t(np.concatenate([mu, raw], -1), dev), t(g, dev), d8(K, dev), lut_of(dev)
    want = ops.sga_normal_step_map_fwd(yd, hd, TAU, kd, lut, gd)
    shifted = torch.cat([torch.zeros(1, device=dev), yd.flatten()])[1:].view(yd.shape)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    for noise in (gd, None):
        a = ops.sga_normal_step_map_fwd(yd, hd, TAU, kd, lut, noise, 5, 2)
        b = ops.sga_normal_step_map_fwd(shifted, hd, TAU, kd, lut, noise, 5, 2)
        for u, v in zip(a[:4], b[:4]):
            assert torch.equal(u, v)
        np.testing.assert_allclose(b[4].cpu().numpy(), a[4].cpu().numpy(), rtol=1e-12)
    g_yt = t(np.random.default_rng(2).standard_normal(y.shape), dev)
    gs = torch.cat([torch.zeros(1, device=dev), g_yt.flatten()])[1:].view(g_yt.shape)
    a = ops.sga_normal_step_map_bwd(g_yt, want[1], want[2], want[3], 0.37, kd, lut)
    b = ops.sga_normal_step_map_bwd(gs, want[1], want[2], want[3], 0.37, kd, lut)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    stray = K.copy()
    stray[:, 0, :4] = [64, -64, 33, -33]
    stray[:, -1, -1] = 127
    clipped = np.clip(stray, -32, 32)
    assert (stray != clipped).sum() >= 5 * N
    a = ops.sga_normal_step_map_fwd(yd, hd, TAU, d8(stray, dev), lut, gd)
    b = ops.sga_normal_step_map_fwd(yd, hd, TAU, d8(clipped, dev), lut, gd)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    a = ops.sga_normal_step_map_bwd(g_yt, want[1], want[2], want[3], 0.37, d8(stray, dev), lut)
    b = ops.sga_normal_step_map_bwd(g_yt, want[1], want[2], want[3], 0.37, d8(clipped, dev), lut)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_map_op_input_checks(dev):
    from shallow_ntc_amd import ops
    y = torch.zeros((2, 3, 4, 8), device=dev)
    hyper = torch.zeros((2, 3, 4, 16), device=dev)
    kmap, lut = torch.zeros((2, 3, 4), dtype=torch.int8, device=dev), lut_of(dev)
    ops.sga_normal_step_map_fwd(y, hyper, TAU, kmap, lut)
    for bad_map, bad_lut in ((kmap[:1], lut), (kmap.to(torch.int32), lut), (kmap.cpu(), lut), (kmap, lut[:1]), (kmap, lut.double()), (None, lut)):
        with pytest.raises(ValueError):
            ops.sga_normal_step_map_fwd(y, hyper, TAU, bad_map, bad_lut)
        with pytest.raises(ValueError):
            ops.sga_normal_step_map_bwd(y, y, y, y, 1.0, bad_map, bad_lut)
    with pytest.raises(ValueError):
        ops.sga_normal_step_map_fwd(y, hyper, TAU, kmap, lut, noise=torch.zeros((2, 3, 4, 8), device=dev))
    with pytest.raises(ValueError):
        ops.sga_normal_step_map_bwd(y, y[:1], y, y, 1.0, kmap, lut)


# ---- 3. / 4. the weighted distortion gradient and the per-block integer SSE ---------------------------------------------------
SIZES = [(60, 64, 64, 64, 16), (17, 33, 32, 48, 16), (9, 13, 16, 16, 8)]      # h x w inside hs x ws, block
SIZE_IDS = ["60x64in64x64-b16", "17x33in32x48-b16", "9x13in16x16-b8"]


def image_pair(h, w, hs, ws, seed):
    rng = np.random.default_rng([seed, h, w])
    x = rng.uniform(-0.5, 0.5, size=(2, h, w, 3)).astype(np.float32)
    xh = rng.uniform(-0.6, 0.6, size=(2, hs, ws, 3)).astype(np.float32)
    xh[:, :h, :w] = (x + 0.05 * rng.standard_normal(x.shape)).astype(np.float32)
    return x, xh


@pytest.mark.parametrize("h,w,hs,ws,block", SIZES, ids=SIZE_IDS)
def test_distortion_grad_weighted(h, w, hs, ws, block, dev):
    from shallow_ntc_amd import ops
    x, xh = image_pair(h, w, hs, ws, 0)
    xd, xhd = t(x, dev), t(xh, dev)
    hb, wb = hs // block, ws // block
    scale = 0.02 * 2.0 * 255.0 * 255.0 / (2 * h * w * 3)
    # weights of 1: the unweighted kernel, bit for bit
    g0, sse0 = ops.distortion_grad(xd, xhd, scale)
    g1, sse1, wsse1 = ops.distortion_grad_weighted(xd, xhd, scale, torch.ones((2, hb, wb), device=dev), block)
    assert torch.equal(g1, g0)
    np.testing.assert_allclose(sse1.cpu().numpy(), sse0.cpu().numpy(), rtol=1e-13)
    np.testing.assert_allclose(wsse1.cpu().numpy(), sse1.cpu().numpy(), rtol=1e-13)
    # random weights over the range 1 / step^2 spans on the ladder, log-uniform
    rng = np.random.default_rng(block)
    wts = np.exp(rng.uniform(np.log(1 / 2700.0), np.log(2700.0), size=(2, hb, wb))).astype(np.float32)
    g, sse, wsse = ops.distortion_grad_weighted(xd, xhd, scale, t(wts, dev), block)
    g = g.cpu().numpy()
    per_pixel = np.repeat(np.repeat(wts.astype(np.float64), block, axis=1), block, axis=2)[:, :h, :w, None]
    d = xh[:, :h, :w].astype(np.float64) - x.astype(np.float64)
    np.testing.assert_allclose(g[:, :h, :w], np.float64(np.float32(scale)) * per_pixel * d, rtol=2e-6, atol=0.0)
    margin = np.ones((hs, ws), bool)
    margin[:h, :w] = False
    assert margin.any() and (g[:, margin] == 0.0).all()
    np.testing.assert_allclose(wsse.cpu().numpy(), (per_pixel * (255.0 * d) ** 2).sum(axis=(1, 2, 3)), rtol=1e-6)
    np.testing.assert_allclose(sse.cpu().numpy(), sse0.cpu().numpy(), rtol=1e-13)        # the unweighted sum keeps its meaning
    # weights that do not cover the reconstruction are refused
    with pytest.raises(ValueError):
        ops.distortion_grad_weighted(xd, xhd, scale, t(wts[:, :hb - 1], dev), block)
    with pytest.raises(ValueError):
        ops.distortion_grad_weighted(xd, xhd, scale, t(wts, dev).double(), block)


def np_block_sse(x, px, block):
    a = O.floats_to_pixels(x, False).astype(np.int64)
    d2 = (a - px.astype(np.int64)) ** 2
    n, h, w, _ = x.shape
    hb, wb = -(-h // block), -(-w // block)
    pad = np.zeros((n, hb * block, wb * block, x.shape[-1]), np.int64)
    pad[:, :h, :w] = d2
    return pad.reshape(n, hb, block, wb, block, -1).sum(axis=(2, 4, 5))


def blocks_of(out):
    return out.view(torch.int32).cpu().numpy().view(np.uint32).astype(np.int64)


@pytest.mark.parametrize("h,w,hs,ws,block", SIZES, ids=SIZE_IDS)
def test_block_sse(h, w, hs, ws, block, dev):
    from shallow_ntc_amd import ops
    x, xh = image_pair(h, w, hs, ws, 1)
    x[0, 0, 0] = [0.6, -0.7, 0.5 / 255.0]                        # saturation at both ends, and a tie
    xd, xhd = t(x, dev), t(xh, dev)
    sse, px = ops.pixels_sse(xd, xhd, want_pixels=True)
    got = ops.block_sse(xd, px, block)
    assert got.dtype == torch.uint32 and tuple(got.shape) == (2, -(-h // block), -(-w // block))
    got = blocks_of(got)
    np.testing.assert_array_equal(got, np_block_sse(x, px.cpu().numpy(), block))
    assert got.sum(axis=(1, 2)).tolist() == sse.cpu().numpy().tolist()
    # independent of the pixels' origin: any uint8 image, here noise
    noise = torch.from_numpy(np.random.default_rng(3).integers(0, 256, size=(2, h, w, 3), dtype=np.uint8)).to(dev)
    np.testing.assert_array_equal(blocks_of(ops.block_sse(xd, noise, block)), np_block_sse(x, noise.cpu().numpy(), block))


def test_block_sse_overflow_bound(dev):
    """The sums are 32-bit: block^2 c 255^2 < 2^32 is checked.  For c = 3 that is block <= 148 (148^2 x 3 x 255^2 = 4 272 922 800 <
    2^32 = 4 294 967 296 < 149^2 x 3 x 255^2).  block = 64 runs; so does 128 (128^2 x 3 x 255^2 = 3 196 108 800: below the bound,
    not above it); the worst case of the largest block is exact; 149 and beyond are refused."""
    from shallow_ntc_amd import _capi as capi
    from shallow_ntc_amd import ops
    assert 148 ** 2 * 3 * 255 ** 2 < 2 ** 32 <= 149 ** 2 * 3 * 255 ** 2 and 128 ** 2 * 3 * 255 ** 2 < 2 ** 32
    x = torch.full((1, 148, 150, 3), -0.5, device=dev)           # pixels 0 against 255 everywhere: the largest error there is
    px = torch.full((1, 148, 150, 3), 255, dtype=torch.uint8, device=dev)
    for block in (64, 128, 148):
        got = blocks_of(ops.block_sse(x, px, block))
        rows = np.minimum(block, 148 - block * np.arange(got.shape[1]))[:, None]
        cols = np.minimum(block, 150 - block * np.arange(got.shape[2]))[None, :]
        np.testing.assert_array_equal(got[0], rows * cols * 3 * 255 ** 2)
    assert got[0, 0, 0] == 148 ** 2 * 3 * 255 ** 2
    for block in (149, 256, 65536):
        with pytest.raises(capi.SntcError) as err:
            ops.block_sse(x, px, block)
        assert err.value.code == capi.ERR_BAD_SHAPE
    with pytest.raises(capi.SntcError):                           # more channels, a smaller bound: 16^2 x 300 x 255^2 > 2^32
        ops.block_sse(torch.zeros((1, 16, 16, 300), device=dev), torch.zeros((1, 16, 16, 300), dtype=torch.uint8, device=dev), 16)
    with pytest.raises(ValueError):
        ops.block_sse(x, px[:, :100], 16)


# ---- 5. the whole model on a map: test_sga_loss_and_gradients_at_a_step with a step per position ---------------------------------
def test_sga_loss_and_gradients_on_a_map(dev):
    """GPU loss terms == the restated float64 loss mean_B(bits_i) / (H W) + (lambda / n) sum_i Dw_i on a map that varies inside
    both images, with the same Gumbel noise; GPU gradients == central differences of it."""
    from shallow_ntc_amd import entropy_coding as ec
    from shallow_ntc_amd.common import data_lib
    model, w, tc = make_model(dev)
    lam, ks, tau = 0.02, [-5, 7], 0.5
    ref_model = model_np.Model(tc, rd_lambda=lam)
    ms, bs, fs = model_np._prior_lists(w)
    x = data_lib.normalize_image(data_lib.synthetic_images(2, 60, 64, seed=9))        # pads to 64 x 64: 4 x 4 positions of 16 pixels
    n, H, W, _ = x.shape
    assert model.step_offsets_shape(H, W) == (4, 4)
    off = np.tile(np.array([0, 3, -3, 0], np.int8), (2, 4, 1))
    off[1] = off[1].T
    model.initialize_itinf(x, step=ks, step_offsets=off)
    K = ec.index_map(ks, off)
    q = model._itinf_grid
    assert q["grid"].kind == "map" and q["lam"] is None and (q["grid"].kmap == K).all() and q["block"] == 16 and q["weight"][1] == 16
    assert all(len(np.unique(K[i])) == 3 for i in range(n))
    step, inv = position_steps(K)
    omega = ec.position_weights(K)
    pixel_w = np.repeat(np.repeat(omega, 16, axis=1), 16, axis=2)[:, :H, :W, None]
    z0 = model.latent_rvs.uq[0].loc.cpu().numpy().astype(np.float64)
    y0 = model.latent_rvs.uq[1].loc.cpu().numpy().astype(np.float64)
    rng = np.random.default_rng(3)
    gz, gy = gumbel(rng, z0.shape), gumbel(rng, y0.shape)

    def image_terms(i, z, y):
        """(bits_z, bits_y, sse, wsse, u) of image i for latents z, y of that image alone ([1, ...])."""
        z_t = O.sga_round(z, tau, gz[i:i + 1].astype(np.float64), offset=0.0)
        bits_z = O.deep_factorized_logprob(z_t, ms, bs, fs).sum() / -LN2
        hyp = ref_model._run(ref_model.hyper_synthesis, w, "hyper_synthesis/", z_t, None)
        c = hyp.shape[-1] // 2
        mu, raw = hyp[..., :c], hyp[..., c:]
        u = (y - mu) * inv[i:i + 1]
        v = O.sga_round(u, tau, gy[i:i + 1].astype(np.float64))
        bits_y = bits_of(v, scale_at(raw, K[i:i + 1].astype(np.float64)[..., None])[0]).sum()
        recon = O.unpad_images(ref_model._run(ref_model.synthesis, w, "synthesis/", step[i:i + 1] * v + mu, None), x[i:i + 1].shape)
        d2 = (O.floats_to_pixels(x[i:i + 1].astype(np.float64), True) - O.floats_to_pixels(recon, True)) ** 2
        return bits_z, bits_y, float(d2.sum()), float((pixel_w[i:i + 1] * d2).sum()), u

    def image_loss(i, z, y):                                    # image i's share of the loss
        bz, by, _, wsse, _ = image_terms(i, z, y)
        return ((bz + by) / (H * W) + lam * wsse / (H * W * 3)) / n

    r = model._sga.loss_and_grads(t(x, dev), t(z0, dev), t(y0, dev), tau, lam, noise_z=t(gz, dev), noise_y=t(gy, dev),
                                  grid=q["grid"], weight=q["weight"])
    bits_z, bits_y, sse, wsse = (r[k].cpu().numpy() for k in ("bits_z", "bits_y", "sse", "wsse"))
    g_z, g_y = r["g_z"].cpu().numpy(), r["g_y"].cpu().numpy()
    hstep = 1e-4
    for i in range(n):
        bz, by, sse64, wsse64, u = image_terms(i, z0[i:i + 1], y0[i:i + 1])
        print(f"\nimage {i} K={sorted(set(K[i].ravel().tolist()))}: bits_z {bits_z[i]:.3f} / {bz:.3f}  bits_y {bits_y[i]:.3f} / {by:.3f}  "
              f"sse {sse[i]:.3f} / {sse64:.3f}  wsse {wsse[i]:.3f} / {wsse64:.3f}")
        for got, want in ((bits_z[i], bz), (bits_y[i], by)):
            assert abs(got - want) / (H * W) < 2e-5 * max(1.0, want / (H * W))
        assert abs(sse[i] - sse64) < 2e-5 * sse64 and abs(wsse[i] - wsse64) < 2e-5 * wsse64
        for which, arr, grad, frac in ((0, z0[i], g_z[i], z0[i]), (1, y0[i], g_y[i], u[0])):
            checked = 0
            for fi in rng.permutation(arr.size):
                idx = np.unravel_index(fi, arr.shape)
                if abs(frac[idx] - np.rint(frac[idx])) < 5e-3:   # away from the kinks at integers
                    continue
                ap, am = arr[None].copy(), arr[None].copy()
                ap[(0,) + idx] += hstep
                am[(0,) + idx] -= hstep
                if which == 0:
                    fd = (image_loss(i, ap, y0[i:i + 1]) - image_loss(i, am, y0[i:i + 1])) / (2 * hstep)
                else:
                    fd = (image_loss(i, z0[i:i + 1], ap) - image_loss(i, z0[i:i + 1], am)) / (2 * hstep)
                assert abs(grad[idx] - fd) <= 2e-3 * abs(fd) + 2e-6, (i, which, idx, grad[idx], fd)
                checked += 1
                if checked == 6:
                    break
            assert checked == 6
    # the step's metrics: rd_loss = bpp + lambda mean_i(Dw_i); everything else unweighted, as before
    m = model.itinf_train_step(x, noise=(t(gz, dev), t(gy, dev))).scalars_float
    mses = sse / (H * W * 3)
    bpp = (bits_z.mean() + bits_y.mean()) / (H * W)
    assert abs(m["rd_loss"] - (bpp + lam * (wsse / (H * W * 3)).mean())) < 1e-5 * m["rd_loss"]
    assert abs(m["bpp"] - bpp) < 1e-6 * bpp and abs(m["mse"] - mses.mean()) < 1e-6 * mses.mean() and m["sched_rd_lambda"] == lam
    # a constant map and all zeros take the per-image route and the route of before
    model.initialize_itinf(x, step=[-9, 4], step_offsets=np.full((2, 4, 4), 3, np.int8))
    assert model._itinf_grid["grid"].kind == "image" and model._itinf_grid["grid"].steps == [-6, 7]
    model.initialize_itinf(x, step_offsets=np.zeros((2, 4, 4), np.int8))
    assert model._itinf_grid is None


# ---- 6. compress end to end ----------------------------------------------------------------------------------------------------
H128 = W128 = 128


def varying_offsets():
    off = np.zeros((2, 8, 8), np.int8)
    off[:, -1, :] = 1
    off[:, :, -1] = 1
    assert int((off != 0).sum()) == 2 * 15
    return off


@pytest.fixture(scope="module")
def x128(dev):
    return images(2, H128, W128, dev)


def check_weighted_report(model, x, blob, rep, ks, off):
    """What every refined file on a varying map has to satisfy: v7, decodes to the chosen candidate's pixels, payload within the
    coder's slack of the reported bits, never worse by the weighted J."""
    from shallow_ntc_amd import ops
    codec = model._get_codec()
    assert blob[4] == 7
    px = model.decompress(blob)
    z, y = (rv.loc for rv in model.last_compress_latents.uq)
    assert torch.equal(px, codec.latents_cost(z, y, x, step=ks, step_offsets=off)[2])
    blocks = blocks_of(ops.block_sse(x, px, 16))
    start = model.coded_cost(x, step=ks, step_offsets=off, weighted=True)
    bits, hd = payload_bits(model, blob)
    for i, r in enumerate(rep):
        assert r["weighted"] is True and r["quant_step"] == ks[i] and "lam" not in r
        np.testing.assert_array_equal(r["sse_blocks"], blocks[i])
        assert r["J_start"] == start["J"][i] and r["bits_start"] == start["bits"][i]
        assert abs(bits[i] - (r["bits_chosen"] + flushed_bits(model, hd))) <= slack_bar(model, hd)
        assert r["J_chosen"] <= r["J_start"]
        assert (r["step_chosen"] == 0) == (r["J_chosen"] == r["J_start"])


def test_constant_maps_are_the_routes_of_before(dev, hyper_model, x128):
    model = hyper_model
    assert model.compress(x128, itinf=dict(ITINF, step_offsets=np.zeros((2, 8, 8), np.int8))) == model.compress(x128, itinf=dict(ITINF))
    assert "weighted" not in model.last_compress_report[0]
    got = model.compress(x128, itinf=dict(ITINF, step=-9, step_offsets=np.full((2, 8, 8), 3, np.int8)))
    rep = model.last_compress_report
    assert got == model.compress(x128, itinf=dict(ITINF, step=-6))
    assert [{k: v for k, v in r.items()} for r in rep] == model.last_compress_report
    off = varying_offsets()
    assert model.compress(x128, itinf=dict(steps=0, step=-6, step_offsets=off)) == model.compress(x128, step=-6, step_offsets=off)
    assert [r["step_chosen"] for r in model.last_compress_report] == [0, 0]


def test_compress_with_itinf_on_a_map(dev, hyper_model, x128):
    from shallow_ntc_amd import entropy_coding as ec
    model = hyper_model
    off, ks = varying_offsets(), [-6, -6]
    blob = model.compress(x128, itinf=dict(ITINF, step=-6, step_offsets=off))
    rep = model.last_compress_report
    print()
    for i, r in enumerate(rep):
        print(f"map image {i}: step {r['step_chosen']}  J {r['J_start']:.6f} -> {r['J_chosen']:.6f}  bits {r['bits_start']:.1f} -> {r['bits_chosen']:.1f}")
    check_weighted_report(model, x128, blob, rep, ks, off)
    assert (model._get_codec()._parse(blob)["kmap"].reshape(2, 8, 8) == ec.index_map(ks, off)).all()
    # the uniform k = -6 run improves both fixture images in 8 steps; this map differs from it in 15 of 64
    # positions by one ladder place
    for r in rep:
        assert r["step_chosen"] in (4, 8) and r["J_chosen"] < r["J_start"]
    # the weighted J is the one of coded_cost on the chosen latents, and D_w is its own arithmetic
    after = model.coded_cost(x128, model.last_compress_latents, step=ks, step_offsets=off, weighted=True)
    assert after["J"].tolist() == [r["J_chosen"] for r in rep] and after["bits"].tolist() == [r["bits_chosen"] for r in rep]
    omega = ec.position_weights(ec.index_map(ks, off))
    np.testing.assert_allclose(after["D_w"], (omega * after["sse_blocks"]).sum(axis=(1, 2)) / (H128 * W128 * 3), rtol=1e-14)
    np.testing.assert_allclose(after["J"], after["bits"] / (H128 * W128) + 0.02 * after["D_w"], rtol=1e-15)
    assert after["sse_blocks"].sum(axis=(1, 2)).tolist() == after["sse"].tolist()
    plain = model.coded_cost(x128, model.last_compress_latents, step=ks, step_offsets=off)
    assert set(after) - set(plain) == {"sse_blocks", "D_w"} and plain["bits"].tolist() == after["bits"].tolist()


def test_target_bpp_on_a_map(dev, hyper_model, x128):
    from shallow_ntc_amd import entropy_coding as ec
    model, codec = hyper_model, hyper_model._get_codec()
    off = varying_offsets()
    # per-image targets between the predictions of bases 0 and -1 over this map, as test_hip_sga_step's budgets builds them
    lat = model.infer_latent_rvs(x128)
    ladder = list(range(ec.STEP_MIN, ec.STEP_MAX + 1))
    cost_z, cost_y = codec.ladder_cost(lat.uq[0].loc.contiguous(), lat.uq[1].loc.contiguous(), (H128, W128), ladder, step_offsets=off)
    fl = codec.flushed_bits(H128, W128)
    map_bits = ec.MAP_RECORD_BITS * ec.count_runs(off)
    pred = (cost_z.cpu().numpy()[:, None] + cost_y.cpu().numpy()) / 65536.0 + fl + map_bits[:, None]
    targets = [0.5 * (pred[i, ladder.index(0)] + pred[i, ladder.index(-1)]) / (H128 * W128) for i in range(2)]
    model.compress(x128, target_bpp=targets, step_offsets=off)
    plain = model.last_compress_report
    blob = model.compress(x128, itinf=dict(ITINF, target_bpp=targets, step_offsets=off))
    rep = model.last_compress_report
    ks = [r["quant_step"] for r in rep]
    pay, hd = payload_bits(model, blob)
    print()
    for i, r in enumerate(rep):
        print(f"map image {i}: base {r['quant_step']}, SGA step {r['step_chosen']}, bits {r['bits_start']:.1f} -> {r['bits_chosen']:.1f} + {fl} flushed "
              f"+ {r['map_bits']:.0f} map, budget {r['budget_bits']:.1f}, payload {pay[i]:.0f}")
        assert r["quant_step"] == plain[i]["step_chosen"] and r["met"] is True and plain[i]["met"] is True
        assert r["budget_bits"] == plain[i]["budget_bits"] == targets[i] * H128 * W128 and r["map_bits"] == plain[i]["map_bits"] == map_bits[i]
        assert r["bits_start"] + fl + r["map_bits"] == plain[i]["bits_predicted"]
        assert r["bits_chosen"] + fl <= r["budget_bits"] and r["bits_chosen"] + fl + r["map_bits"] <= r["budget_bits"]
        assert pay[i] <= r["budget_bits"] + slack_bar(model, hd)
    check_weighted_report(model, x128, blob, rep, ks, off)


def test_half_image_roi(dev, hyper_model, x128):
    from shallow_ntc_amd import entropy_coding as ec
    model = hyper_model
    mask = np.zeros((2, H128, W128), bool)
    mask[:, :, :W128 // 2] = True
    off = ec.roi_offsets(mask, 16, inside=0, outside=12, latent_hw=model.step_offsets_shape(H128, W128))
    assert set(np.unique(off).tolist()) == {0, 12}
    blob = model.compress(x128, itinf=dict(ITINF, step_offsets=off))
    rep = model.last_compress_report
    check_weighted_report(model, x128, blob, rep, [0, 0], off)
    # the ROI metric of coded_cost's docstring: the PSNR inside the mask from sse_blocks (whole 16 x 16 blocks here)
    px = model.decompress(blob).cpu().numpy().astype(np.float64)
    ref = O.floats_to_pixels(x128.cpu().numpy(), False).astype(np.float64)
    inside = off[0] == 0
    for i, r in enumerate(rep):
        mse = r["sse_blocks"][inside].sum() / (3.0 * 256 * inside.sum())
        want = ((px[i] - ref[i]) ** 2)[np.repeat(np.repeat(inside, 16, 0), 16, 1)].mean()
        assert mse == want
        print(f"roi image {i}: PSNR inside {10 * np.log10(255.0 ** 2 / mse):.2f} dB, J {r['J_start']:.6f} -> {r['J_chosen']:.6f}")


def test_map_refusals_on_the_device(dev, hyper_model, x128, monkeypatch):
    model = hyper_model
    launches = []
    analysis = model.infer_latent_rvs
    monkeypatch.setattr(model, "infer_latent_rvs", lambda *a, _f=analysis, **k: launches.append(1) or _f(*a, **k))
    for bad in (np.zeros((2, 8, 7), np.int8), np.zeros((1, 8, 8), np.int8), np.zeros((2, 8, 8), np.float32), np.full((2, 8, 8), 65)):
        with pytest.raises(ValueError, match="step_offsets"):
            model.compress(x128, itinf=dict(ITINF, step_offsets=bad))
        with pytest.raises(ValueError, match="step_offsets"):
            model.initialize_itinf(x128, step_offsets=bad)
    off = varying_offsets()
    with pytest.raises(ValueError, match="rd_lambda"):
        model.compress(x128, itinf=dict(ITINF, rd_lambda=0.1, step_offsets=off))
    with pytest.raises(ValueError, match="exclude"):
        model.compress(x128, itinf=dict(ITINF, step=1, target_bpp=0.3, step_offsets=off))
    with pytest.raises(ValueError, match="itinf"):
        model.compress(x128, itinf=dict(ITINF), step_offsets=off)
    for kw in (dict(), dict(lam=[0.1, 0.1], step=1)):
        with pytest.raises(ValueError):
            model.coded_cost(x128, weighted=True, **kw)
    assert not launches
