"""SGA iterative inference at a quantisation step (-m gpu): the step-aware sample / rate kernels against
the kernels of step 1 (bit for bit at ladder index 0) and against a float64 restatement of the step loss, the whole model's
loss and gradients at a step, and ``compress(x, itinf=dict(step=... | target_bpp=...))`` end to end."""
import math

import numpy as np
import pytest
import torch

from oracle import model_np
from oracle import ops_np as O
from test_hip_itinf_bitstream import (ITINF, flushed_bits, hyper_model, image_words, images, payload_bits,  # noqa: F401
                                      slack_bar)
from test_hip_sga import gumbel, make_model, t

pytestmark = pytest.mark.gpu

LN2 = math.log(2.0)
TAU = 0.4
SKIP_CAP = 0.05


def step_values(ks):
    """(step, inv_step) of the ladder indexes as the kernels read them: float32-rounded, held as float64 numbers."""
    from shallow_ntc_amd import entropy_coding as ec
    return np.array([ec.step_size(k) for k in ks]), np.array([ec.step_size(-k) for k in ks])


def quant_of(ks, dev, dweight=None):
    from shallow_ntc_amd import entropy_coding as ec
    st, inv, sh = ec.step_tensors(ks, dev)
    dw = torch.tensor([1.0] * len(ks) if dweight is None else list(dweight), dtype=torch.float32, device=dev)
    return st, inv, sh, dw


def per_image(a):
    return np.asarray(a, np.float64)[:, None, None, None]


# ---- the float64 restatement of the step loss's element-wise half, from the oracle's public pieces ------------------------
def scale_at(raw, k):
    """-> (sigma, e, j): sigma = SCALE_FN(clamp(clamp(exp(raw), 0, 63) - k, 0, 63))."""
    e = np.exp(raw)
    j = np.clip(e, 0.0, 63.0) - k
    return O.scale_fn(np.clip(j, 0.0, 63.0)), e, j


def bits_of(v, sigma):
    return O.noisy_normal_logprob(v, sigma) / -LN2


def restate(y, mu, raw, g, tau, ks):
    """Forward outputs of sntc_sga_normal_step_fwd in float64, and the mask of elements the comparison skips."""
    step, inv = (per_image(a) for a in step_values(ks))
    k = per_image(ks)
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


def plant_integers(y, mu, ks, rng, share=0.005):
    """Move a few y (and, where that fails, their mu to 0) so that the KERNEL's float32 u = (y - mu) * inv_step is an exact
    integer: try the float32 neighbours of mu + s step.  Returns how many were placed."""
    step, inv = step_values(ks)
    placed = 0
    n = y.shape[0]
    per = y[0].size
    for i in range(n):
        inv32 = np.float32(inv[i])
        for fi in rng.choice(per, size=min(40, max(2, int(share * per))), replace=False):
            idx = (i,) + np.unravel_index(fi, y.shape[1:])
            s = np.float32(rng.choice([-7, -3, -1, 0, 1, 2, 3, 5, 6, 11]))
            for m in (mu[idx], np.float32(0.0)):                 # a fine step leaves no neighbour of a mu of size 1 that hits: mu = 0 then
                lo = hi = np.float32(np.float64(m) + np.float64(s) * step[i])
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


def draw(rng, n, h, w, c, ks):
    mu = rng.standard_normal((n, h, w, c)).astype(np.float32)
    raw = rng.uniform(-2.5, 4.5, size=mu.shape).astype(np.float32)
    y = (mu + per_image(step_values(ks)[0]) * rng.laplace(0, 2, size=mu.shape)).astype(np.float32)
    return y, mu, raw, gumbel(rng, mu.shape)


def make_inputs(n, h, w, c, ks, plant=True):
    """mu normal, raw uniform in [-2.5, 4.5] (exp(raw) crosses 63; the shifted index leaves [0, 63] at both ends for the large
    shifts), y = mu + step Laplace(0, 2) (|u| <= 60), Gumbel pairs.  The seed is the first whose float64 restatement skips at most
    SKIP_CAP of the elements (a 12-element case has no room for one near-integer u)."""
    for seed in range(64):
        rng = np.random.default_rng([seed, n, h, w, c] + [k + 64 for k in ks])
        y, mu, raw, g = draw(rng, n, h, w, c, ks)
        planted = plant_integers(y, mu, ks, rng) if plant and mu[0].size >= 400 else 0
        ref = restate(y, mu, raw, g, TAU, ks)
        if ref["skip"].mean() <= SKIP_CAP and np.abs(ref["u"]).max() <= 60.0:
            return dict(y=y, mu=mu, raw=raw, g=g, hyper=np.concatenate([mu, raw], -1), ref=ref, planted=planted, seed=seed)
    raise AssertionError("no seed keeps the restatement's skipped share under the cap")


# ---- 1. ladder index 0 is the kernel pair of step 1 ---------------------------------------------------------------------
@pytest.mark.parametrize("h,w,c", [(3, 5, 8), (7, 37, 5)], ids=["c8-vector", "c5-scalar"])
def test_index_zero_is_todays_kernels(h, w, c, dev):
    from shallow_ntc_amd import ops
    n = 3
    ks = [0, 0, 0]
    y, mu, raw, g = draw(np.random.default_rng(h * w), n, h, w, c, ks)
    y[:, 0, 0, :3] = mu[:, 0, 0, :3] = 0.0                      # exact integers u (floor == ceil), a tie, and plain values
    y[:, 0, 0, :3] += np.array([3.0, -7.0, 0.5], np.float32)
    yd, hd, gd = t(y, dev), t(np.concatenate([mu, raw], -1), dev), t(g, dev)
    quant = quant_of(ks, dev)
    for noise, seed, step in ((gd, 0, 0), (None, 7, 3)):         # supplied noise; the generator with the same (seed, step)
        old = ops.sga_normal_fwd(yd, hd, TAU, noise, seed, step)
        new = ops.sga_normal_step_fwd(yd, hd, TAU, quant, noise, seed, step)
        for name, a, b in zip(("y_tilde", "sprime", "dbits_dv", "dbits_draw"), old, new):
            assert torch.equal(a, b), (name, "noise" if noise is not None else "generator")
        np.testing.assert_allclose(new[4].cpu().numpy(), old[4].cpu().numpy(), rtol=1e-12)       # the summation order may differ
    assert old[0][0, 0, 0, 0].item() == 3.0 and old[0][0, 0, 0, 1].item() == -7.0                # the sample at an integer is it
    rng = np.random.default_rng(c)
    g_yt = t(rng.standard_normal(y.shape), dev)
    got = ops.sga_normal_step_bwd(g_yt, new[1], new[2], new[3], 1.0 / (n * 64 * 64), quant)
    want = ops.sga_normal_bwd(g_yt, old[1], old[2], old[3], 1.0 / (n * 64 * 64))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    a = ops.sga_normal_step_fwd(yd, hd, TAU, quant, None, 7, 4)[0]
    assert not torch.equal(a, new[0])                            # another step of the generator is another draw


# ---- 2. the kernels against float64 ----------------------------------------------------------------------------------
# units per image (a unit = 4 channels of a pixel where c % 4 == 0): 1; 255 / 256 / 257 around one workgroup's 256 threads; 1334 =
# six workgroups, the last one partly idle; c = 5: the element-wise path, 1295 units; 131 200 units = more than the 512 workgroups of
# one pass: every workgroup loops (that case with one ladder only: its float64 restatement takes seconds)
SHAPES = [(1, 1, 4), (15, 17, 4), (8, 16, 8), (1, 257, 4), (23, 29, 8), (7, 37, 5)]
LADDERS = [(-32, 0, 32), (-5, 3, 17)]
CASES = [(h, w, c, ks) for ks in LADDERS for h, w, c in SHAPES] + [(1, 131200, 4, LADDERS[0])]
DWEIGHT = (0.25, 1.0, 7.5)


def close(got, want, ok, rtol, atol, label):
    err = np.abs(got - want)
    bad = ok & ~(err <= rtol * np.abs(want) + atol)
    assert not bad.any(), (label, int(bad.sum()), float(err[bad].max()), got[bad][:4], want[bad][:4])


@pytest.mark.parametrize("h,w,c,ks", CASES, ids=[f"{h}x{w}x{c}-{'ends' if ks == LADDERS[0] else 'inner'}" for h, w, c, ks in CASES])
def test_step_kernels_against_float64(h, w, c, ks, dev):
    from shallow_ntc_amd import entropy_coding as ec
    from shallow_ntc_amd import ops
    n = 3
    case = make_inputs(n, h, w, c, list(ks))
    ref = case["ref"]
    ok = ~ref["skip"]
    share = float(ref["skip"].mean())
    print(f"\n{h}x{w}x{c} k={ks}: seed {case['seed']}, skipped {share:.4f}, planted integer u {case['planted']}, max |u| {np.abs(ref['u']).max():.1f}")
    assert share <= SKIP_CAP
    yd, hd, gd = t(case["y"], dev), t(case["hyper"], dev), t(case["g"], dev)
    quant = quant_of(ks, dev, DWEIGHT)
    yt, sp, dv, dr, bits = (a.cpu().numpy() for a in ops.sga_normal_step_fwd(yd, hd, TAU, quant, gd))
    step, inv = (per_image(a) for a in step_values(ks))
    mu64 = case["mu"].astype(np.float64)
    close((yt.astype(np.float64) - mu64) / step, ref["v"], ok, 0.0, 3e-5, "sample v")
    np.testing.assert_allclose(bits, ref["bits"].sum(axis=(1, 2, 3)), rtol=2e-5)
    for got, name in ((sp, "sp"), (dv, "dv"), (dr, "dr")):
        close(got.astype(np.float64), ref[name], ok, 3e-3, 1e-3, name)
    # the plain clamp gradient of the outer clamp: exactly zero off the ladder's ends
    off = (ref["j"] < -1e-3) | (ref["j"] > 63.0 + 1e-3)
    assert (dr[off] == 0.0).all()
    if ks == LADDERS[0]:
        assert off[0].any() and off[2].any() and (dr[~off] != 0.0).any()        # both ends are reached, and the middle is live
    # where the kernel's own u is an integer, y~ is the coder's value of the coder's symbol
    u32 = (case["y"] - case["mu"]) * inv.astype(np.float32)
    assert u32.dtype == np.float32
    exact = u32 == np.rint(u32)
    if c % 4 == 0 and case["planted"]:
        assert all(exact[i].sum() >= 2 for i in range(n))
        sym, _ = ops.step_symbols(yd, hd, ec.scale_table_ids(hd), quant[1], quant[2])
        coder = ops.dequant_step(sym, hd, quant[0]).cpu().numpy()
        np.testing.assert_array_equal(sym.cpu().numpy()[exact], u32[exact].astype(np.int32))
        np.testing.assert_array_equal(yt[exact].view(np.uint32), coder[exact].view(np.uint32))
    # backward: the three formulas in float64 on the forward outputs
    rng = np.random.default_rng(h * w)
    g_yt = rng.standard_normal(yt.shape).astype(np.float32)
    wgt = 0.37
    g_y, g_h = (a.cpu().numpy().astype(np.float64) for a in ops.sga_normal_step_bwd(t(g_yt, dev), t(sp, dev), t(dv, dev), t(dr, dev), wgt, quant))
    a = sp.astype(np.float64) * inv
    dvw = np.float64(np.float32(wgt)) * dv
    g = g_yt * per_image(np.float32(DWEIGHT))
    every = np.ones(yt.shape, bool)
    close(g_y, (g * step + dvw) * a, every, 3e-3, 1e-3, "g_yloc")
    close(g_h[..., :c], g * (1.0 - step * a) - dvw * a, every, 3e-3, 1e-3, "g_mu")
    close(g_h[..., c:], np.float64(np.float32(wgt)) * dr, every, 3e-3, 1e-3, "g_raw")


def test_op_input_checks(dev):
    from shallow_ntc_amd import ops
    y = torch.zeros((2, 3, 4, 8), device=dev)
    hyper = torch.zeros((2, 3, 4, 16), device=dev)
    quant = quant_of([1, -1], dev)
    ops.sga_normal_step_fwd(y, hyper, TAU, quant)
    for bad in (quant[:2], quant_of([1], dev), (quant[0], quant[1], quant[2].float(), quant[3]), tuple(q.cpu() for q in quant), None):
        with pytest.raises(ValueError):
            ops.sga_normal_step_fwd(y, hyper, TAU, bad)
    with pytest.raises(ValueError):
        ops.sga_normal_step_fwd(y, hyper[..., :8].contiguous(), TAU, quant)
    with pytest.raises(ValueError):
        ops.sga_normal_step_fwd(y, hyper, TAU, quant, noise=torch.zeros((2, 3, 4, 8), device=dev))
    with pytest.raises(ValueError):
        ops.sga_normal_step_bwd(y, y, y, y, 1.0, quant[:3])
    with pytest.raises(ValueError):
        ops.sga_normal_step_bwd(y, y[:1], y, y, 1.0, quant)


# ---- 3. the whole model at a step: test_sga_loss_and_gradients with quant -------------------------------------------------
def test_sga_loss_and_gradients_at_a_step(dev):
    """GPU loss terms == the restated float64 loss mean_B(bits_i) / (H W) + (1 / n) sum_i lambda_i MSE_i at ladder indexes
    (-5, +7) with the default lambda_i and the same Gumbel noise; GPU gradients == central differences of it."""
    from shallow_ntc_amd import entropy_coding as ec
    from shallow_ntc_amd.common import data_lib
    from shallow_ntc_amd.mshyper.models import step_lambdas
    model, w, tc = make_model(dev)
    lam, ks, tau = 0.02, [-5, 7], 0.5
    ref_model = model_np.Model(tc, rd_lambda=lam)
    ms, bs, fs = model_np._prior_lists(w)
    x = data_lib.normalize_image(data_lib.synthetic_images(2, 60, 64, seed=9))        # pads to 64 x 64
    n, H, W, _ = x.shape
    model.initialize_itinf(x, step=ks)
    lams = step_lambdas(lam, ks)
    assert model._itinf_grid["grid"].kind == "image" and model._itinf_grid["grid"].steps == ks
    assert model._itinf_grid["lam"].tolist() == lams.tolist() == [lam / ec.step_size(k) ** 2 for k in ks]
    z0 = model.latent_rvs.uq[0].loc.cpu().numpy().astype(np.float64)
    y0 = model.latent_rvs.uq[1].loc.cpu().numpy().astype(np.float64)
    rng = np.random.default_rng(3)
    gz, gy = gumbel(rng, z0.shape), gumbel(rng, y0.shape)
    step, inv = step_values(ks)

    def image_terms(i, z, y):
        """(bits_z, bits_y, mse) of image i for latents z, y of that image alone ([1, ...])."""
        z_t = O.sga_round(z, tau, gz[i:i + 1].astype(np.float64), offset=0.0)
        bits_z = O.deep_factorized_logprob(z_t, ms, bs, fs).sum() / -LN2
        hyp = ref_model._run(ref_model.hyper_synthesis, w, "hyper_synthesis/", z_t, None)
        c = hyp.shape[-1] // 2
        mu, raw = hyp[..., :c], hyp[..., c:]
        v = O.sga_round((y - mu) * inv[i], tau, gy[i:i + 1].astype(np.float64))
        bits_y = bits_of(v, scale_at(raw, ks[i])[0]).sum()
        recon = O.unpad_images(ref_model._run(ref_model.synthesis, w, "synthesis/", step[i] * v + mu, None), x[i:i + 1].shape)
        mses, _ = O.mse_psnr(O.floats_to_pixels(x[i:i + 1].astype(np.float64), True), O.floats_to_pixels(recon, True))
        return bits_z, bits_y, float(mses[0]), (y - mu) * inv[i]

    def image_loss(i, z, y):                                    # image i's share of the loss
        bz, by, mse, _ = image_terms(i, z, y)
        return ((bz + by) / (H * W) + lams[i] * mse) / n

    r = model._sga.loss_and_grads(t(x, dev), t(z0, dev), t(y0, dev), tau, lam, noise_z=t(gz, dev), noise_y=t(gy, dev),
                                  grid=model._itinf_grid["grid"], weight=model._itinf_grid["weight"])
    bits_z, bits_y, sse = (r[k].cpu().numpy() for k in ("bits_z", "bits_y", "sse"))
    g_z, g_y = r["g_z"].cpu().numpy(), r["g_y"].cpu().numpy()
    hstep = 1e-4
    for i in range(n):
        bz, by, mse, u = image_terms(i, z0[i:i + 1], y0[i:i + 1])
        print(f"\nimage {i} k={ks[i]} lambda={lams[i]:.5f}: bits_z {bits_z[i]:.3f} / {bz:.3f}  bits_y {bits_y[i]:.3f} / {by:.3f}  "
              f"mse {sse[i] / (H * W * 3):.5f} / {mse:.5f}")
        for got, want in ((bits_z[i], bz), (bits_y[i], by)):
            assert abs(got - want) / (H * W) < 2e-5 * max(1.0, want / (H * W))
        assert abs(sse[i] / (H * W * 3) - mse) < 2e-5 * mse
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
    # the step's metrics: rd_loss = bpp + mean_i(lambda_i D_i); everything else as at step 1
    m = model.itinf_train_step(x, noise=(t(gz, dev), t(gy, dev))).scalars_float
    mses = sse / (H * W * 3)
    bpp = (bits_z.mean() + bits_y.mean()) / (H * W)
    assert abs(m["rd_loss"] - (bpp + (lams * mses).mean())) < 1e-5 * m["rd_loss"]
    assert abs(m["bpp"] - bpp) < 1e-6 * bpp and abs(m["mse"] - mses.mean()) < 1e-6 * mses.mean() and m["sched_rd_lambda"] == lam


# ---- 4. compress end to end ----------------------------------------------------------------------------------------------
STEP_RUNS = {"fine": -6, "coarse": 6, "mixed": (-6, 6)}


@pytest.fixture(scope="module")
def runs(dev, hyper_model):
    """compress(x, itinf=dict(ITINF, step=...)) once per case: (blob, report, chosen latents)."""
    x = images(2, 128, 128, dev)
    out = {}
    for name, step in STEP_RUNS.items():
        blob = hyper_model.compress(x, itinf=dict(ITINF, step=step))
        out[name] = (blob, hyper_model.last_compress_report, [rv.loc.clone() for rv in hyper_model.last_compress_latents.uq])
    return x, out


@pytest.mark.parametrize("name", list(STEP_RUNS))
def test_compress_with_itinf_at_a_step(name, dev, hyper_model, runs):
    from shallow_ntc_amd import entropy_coding as ec
    model, codec = hyper_model, hyper_model._get_codec()
    n, h, w = 2, 128, 128
    x, out = runs
    blob, rep, (z, y) = out[name]
    ks = ec.check_steps(STEP_RUNS[name], n)
    lams = [0.02 / ec.step_size(k) ** 2 for k in ks]
    assert blob[4] == 5 and codec._parse(blob)["steps"] == ks   # the header carries the indexes
    start = model.coded_cost(x, step=ks)
    plain = model.compress(x, step=ks)
    print()
    for i, r in enumerate(rep):
        print(f"k={ks[i]} image {i}: step {r['step_chosen']}  J {r['J_start']:.6f} -> {r['J_chosen']:.6f}  "
              f"bits {r['bits_start']:.1f} -> {r['bits_chosen']:.1f}  lambda {r['lam']:.5f}")
        assert r["quant_step"] == ks[i] and r["lam"] == lams[i] and r["step_chosen"] in (0, 4, 8)
        assert r["J_start"] == start["bits"][i] / (h * w) + lams[i] * start["D"][i] and r["bits_start"] == start["bits"][i]
        assert r["J_chosen"] <= r["J_start"]
        assert (r["step_chosen"] == 0) == (r["J_chosen"] == r["J_start"])
    from shallow_ntc_amd.common.latent_rvs_lib import LatentRVCollection, UQLatentRV
    after = model.coded_cost(x, LatentRVCollection(uq=(UQLatentRV(z), UQLatentRV(y))), step=ks, lam=lams)
    assert after["J"].tolist() == [r["J_chosen"] for r in rep] and after["bits"].tolist() == [r["bits_chosen"] for r in rep]
    assert torch.equal(model.decompress(blob), codec.latents_cost(z, y, x, step=ks)[2])
    bits, hd = payload_bits(model, blob)
    for i in range(n):
        assert abs(bits[i] - (rep[i]["bits_chosen"] + flushed_bits(model, hd))) <= slack_bar(model, hd)
        if rep[i]["step_chosen"] == 0:                          # the encoder's own latents were kept: the streams of compress(x, step=ks)
            assert image_words(model, blob, i) == image_words(model, plain, i)
        alone = codec.compress_latents(z[i:i + 1].contiguous(), y[i:i + 1].contiguous(), (h, w), step=[ks[i]])
        assert image_words(model, alone, 0) == image_words(model, blob, i)


def test_identities_and_improvement(dev, hyper_model, runs):
    model = hyper_model
    x, out = runs
    assert model.compress(x, itinf=dict(ITINF, step=0)) == model.compress(x, itinf=ITINF)
    assert model.compress(x, itinf=dict(steps=0, step=6)) == model.compress(x, step=6)
    assert [r["step_chosen"] for r in model.last_compress_report] == [0, 0]
    # at ladder index 0 this fixture improves both images within 8 steps; off it, at least one
    chosen = [r["step_chosen"] for name in ("fine", "coarse") for r in out[name][1]]
    assert any(s > 0 for s in chosen), chosen


# ---- 5. target_bpp inside itinf -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def budgets(dev, hyper_model):
    """Per-image targets between bits(k*) and bits(k* - 1) of the encoder's latents, k* = (-2, 3), as test_target_bpp builds them."""
    from shallow_ntc_amd import entropy_coding as ec
    model, codec = hyper_model, hyper_model._get_codec()
    n, h, w = 2, 128, 128
    x = images(n, h, w, dev)
    lat = model.infer_latent_rvs(x)
    ladder = list(range(ec.STEP_MIN, ec.STEP_MAX + 1))
    cost_z, cost_y = codec.ladder_cost(lat.uq[0].loc.contiguous(), lat.uq[1].loc.contiguous(), (h, w), ladder)
    bits = (cost_z.cpu().numpy()[:, None] + cost_y.cpu().numpy()) / 65536.0 + codec.flushed_bits(h, w)
    at = lambda i, k: float(bits[i, ladder.index(k)])
    targets = []
    for i, k in enumerate((-2, 3)):
        assert at(i, k) < at(i, k - 1)
        targets.append(0.5 * (at(i, k) + at(i, k - 1)) / (h * w))
    return x, targets, bits


def test_target_bpp_inside_itinf(dev, hyper_model, budgets):
    from shallow_ntc_amd import entropy_coding as ec
    model, codec = hyper_model, hyper_model._get_codec()
    n, h, w = 2, 128, 128
    x, targets, bits = budgets
    model.compress(x, target_bpp=targets)
    plain = model.last_compress_report
    assert [r["step_chosen"] for r in plain] == [-2, 3]
    blob = model.compress(x, itinf=dict(ITINF, target_bpp=targets))
    rep = model.last_compress_report
    pay, hd = payload_bits(model, blob)
    fl = codec.flushed_bits(h, w)
    print()
    for i, r in enumerate(rep):
        print(f"image {i}: quant step {r['quant_step']}, SGA step {r['step_chosen']}, bits {r['bits_start']:.1f} -> {r['bits_chosen']:.1f} "
              f"+ {fl} flushed, budget {r['budget_bits']:.1f}, payload {pay[i]:.0f}")
        assert r["quant_step"] == plain[i]["step_chosen"] and r["met"] is True and plain[i]["met"] is True
        assert r["budget_bits"] == plain[i]["budget_bits"] == targets[i] * h * w
        assert r["bits_start"] + fl == plain[i]["bits_predicted"]
        assert r["bits_chosen"] + fl <= r["budget_bits"]
        assert pay[i] <= r["budget_bits"] + slack_bar(model, hd)
        assert r["J_chosen"] <= r["J_start"]
    assert codec._parse(blob)["steps"] == [-2, 3]
    z, y = (rv.loc for rv in model.last_compress_latents.uq)
    assert torch.equal(model.decompress(blob), codec.latents_cost(z, y, x, step=[-2, 3])[2])
    # a budget nothing meets: the coarsest step, and the candidate with the fewest bits
    model.compress(x, itinf=dict(ITINF, target_bpp=0.5 * float(bits[:, -1].min()) / (h * w)))
    for r in model.last_compress_report:
        assert r["quant_step"] == ec.STEP_MAX and r["met"] is False and r["bits_chosen"] <= r["bits_start"]
        assert (r["step_chosen"] == 0) == (r["bits_chosen"] == r["bits_start"])


def test_over_budget_candidate_is_not_taken(dev, hyper_model, budgets, monkeypatch):
    """Scripted J and bits per candidate.  Image 0: step 4 has the smallest J but one bit too many, step 8 fits with a J below the
    start's -> 8.  Image 1: step 4 fits and is best, step 8 is better still but over budget -> 4."""
    model, codec = hyper_model, hyper_model._get_codec()
    n, h, w = 2, 128, 128
    x, targets, _ = budgets
    room = np.array(targets) * h * w - codec.flushed_bits(h, w)   # the most bits a candidate may have
    script = iter([([5.0, 5.0], room - 10.0),
                   ([1.0, 3.0], room + [1.0, -20.0]),
                   ([4.0, 1.0], room + [0.0, 0.5])])
    real_cost, snaps = model.coded_cost, {}

    def cost(xx, latent_rvs=None, **kw):
        c = real_cost(xx, latent_rvs, **kw)
        assert kw["step"] == [-2, 3] and len(kw["lam"]) == n
        j, b = next(script)
        c["J"], c["bits"] = np.array(j), np.array(b, np.float64)
        snaps[model.global_step] = [rv.loc.clone() for rv in latent_rvs.uq]
        return c

    monkeypatch.setattr(model, "coded_cost", cost)
    blob = model.compress(x, itinf=dict(ITINF, target_bpp=targets))
    monkeypatch.undo()
    rep = model.last_compress_report
    assert [r["step_chosen"] for r in rep] == [8, 4] and [r["J_chosen"] for r in rep] == [4.0, 3.0]
    assert [r["bits_chosen"] for r in rep] == [room[0], room[1] - 20.0]
    assert sorted(snaps) == [0, 4, 8]
    for i, step in enumerate((8, 4)):
        for kept, snap in zip(model.last_compress_latents.uq, snaps[step]):
            assert torch.equal(kept.loc[i], snap[i])
    z, y = (rv.loc for rv in model.last_compress_latents.uq)
    assert torch.equal(model.decompress(blob), codec.latents_cost(z, y, x, step=[-2, 3])[2])


def test_ms_ssim_at_a_step(dev):
    """distortion="ms_ssim" works unchanged: D = 1 - SSIM of the decoded pixels (64 x 96: single scale), J at lambda_i."""
    from shallow_ntc_amd import entropy_coding as ec
    from shallow_ntc_amd import ops
    from shallow_ntc_amd.mshyper import configs
    from shallow_ntc_amd.mshyper.models import Model
    model = Model(device=dev, distortion="ms_ssim", **{**configs.two_layer_syn(rd_lambda=8.0), **configs.itinf()})
    x = images(2, 64, 96, dev, seed=4)
    ks = [-4, 5]
    blob = model.compress(x, itinf=dict(ITINF, step=ks))
    rep = model.last_compress_report
    px = model.decompress(blob)
    q = ops.image_quality(ops.pixels_float(x, 64, 96), px.to(torch.float32), 255.0)
    for i, r in enumerate(rep):
        lam = 8.0 / ec.step_size(ks[i]) ** 2
        print(f"ms_ssim k={ks[i]} image {i}: step {r['step_chosen']}  J {r['J_start']:.6f} -> {r['J_chosen']:.6f}")
        assert r["lam"] == lam and r["J_chosen"] <= r["J_start"]
        np.testing.assert_allclose(r["J_chosen"], r["bits_chosen"] / (64 * 96) + lam * (1.0 - q[i]), rtol=1e-12)
