"""(MS-)SSIM as a differentiable distortion on the GPU (-m gpu; csrc/msssim_grad.hip): value and gradient against
float64 autograd of the restatement in tests/test_msssim_grad_host.py, the pool adjoint, the clamp rule, the SGA step of both
model families under ``distortion="ms_ssim"``, and the refusals."""
import numpy as np
import pytest
import torch

from oracle import ops_np as O
from oracle import train_ref
from test_msssim_grad_host import clamp_pair, distortion, quality, smooth_pair
from test_hip_sga import ITINF, TC, gumbel, t

pytestmark = pytest.mark.gpu


def to_model_range(a):
    """0-255 floats -> the model's [-0.5, 0.5] floats, and the float32 pixel values the kernels rebuild from them."""
    x = (a / np.float32(255) - np.float32(0.5)).astype(np.float32)
    return x, ((x + np.float32(0.5)) * np.float32(255)).astype(np.float32)


def reference(a, b, lam):
    """float64 autograd: -> (q[n], d(lam (1 - mean q)) / d x_hat = 255 d / d b)."""
    at = torch.from_numpy(a).double()
    bt = torch.from_numpy(b).double().requires_grad_(True)
    q = quality(at, bt)
    (g,) = torch.autograd.grad(lam * (1.0 - q.mean()), bt)
    return q.detach().numpy(), 255.0 * g.numpy()


def assert_gradient(got, want, label=""):
    err = np.abs(got - want)
    bar = 2e-4 * np.abs(want) + 2e-5 * np.abs(want).max()
    worst = float((err / bar).max())
    print(f"{label}: max err / bar = {worst:.3f}, max |want| = {np.abs(want).max():.3e}")
    assert np.abs(want).max() > 0 and (err <= bar).all(), (label, worst, float(err.max()), float(np.abs(want).max()))


@pytest.mark.parametrize("n,h,w,c,pad", [(2, 176, 200, 3, (0, 0)), (1, 161, 187, 3, (15, 5)), (2, 100, 120, 3, (0, 0)), (1, 512, 768, 3, (0, 0)),
                                         (1, 11, 40, 3, (5, 8)), (1, 176, 200, 1, (0, 0)), (2, 90, 75, 1, (6, 5)), (2, 176, 200, 3, (16, 24))])
def test_value_and_gradient_against_float64_autograd(n, h, w, c, pad, dev):
    from shallow_ntc_amd import ops
    lam = 50.0
    a, b = smooth_pair(n, h, w, c)
    x, a = to_model_range(a)
    xh, b = to_model_range(b)
    xh_pad = np.pad(xh, ((0, 0), (0, pad[0]), (0, pad[1]), (0, 0)), constant_values=0.25)
    g, sse, q = ops.msssim_distortion_grad(t(x, dev), t(xh_pad, dev), lam)
    assert g.shape == xh_pad.shape and q.dtype == torch.float64 and q.is_cuda and sse.is_cuda
    q_ref, g_ref = reference(a, b, lam)
    # value: the device finish == the host finish on the same tensors, and the float64 restatement at test_ms_ssim's bar
    np.testing.assert_allclose(q.cpu().numpy(), ops.image_quality(t(a, dev), t(b, dev)), rtol=1e-12)
    np.testing.assert_allclose(q.cpu().numpy(), q_ref, rtol=3e-5)
    np.testing.assert_allclose(q_ref, O.image_quality(a, b)[0], rtol=1e-12)
    g = g.cpu().numpy()
    assert np.isfinite(g).all()
    assert_gradient(g[:, :h, :w], g_ref, f"{n}x{h}x{w}x{c}")
    assert (g[:, h:] == 0).all() and (g[:, :, w:] == 0).all()                 # the padded margin: exactly zero
    _, sse_ref = ops.distortion_grad(t(x, dev), t(xh_pad, dev), 1.0)
    np.testing.assert_allclose(sse.cpu().numpy(), sse_ref.cpu().numpy(), rtol=1e-13)     # the same partial sums; double atomics


@pytest.mark.parametrize("h,w", [(9, 13), (9, 12), (8, 12), (1, 1), (33, 2)])
@pytest.mark.parametrize("c", [1, 3])
def test_pool_adjoint(h, w, c, dev):
    from shallow_ntc_amd import ops
    rng = np.random.default_rng(h * 100 + w)
    u = rng.standard_normal((2, h, w, c)).astype(np.float32)
    v = rng.standard_normal((2, (h + 1) // 2, (w + 1) // 2, c)).astype(np.float32)
    pu = ops._avgpool2(t(u, dev)).cpu().numpy().astype(np.float64)
    ptv = ops.avgpool2_symmetric_grad(t(v, dev), h, w).cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(pu, O._avg_pool2_symmetric(u.astype(np.float64)), rtol=0, atol=1e-6)
    lhs, rhs = (pu * v).sum(), (u * ptv).sum()
    assert abs(lhs - rhs) <= 1e-6 * (np.abs(pu * v).sum() + 1e-30), (lhs, rhs)


def test_batch_consistency(dev):
    from shallow_ntc_amd import ops
    a, b = smooth_pair(3, 176, 200)
    x, _ = to_model_range(a)
    xh, _ = to_model_range(b)
    g3, _, q3 = ops.msssim_distortion_grad(t(x, dev), t(xh, dev), 10.0)
    g1, _, q1 = ops.msssim_distortion_grad(t(x[1:2], dev), t(xh[1:2], dev), 10.0)
    np.testing.assert_allclose(q3.cpu().numpy()[1:2], q1.cpu().numpy(), rtol=1e-12)
    assert_gradient(3.0 * g3.cpu().numpy()[1:2], g1.cpu().numpy().astype(np.float64), "batch 3 vs 1")


def test_clamped_factor_gives_zeros(dev):
    from shallow_ntc_amd import ops
    a, b = clamp_pair()
    x, a = to_model_range(a)
    xh, b = to_model_range(b)
    g, _, q = ops.msssim_distortion_grad(t(x, dev), t(xh, dev), 20.0)
    q_ref, g_ref = reference(a, b, 20.0)
    g = g.cpu().numpy()
    assert np.isfinite(g).all() and np.isfinite(q.cpu().numpy()).all()
    assert (g[0, :, :, 1] == 0).all() and (g_ref[0, :, :, 1] == 0).all()
    np.testing.assert_allclose(q.cpu().numpy(), q_ref, rtol=3e-5)
    assert_gradient(g, g_ref, "clamp pair")


# ---- the SGA step ---------------------------------------------------------------------------------------------------
def sga_reference(transform_config, params, x, z_loc, y_loc, tau, gumbel_z, gumbel_y, lam, factorized=False, num_filters=(3, 3)):
    """oracle/train_ref.py::sga_loss_and_grads with the MSE term replaced by the restatement's D = 1 - mean_B q_i."""
    R = train_ref
    eff = {k: torch.tensor(np.asarray(v, np.float64)) for k, v in params.items()}
    y = torch.tensor(np.asarray(y_loc, np.float64), requires_grad=True)
    gy = torch.tensor(np.asarray(gumbel_y, np.float64))
    xt = R.as_input(x)
    n, _, h, w = xt.shape
    b = y.shape[-1]
    sy = dict(transform_config["synthesis"])
    synthesis = R.T.build(sy.pop("cls"), cin=b, **sy)
    nl = len(num_filters) + 1
    mats = [eff[f"prior/matrix_{k}"] for k in range(nl)]
    biases = [eff[f"prior/bias_{k}"] for k in range(nl)]
    factors = [eff[f"prior/factor_{k}"] for k in range(nl - 1)]
    if factorized:
        z = None
        y_t = R.sga_round(y, tau, gy)
        bits_y = R.noisy_deep_factorized_bits(y_t, mats, biases, factors).sum(dim=(1, 2, 3))
        bpp = bits_y.mean() / (h * w)
    else:
        z = torch.tensor(np.asarray(z_loc, np.float64), requires_grad=True)
        gz = torch.tensor(np.asarray(gumbel_z, np.float64))
        hs = dict(transform_config.get("hyper_synthesis", dict(cls="HyperSynthesis", bottleneck_size=b)))
        hyper_synthesis = R.T.build(hs.pop("cls"), cin=z.shape[-1], **hs)
        z_t = R.sga_round(z, tau, gz)
        bits_z = R.noisy_deep_factorized_bits(z_t, mats, biases, factors).sum(dim=(1, 2, 3))
        hyper = hyper_synthesis(R.T.sub_params(eff, "hyper_synthesis/"), z_t.permute(0, 3, 1, 2), be=R._SELF)
        mu, raw = hyper[:, :b].permute(0, 2, 3, 1), hyper[:, b:].permute(0, 2, 3, 1)
        y_t = R.sga_round(y, tau, gy, offset=mu)
        bits_y = R.noisy_normal_bits(y_t - mu, raw).sum(dim=(1, 2, 3))
        bpp = bits_z.mean() / (h * w) + bits_y.mean() / (h * w)
    recon = synthesis(R.T.sub_params(eff, "synthesis/"), y_t.permute(0, 3, 1, 2), be=R._SELF)[:, :, :h, :w]
    q = quality(((xt + 0.5) * 255.0).permute(0, 2, 3, 1), ((recon + 0.5) * 255.0).permute(0, 2, 3, 1))
    loss = bpp + lam * (1.0 - q.mean())
    grads = torch.autograd.grad(loss, [y] if factorized else [z, y])
    return dict(loss=float(loss.detach()), bpp=float(bpp.detach()), msssim=float(q.mean().detach()),
                g_z=None if factorized else grads[0].numpy(), g_y=grads[-1].numpy())


def spread_weights(model, hyper_half=None, seed=8):
    w = dict(model.get_weights())
    rng = np.random.default_rng(seed)
    for k in list(w):
        if k.endswith("/bias"):
            w[k] = (0.1 * rng.standard_normal(w[k].shape)).astype(np.float32)
        elif k.endswith("/beta"):
            w[k] = (1 + 0.5 * rng.random(w[k].shape)).astype(np.float32)
        elif k.startswith("prior/"):
            w[k] = (w[k] + 0.2 * rng.standard_normal(w[k].shape)).astype(np.float32)
    if hyper_half:
        b = w["hyper_synthesis/layer_2/bias"].copy()
        b[hyper_half:] = rng.uniform(-1, 2.5, size=hyper_half)
        w["hyper_synthesis/layer_2/bias"] = b.astype(np.float32)
    model.set_weights(w)
    return w


@pytest.mark.parametrize("case", ["hyperprior_small_msssim", "factorized_small_msssim", "hyperprior_full_width_ssim"])
def test_sga_loss_and_gradients_under_ms_ssim(case, dev):
    """tests/test_hip_sga.py::test_sga_gradients_at_full_width_against_float64_autograd with the MSE term replaced: every
    component of d loss / d z_loc and d loss / d y_loc, and rd_loss / bpp / msssim, against float64 autograd."""
    from shallow_ntc_amd.common import data_lib
    from shallow_ntc_amd.mshyper import configs
    rng = np.random.default_rng(8)
    tau, lam = 0.4, 40.0
    factorized = case.startswith("factorized")
    if case == "hyperprior_full_width_ssim":
        from shallow_ntc_amd.mshyper.models import Model
        cfg = configs.CONFIGS["two_layer_syn2"](rd_lambda=lam)
        cfg.update(configs.itinf())
        model = Model(device=dev, distortion="ms_ssim", **cfg)
        tc, c, (h, wd) = cfg["transform_config"], 320, (128, 128)           # both sides < 160: the single-scale branch
        w = spread_weights(model, 320)
    elif factorized:
        from shallow_ntc_amd.factorized.models import Model
        tc = dict(analysis=dict(cls="BLS2017Analysis", num_filters=32), synthesis=dict(cls="BLS2017Synthesis", num_filters=32))
        model = Model(device=dev, rd_lambda=lam, transform_config=tc, distortion="ms_ssim", **ITINF)
        c, (h, wd) = 32, (176, 192)
        w = spread_weights(model)
    else:
        from shallow_ntc_amd.mshyper.models import Model
        tc = dict(TC)
        model = Model(device=dev, rd_lambda=lam, transform_config=tc, distortion="ms_ssim", **ITINF)
        c, (h, wd) = 64, (180, 200)                                         # pads to 192 x 256: a padded x_hat
        w = spread_weights(model, 64)
    x = data_lib.normalize_image(data_lib.synthetic_images(1, h, wd, seed=3))
    model.initialize_itinf(x)
    shapes = [tuple(rv.loc.shape) for rv in model.latent_rvs.uq]
    assert shapes[-1][-1] == c
    y0 = (3.0 * rng.standard_normal(shapes[-1])).astype(np.float32)
    gy = gumbel(rng, y0.shape)
    z0 = gz = None
    if not factorized:
        z0 = (2.0 * rng.standard_normal(shapes[0])).astype(np.float32)
        gz = gumbel(rng, z0.shape)
    args = (None if factorized else t(z0, dev), t(y0, dev), tau, lam)
    noise = dict(noise_z=None if factorized else t(gz, dev), noise_y=t(gy, dev))
    # the reconstruction depends on the latents only: take the image to be it plus noise, so that the pair is correlated and
    # every (MS-)SSIM factor is well inside the positive range (a random network's output is unrelated to any other image)
    recon = model._sga.loss_and_grads(t(x, dev), *args, **noise)["recon"].cpu().numpy()[:, :h, :wd]
    x = (recon + 0.02 * rng.standard_normal(recon.shape)).astype(np.float32)
    r = model._sga.loss_and_grads(t(x, dev), *args, **noise)
    ref = sga_reference(tc, w, x, z0, y0, tau, gz, gy, lam, factorized=factorized)
    bpp = (r["bits_z"].cpu().numpy().mean() + r["bits_y"].cpu().numpy().mean()) / (h * wd)
    ms = float(r["msssim"].cpu().numpy().mean())
    loss = bpp + lam * (1.0 - ms)
    print(f"{case}: bpp {bpp:.6f} / {ref['bpp']:.6f}  msssim {ms:.7f} / {ref['msssim']:.7f}  loss {loss:.6f} / {ref['loss']:.6f}")
    assert abs(bpp - ref["bpp"]) < 2e-5 * ref["bpp"], (bpp, ref["bpp"])
    assert abs(ms - ref["msssim"]) < 3e-5 * ref["msssim"], (ms, ref["msssim"])
    assert abs(loss - ref["loss"]) < 2e-5 * ref["bpp"] + lam * 3e-5 * ref["msssim"], (loss, ref["loss"])
    for got, want, label in ((r["g_z"], ref["g_z"], "z"), (r["g_y"], ref["g_y"], "y")):
        if want is not None:
            assert_gradient(got.cpu().numpy(), want, f"{case} g_{label}")


def small_model(dev, lam, distortion="ms_ssim", factorized=False):
    if factorized:
        from shallow_ntc_amd.factorized.models import Model
        tc = dict(analysis=dict(cls="BLS2017Analysis", num_filters=32), synthesis=dict(cls="BLS2017Synthesis", num_filters=32))
    else:
        from shallow_ntc_amd.mshyper.models import Model
        tc = dict(TC)
    model = Model(device=dev, rd_lambda=lam, transform_config=tc, distortion=distortion, **ITINF)
    spread_weights(model, None if factorized else 64, seed=5)
    return model


def msssim_rd(m, lam):
    return m["bpp"] + lam * (1.0 - m["msssim"])


@pytest.mark.parametrize("factorized", [False, True], ids=["hyperprior", "factorized"])
def test_sga_optimisation_improves_rd_under_ms_ssim(factorized, dev):
    """tests/test_hip_sga.py::test_sga_optimisation_improves_rd with distortion="ms_ssim": after the same number of steps the
    hard-rounded validation loss bpp + lambda (1 - msssim) is lower than at step 0."""
    from shallow_ntc_amd.common import data_lib
    lam = 100.0
    model = small_model(dev, lam, factorized=factorized)
    x = data_lib.normalize_image(data_lib.synthetic_images(2, 64, 64, seed=4))
    before = model.validation_step(x).scalars_float
    model.initialize_itinf(x)
    first = None
    for step in range(150):
        m = model.itinf_train_step(x, seed=11).scalars_float
        first = first if first is not None else m
        assert np.isfinite(m["rd_loss"])
    assert model.global_step == 150
    assert m["rd_loss"] < first["rd_loss"]
    assert abs(m["rd_loss"] - msssim_rd(m, lam)) < 1e-5 * m["rd_loss"]
    after = model.itinf_validation_step(x).scalars_float
    print("before", before, "after", after)
    assert abs(after["rd_loss"] - msssim_rd(after, lam)) < 1e-5 * after["rd_loss"]
    assert msssim_rd(after, lam) < msssim_rd(before, lam), (before, after)
    assert {"rd_loss", "bpp", "mse", "psnr", "msssim", "msssim_db", "tau", "scheduled_lr", "sched_rd_lambda"} <= set(m)


def test_step_interface_and_refusals(dev):
    from shallow_ntc_amd import ops
    from shallow_ntc_amd.common import data_lib
    from shallow_ntc_amd.mshyper.models import Model
    with pytest.raises(ValueError):
        Model(device=dev, rd_lambda=1.0, transform_config=dict(TC), distortion="psnr", **ITINF)
    model = small_model(dev, 50.0)
    x = data_lib.normalize_image(data_lib.synthetic_images(1, 176, 192, seed=6))
    model.initialize_itinf(x)
    assert model.itinf_train_step(x, seed=3, fetch=False) is None
    assert model.itinf_train_step(x, seed=3, fetch=False) is None
    m = model.itinf_last_metrics().scalars_float
    assert np.isfinite(m["msssim"]) and m["msssim"] < 1 and np.isfinite(m["msssim_db"]) and np.isfinite(m["psnr"]) and m["mse"] > 0
    assert abs(m["rd_loss"] - msssim_rd(m, 50.0)) < 1e-5 * m["rd_loss"]
    # the forward-only training frame reports the same definition
    loss_t, mt = model.frame_loss_given_latent_rvs(x, model.latent_rvs, training=True, seed=3)
    assert abs(loss_t - msssim_rd(mt.scalars_float, 50.0)) < 1e-5 * loss_t
    with pytest.raises(NotImplementedError):
        model.train_step(x)
    thin = data_lib.normalize_image(data_lib.synthetic_images(1, 10, 300, seed=6))
    with pytest.raises(ValueError):
        model.itinf_train_step(thin, seed=3)
    with pytest.raises(ValueError):
        model.initialize_itinf(thin)
    with pytest.raises(ValueError):
        ops.msssim_distortion_grad(t(thin, dev), t(thin, dev), 1.0)


def test_mse_model_is_unchanged(dev):
    """distortion="mse" (the default): the step's tensors are bit-identical to ops.distortion_grad composed by hand, and the
    metric keys are the ones the step always had."""
    from shallow_ntc_amd import ops
    from shallow_ntc_amd.common import data_lib
    lam, tau = 0.02, 0.5
    model = small_model(dev, lam, distortion="mse")
    x = data_lib.normalize_image(data_lib.synthetic_images(2, 60, 64, seed=9))
    model.initialize_itinf(x)
    z0, y0 = (rv.loc.clone() for rv in model.latent_rvs.uq)
    rng = np.random.default_rng(3)
    gz, gy = t(gumbel(rng, tuple(z0.shape)), dev), t(gumbel(rng, tuple(y0.shape)), dev)
    xd = t(x, dev)
    r = model._sga.loss_and_grads(xd, z0, y0, tau, lam, noise_z=gz, noise_y=gy)
    assert "msssim" not in r
    eng, n = model._sga, x.shape[0]
    z_t, sp_z, dbz, bits_z = ops.sga_factorized_fwd(model._get_prior(), z0, tau, gz, 0, 0)
    hyper, acts = eng.hyper.forward(z_t)
    y_t, sp_y, dv, dr, bits_y = ops.sga_normal_fwd(y0, hyper, tau, gy, 0, 0)
    recon, cache = eng.syn.forward(y_t)
    g_x, sse = ops.distortion_grad(xd, recon, lam * 2.0 * 255.0 * 255.0 / (n * 60 * 64 * 3))
    g_y, g_hyper = ops.sga_normal_bwd(eng.syn.backward(g_x, cache), sp_y, dv, dr, 1.0 / (n * 60 * 64))
    g_z = ops.sga_chain(eng.hyper.backward(g_hyper, acts), dbz, sp_z, 1.0 / (n * 60 * 64))
    assert torch.equal(r["g_y"], g_y) and torch.equal(r["g_z"], g_z) and torch.equal(r["recon"], recon)
    assert torch.equal(r["bits_z"], bits_z) and torch.equal(r["bits_y"], bits_y)
    np.testing.assert_allclose(r["sse"].cpu().numpy(), sse.cpu().numpy(), rtol=1e-13)      # double atomics: not bitwise
    m = model.itinf_train_step(x, seed=1).scalars_float
    assert set(m) == {"rd_loss", "bpp", "mse", "psnr", "tau", "scheduled_lr", "sched_rd_lambda"}
    assert abs(m["rd_loss"] - (m["bpp"] + lam * m["mse"])) < 1e-5 * m["rd_loss"]
