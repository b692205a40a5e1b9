"""Mean-scale hyperprior model: the reference's ``Model`` API on the MI355X kernels.

Mirrors reference mshyper/models.py: constructor arguments (:46-51), ``infer_latent_rvs`` (:212-232),
``frame_loss_given_latent_rvs`` (:234-359), ``end_to_end_frame_loss`` (:361-373), ``validation_step``
(:385-387), ``evaluate`` (:415-433), ``downsample_factor`` (:137-140) and the ``Metrics.scalars`` keys
(:342-354: rd_loss, bpp, mse, psnr, scheduled_lr, sched_rd_lambda).  MS-SSIM / LPIPS (:321-340) and the
training step (:375-383) are out of scope.

Additionally exposes the codec regions SURVEY.md 8(d) measures: ``encode`` (x -> z_hat, symbols, bits)
and ``decode`` ((z_hat, symbols) -> uint8 pixels).
"""
from __future__ import annotations

import math
from collections import OrderedDict

import numpy as np
import torch

from .. import _capi as capi
from .. import ops
from ..common import data_lib, image_utils
from ..common.latent_rvs_lib import LatentRVCollection, UQLatentRV
from ..common.latent_rvs_utils import sga_schedule_at_step
from ..common.train_lib import Metrics
from ..common.transforms import class_builder as transform_builder
from ..entropy_coding import StepGrid, check_shifts, require_fp32

EMPTY_DICT = {}

# Fixed configs for the ScaleIndexedEntropyModel (reference :28-34); applied inside
# csrc/entropy.hip (kLogScaleMin, kScaleFactor).
NUM_SCALES = 64
SCALE_MIN = 0.11
SCALE_MAX = 256.0
SCALE_FACTOR = (math.log(SCALE_MAX) - math.log(SCALE_MIN)) / (NUM_SCALES - 1.0)
CODING_RANK = 3
DUMMY_IMG_DIM = 64
HIGHER_LAMBDA_UNTIL = 0.2
HIGHER_LAMBDA_FACTOR = 10.0


def step_lambdas(lam, steps, rd_lambda=None):
    """The weight of each image's distortion at its quantisation step, a pure function: -> float64 [n].  Default
    lambda_i = lam / step_size(k_i)^2: in the high-resolution regime D grows as the square of the step while the rate falls by
    log2 of it per element, so the slope -dR/dD the weights were trained to scales with step^-2 (a modelling choice,
    DESIGN.md 4.7).  ``rd_lambda``: a positive finite number, or one per image, instead."""
    from ..entropy_coding import step_size
    n = len(steps)
    if rd_lambda is None:
        return np.array([float(lam) / step_size(k) ** 2 for k in steps], np.float64)
    try:
        lams = np.asarray(rd_lambda, np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"rd_lambda must be a positive finite number or {n} of them, not {rd_lambda!r}") from None
    if lams.ndim == 0:
        lams = np.full(n, float(lams))
    if lams.shape != (n,) or not np.isfinite(lams).all() or not (lams > 0).all():
        raise ValueError(f"rd_lambda must be a positive finite number or {n} of them, not {rd_lambda!r}")
    return lams


def candidate_wins(j_cand, bits_cand, j_best, bits_best, budget_bits=None, flushed_bits=0.0, met=None):
    """The selection rule of ``compress(x, itinf=...)``, a pure function over per-image arrays: -> bool [n], True where the
    candidate replaces the image's best so far.  Without budgets: a strictly smaller J (the earlier candidate wins a tie).
    With ``budget_bits`` (``target_bpp``): where ``met`` (the start candidate fits) a candidate is eligible only if
    bits + flushed_bits <= budget, and wins by a strictly smaller J among the eligible; where not, the fewest bits win."""
    j_cand, bits_cand = np.asarray(j_cand, np.float64), np.asarray(bits_cand, np.float64)
    j_best, bits_best = np.asarray(j_best, np.float64), np.asarray(bits_best, np.float64)
    if budget_bits is None:
        return j_cand < j_best
    eligible = bits_cand + float(flushed_bits) <= np.asarray(budget_bits, np.float64)
    return np.where(np.asarray(met, bool), eligible & (j_cand < j_best), bits_cand < bits_best)


def weighted_distortion(sse_blocks, weights, elements):
    """D_w of ``coded_cost(..., weighted=True)``, a pure function: ``sse_blocks`` [n, hb, wb] = the integer squared error of the
    decoded pixels per pixel block (``ops.block_sse``), ``weights`` float64 [n, h, w] = ``entropy_coding.position_weights`` of the
    map with h >= hb, w >= wb (positions that lie wholly in the padding have no pixels), ``elements`` = H W C.
    -> float64 [n], sum_p weights[i, p] sse_blocks[i, p] / elements, each image's sum formed exactly (math.fsum) from its
    rounded products.  With a constant map this is step_lambdas(1.0, [k])[0] * sse_i / elements: the per-image rule's D_i
    times its weight."""
    s = np.asarray(sse_blocks, np.float64)
    w = np.asarray(weights, np.float64)
    if s.ndim != 3 or w.ndim != 3 or w.shape[0] != s.shape[0] or w.shape[1] < s.shape[1] or w.shape[2] < s.shape[2]:
        raise ValueError(f"weighted_distortion: blocks {s.shape} against weights {w.shape}")
    prod = w[:, :s.shape[1], :s.shape[2]] * s
    return np.array([math.fsum(row.ravel().tolist()) for row in prod], np.float64) / float(elements)


def deep_factorized_shapes(channels, num_filters=(3, 3)):
    filters = (1,) + tuple(num_filters) + (1,)
    d = OrderedDict()
    for k in range(len(filters) - 1):
        d[f"prior/matrix_{k}"] = (channels, filters[k + 1], filters[k])
        d[f"prior/bias_{k}"] = (channels, filters[k + 1])
        if k < len(filters) - 2:
            d[f"prior/factor_{k}"] = (channels, filters[k + 1])
    return d


def deep_factorized_init(channels, num_filters=(3, 3), init_scale=10.0, seed=4321):
    """tfc.DeepFactorized initial values: matrix = log(expm1(1/scale/f_{k+1})), bias ~ U(-.5,.5), factor = 0."""
    rng = np.random.default_rng(seed)
    filters = (1,) + tuple(num_filters) + (1,)
    scale = init_scale ** (1.0 / (len(num_filters) + 1))
    out = OrderedDict()
    for name, shp in deep_factorized_shapes(channels, num_filters).items():
        kind, k = name.split("/")[1].rsplit("_", 1)
        if kind == "matrix":
            v = np.full(shp, np.log(np.expm1(1.0 / scale / filters[int(k) + 1])))
        elif kind == "bias":
            v = rng.uniform(-0.5, 0.5, size=shp)
        else:
            v = np.zeros(shp)
        out[name] = v.astype(np.float32)
    return out


def compression_lr(optimizer_config, scheduled_num_steps, step):
    """Learning rate the reference's Adam uses for the update taken at optimizer iteration ``step`` (0-based):
    CompressionSchedule (common/schedule.py:155-176 via mshyper/models.py:95-108) = base * piecewise-constant
    [1, reduce_lr_factor] switching at int(reduce_lr_after * total) (boundary <= step picks the second value,
    schedule.py:46-48) * linear warm-up min(1, (step + 1) / warmup_steps) (schedule.py:121-123 -- the `+ 1` makes the
    very first update non-zero, and the warm-up factor also multiplies the dropped value)."""
    cfg = optimizer_config
    lr = cfg.get("learning_rate", 1e-4)
    after = cfg.get("reduce_lr_after", 0.8)
    factor = cfg.get("reduce_lr_factor", 0.1)
    warmup = cfg["warmup_steps"] if "warmup_steps" in cfg else int(cfg.get("warmup_until", 0.02) * scheduled_num_steps)
    value = lr * (factor if step >= int(after * scheduled_num_steps) else 1.0)
    if warmup > 0:
        value *= min(1.0, (step + 1) / warmup)
    return value


class Model:
    """Encapsulates the transforms + entropy models (reference :45-149)."""

    factorized = False

    def __init__(self, scheduled_num_steps=1500000, rd_lambda=0.01, offset_heuristic=True,
                 transform_config=EMPTY_DICT, optimizer_config=EMPTY_DICT,
                 latent_config=None, profile=False, device=None, prior_num_filters=(3, 3), seed=4321,
                 quality_metrics=True, precision="fp32", distortion="mse"):
        """``distortion``: "mse" (default) or "ms_ssim": what SGA iterative inference (``itinf_train_step``) descends.
        "ms_ssim": rd_loss = bpp + rd_lambda * (1 - mean_B q_i), q_i the (MS-)SSIM of reference :321-331 on the unrounded
        0-255 floats (single-scale SSIM when both sides are < 160).  rd_lambda is NOT rescaled: 1 - q lies in
        [0, 1] where the MSE of 0-255 pixels runs to the hundreds, so useful values are orders of magnitude larger than for
        "mse".  Images on which the metric is not computable raise ValueError; training (``train_step``) is MSE only.
        ``precision``: "fp32" (default: exact fp32 MFMA everywhere, the reference's arithmetic) or "bf16x3": the
        convolutions that qualify (Cin % 16 == 0, at least one 256-row strip per image) run the split-precision contraction
        on pre-split operands (csrc/bf3_gemm.hip; ~fp32 accuracy, not bit-identical to it).  An encoder and a decoder must
        use the same precision: the bitstream header carries it."""
        capi.require_gpu()
        self._scheduled_num_steps = scheduled_num_steps
        self._rd_lambda = rd_lambda
        self._latent_config = dict(latent_config) if latent_config is not None else dict(uq=dict(method="unoise"))
        uq_method = self._latent_config["uq"].get("method", "unoise")
        if uq_method == "mixedq" and offset_heuristic:
            offset_heuristic = False      # reference :70-76
        self._offset_heuristic = offset_heuristic
        self.itinf = False
        self._optimizer_config = dict(optimizer_config)
        self._transform_config = transform_config
        self._profile = profile
        self._prior_num_filters = tuple(prior_num_filters)
        if precision not in ("fp32", "bf16x3"):
            raise ValueError(f"precision must be 'fp32' or 'bf16x3', not {precision!r}")
        self._precision = precision
        if distortion not in ("mse", "ms_ssim"):
            raise ValueError(f"distortion must be 'mse' or 'ms_ssim', not {distortion!r}")
        self._distortion = distortion
        self._seed = seed
        self._quality_metrics = quality_metrics     # MS-SSIM at eval (reference :321-331); LPIPS is not vendored
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self._step = 0
        self._timing = {}
        self._prior = None
        self._init_transforms(transform_config)

    # -- construction (reference :111-149) ---------------------------------------------------------
    def _build_named(self, cfg, cin, seed_offset):
        cfg = dict(cfg)
        t = transform_builder.build(cfg.pop("cls"), **cfg)
        t._precision = self._precision
        t._seed = self._seed + seed_offset
        t._cin = t._cin or cin
        return t

    def _init_transforms(self, transform_config=EMPTY_DICT):
        self._analysis = self._build_named(transform_config["analysis"], 3, 0)
        self._bottleneck_size = b = self._analysis.out_channels(3)
        self._synthesis = self._build_named(transform_config["synthesis"], b, 1)
        ha = transform_config.get("hyper_analysis", dict(cls="HyperAnalysis", bottleneck_size=b))
        hs = transform_config.get("hyper_synthesis", dict(cls="HyperSynthesis", bottleneck_size=b))
        self._hyper_analysis = self._build_named(ha, b, 2)
        self._hyper_bottleneck_size = hb = self._hyper_analysis.out_channels(b)
        self._hyper_synthesis = self._build_named(hs, hb, 3)
        if self._hyper_synthesis.out_channels(hb) != 2 * b:
            raise ValueError("hyper-synthesis must emit 2 * bottleneck channels (mean and scale)")
        self._prior_weights = deep_factorized_init(hb, self._prior_num_filters, seed=self._seed + 4)
        # downsample_factor = 64 / spatial size of the hyper-latents of a 64 x 64 dummy image (:137-140)
        self.downsample_factor = self._compute_downsample_factor()

    def _transforms(self):
        return OrderedDict(analysis=self._analysis, synthesis=self._synthesis,
                           hyper_analysis=self._hyper_analysis, hyper_synthesis=self._hyper_synthesis)

    def _compute_downsample_factor(self):
        for t in self._transforms().values():
            t.build(device=self.device)
        # the reference pushes a zero 64 x 64 image through analysis + hyper-analysis; the spatial size of
        # the result is all it uses, so shape inference suffices
        _, dim = self._hyper_analysis.out_hw(*self._analysis.out_hw(DUMMY_IMG_DIM, DUMMY_IMG_DIM))
        factor = int(DUMMY_IMG_DIM / dim)
        assert dim * factor == DUMMY_IMG_DIM, "Downsample factor should divide evenly into the dummy image size."
        return factor

    # -- weights --------------------------------------------------------------------------------
    def get_weights(self):
        """Flat ``{prefix/name: ndarray}`` over all transforms + the hyper-prior ('prior/...')."""
        out = OrderedDict()
        for pre, t in self._transforms().items():
            for k, v in t.get_weights().items():
                out[f"{pre}/{k}"] = v
        out.update(self._prior_weights)
        return out

    def set_weights(self, weights, _from_trainer=False):
        """Load variables (``get_weights()`` naming).  A ``Trainer`` attached to this model keeps its own flat copy of the
        variables and the Adam moments: weights set from anywhere else make that state stale, so it is dropped and the
        next ``train_step`` builds a fresh one from these weights and ``self._step``."""
        if not _from_trainer:
            self.trainer = None
        for pre, t in self._transforms().items():
            sub = {k[len(pre) + 1:]: v for k, v in weights.items() if k.startswith(pre + "/")}
            t.set_weights(sub)
            t.build(device=self.device)
        shapes = deep_factorized_shapes(self._prior_channels(), self._prior_num_filters)
        pw = OrderedDict()
        for k, shp in shapes.items():
            a = np.asarray(weights[k], np.float32)
            if tuple(a.shape) != tuple(shp):
                raise ValueError(f"{k}: expected {shp}, got {a.shape}")
            pw[k] = a
        self._prior_weights = pw
        self._prior = None
        self._codec = None
        self._latent_gains = None

    def _prior_channels(self):
        return self._hyper_bottleneck_size

    def _get_prior(self):
        if self._prior is None:
            nl = len(self._prior_num_filters) + 1
            pw = self._prior_weights
            with torch.cuda.device(self.device):
                self._prior = ops.DeepFactorizedPrior([pw[f"prior/matrix_{k}"] for k in range(nl)],
                                                      [pw[f"prior/bias_{k}"] for k in range(nl)],
                                                      [pw[f"prior/factor_{k}"] for k in range(nl - 1)])
        return self._prior

    # -- schedules (reference :151-209) ----------------------------------------------------------
    @property
    def global_step(self):
        return self._itinf_step if self.itinf else self._step

    @property
    def _scheduled_lr(self):
        return compression_lr(self._optimizer_config, self._scheduled_num_steps, self.global_step)

    @property
    def _scheduled_rd_lambda(self):
        if self._rd_lambda <= 0.01 and not self.itinf:
            boundary = int(self._scheduled_num_steps * HIGHER_LAMBDA_UNTIL)
            return self._rd_lambda * (HIGHER_LAMBDA_FACTOR if self.global_step < boundary else 1.0)
        return self._rd_lambda

    @property
    def latent_config(self):
        config = {k: dict(v) if isinstance(v, dict) else v for k, v in self._latent_config.items()}
        cfg = config.get("uq")
        if cfg and cfg.get("method") == "sga":
            cfg["tau"] = sga_schedule_at_step(self.global_step, r=cfg["tau_r"], ub=cfg["tau_ub"],
                                              lb=cfg.get("tau_lb", 1e-8), t0=cfg["tau_t0"])
        return config

    # -- inference path (reference :212-232) -----------------------------------------------------
    def _as_device_images(self, x):
        if isinstance(x, np.ndarray):
            if x.dtype == np.uint8:                                   # raw pixels: scale as data_lib.py:24-25 does
                x = data_lib.normalize_image(x)
            x = ops.to_device(x, self.device)
        if x.dim() == 3:
            x = x.unsqueeze(0)
        return x.contiguous()

    def _timed(self, name, fn, *args):
        """``profile=True`` (reference :142-149, common/profile_utils.py:62-77): per-transform wall time as Metrics scalars
        ``<name>_time`` in seconds -- here GPU time between two HIP events on the launch stream (the reference's
        perf_counter around a tf.function is documented as inaccurate, README.md:44-45)."""
        if not self._profile:
            return fn(*args)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(*args)
        e1.record()
        e1.synchronize()
        self._timing[f"{name}_time"] = e0.elapsed_time(e1) * 1e-3
        return out

    def infer_latent_rvs(self, x):
        x = self._as_device_images(x)
        self._timing = {}
        with torch.cuda.device(self.device):
            xp = image_utils.pad_images(x, self.downsample_factor)
            y = self._timed("analysis", self._analysis, xp)
            z = self._timed("hyper_analysis", self._hyper_analysis, y)
        return LatentRVCollection(uq=(UQLatentRV(z), UQLatentRV(y)))

    # -- generative path + losses (reference :234-359, training=False branch) ------------------------
    def _rate_and_reconstruction(self, latent_rvs, want_symbols=False):
        z, y = latent_rvs.uq[0].loc, latent_rvs.uq[1].loc
        z_hat, bits_z = self._get_prior()(z)                          # :254-259 (offset 0)
        hyper = self._timed("hyper_synthesis", self._hyper_synthesis, z_hat)    # :273; split + exp fused below
        y_hat, bits_y, sym = ops.entropy_scale_normal(y, hyper, want_symbols)   # :274-279
        recon = self._timed("synthesis", self._synthesis, y_hat)                # :297
        return dict(z_hat=z_hat, y_hat=y_hat, symbols=sym, hyper=hyper, bits_z=bits_z, bits_y=bits_y, recon=recon)

    def frame_loss_given_latent_rvs(self, image_batch, latent_rvs, training, noise=None, seed=None):
        """reference :234-359.  ``training=False``: hard rounding, uint8 distortion, MS-SSIM.  ``training=True``: the loss value
        the reference's ``train_step`` / ``itinf_train_step`` differentiate -- the latents are perturbed as
        ``latent_config['uq']['method']`` says ('unoise' / 'mixedq': additive uniform noise, :253-259,277-283; anything else,
        e.g. 'sga' / 'soft_round': explicit ``UQLatentRV.sample``, :260-268,285-291), the rate is the noisy densities' at those
        samples and the distortion is taken on unrounded 0-255 floats (data_lib.py:48-52).  Forward value only: the
        gradients live in ``train_step`` (shallow_ntc_amd.train.Trainer) and ``itinf_train_step`` (sga.SGAEngine), which
        draw the same numbers from the same (seed, step).  ``noise`` = (for z, for y) fixes the draw (tests)."""
        if training:
            return self._training_frame(image_batch, latent_rvs, noise, seed)
        return self._finish_frame(self._launch_frame(image_batch, latent_rvs))

    def _training_samples(self, latent_rvs, noise, seed):
        """-> (bits_z[n] or None, bits_y[n], the tensor the synthesis decodes): the training=True branch up to the synthesis."""
        uq = self._latent_config["uq"].get("method", "unoise")
        step = self.global_step
        nz, ny = (None, None) if noise is None else noise
        z_rv, y_rv = latent_rvs.uq
        prior = self._get_prior()
        if uq in ("unoise", "mixedq"):
            z_t = z_rv.sample(True, "unoise", noise=nz, seed=seed, step=2 * step)                 # :253-259
            bits_z, _ = ops.noisy_factorized(prior, z_t)
            z_dec = z_rv.quantize() if uq == "mixedq" else z_t                                    # offset 0
            hyper = self._hyper_synthesis(z_dec)                                                  # :273
            y_t = y_rv.sample(True, "unoise", noise=ny, seed=seed, step=2 * step + 1)             # :277-283
            bits_y, _, _ = ops.noisy_normal(y_t, hyper)
            y_dec = ops.entropy_scale_normal(y_rv.loc, hyper)[0] if uq == "mixedq" else y_t
            return bits_z, bits_y, y_dec
        cfg = dict(self.latent_config["uq"])                                                      # explicit sampling, :260-268
        if uq == "sga":       # the fused kernels of itinf_train_step: same draw, same rate arithmetic
            z_t, _, _, bits_z = ops.sga_factorized_fwd(prior, z_rv.loc, cfg["tau"], nz, seed, step)
            hyper = self._hyper_synthesis(z_t)
            y_t, _, _, _, bits_y = ops.sga_normal_fwd(y_rv.loc, hyper, cfg["tau"], ny, seed, step)
            return bits_z, bits_y, y_t
        z_t = z_rv.sample(True, offset=None, noise=nz, seed=seed, step=2 * step, **cfg)
        bits_z, _ = ops.noisy_factorized(prior, z_t)
        hyper = self._hyper_synthesis(z_t)
        c = y_rv.loc.shape[-1]
        y_t = y_rv.sample(True, offset=hyper[..., :c], noise=ny, seed=seed, step=2 * step + 1, **cfg)       # :285-291
        bits_y, _, _ = ops.noisy_normal(y_t, hyper)
        return bits_z, bits_y, y_t

    def _training_frame(self, image_batch, latent_rvs, noise=None, seed=None):
        x = self._as_device_images(image_batch)
        seed = self._seed if seed is None else seed
        with torch.cuda.device(self.device):
            bits_z, bits_y, y_dec = self._training_samples(latent_rvs, noise, seed)
            recon = self._synthesis(y_dec, training=True)                                         # :297
            sse = ops.float_sse(x, recon)                                                         # unpad + 0-255 floats, unrounded
            rows = [bits_y if bits_z is None else bits_z, bits_y, sse]
            msssim = None
            if self._distortion == "ms_ssim":                                                     # the same unrounded floats
                ops.msssim_scale_sizes(x.shape[1], x.shape[2])
                a, b, _ = ops.msssim_inputs(x, recon)
                msssim = ops.image_quality(a, b, 255.0)
            host = torch.stack(rows).cpu().numpy()
            ops.check_conv_status()
        rd_loss, metrics = self._finish_metrics(x.shape, None if bits_z is None else host[0], host[1], host[2], msssim)
        metrics.record_image("reconstruction", recon)
        return rd_loss, metrics

    def _launch_frame(self, image_batch, latent_rvs=None):
        """Everything of end_to_end_frame_loss(training=False) that runs on the GPU, launched on the current stream with
        no host synchronisation: -> the pending device results for ``_finish_frame``."""
        x = self._as_device_images(image_batch)
        with torch.cuda.device(self.device):
            if latent_rvs is None:
                latent_rvs = self.infer_latent_rvs(x)
            r = self._rate_and_reconstruction(latent_rvs)
            sse, _ = ops.pixels_sse(x, r["recon"])                    # unpad + floats_to_pixels + mse fused
            dev = torch.stack([r["bits_z"], r["bits_y"], sse.to(torch.float64)])
            quality = None
            h, w = x.shape[1], x.shape[2]
            if self._msssim_applies(h, w):
                quality = ops.image_quality_launch(ops.pixels_float(x, h, w), ops.pixels_float(r["recon"], h, w), 255.0)
        return dict(shape=tuple(x.shape), dev=dev, quality=quality, recon=r["recon"])

    def _finish_frame(self, pending):
        """Host side of a launched frame: one device -> host copy, then the reference's float32 metric arithmetic."""
        host = pending["dev"].cpu().numpy()
        ops.check_conv_status()                      # the copy above synchronised the stream: a flagged stream-K launch raises here
        msssim = None
        if pending["quality"] is not None:
            sums, counts, single = pending["quality"]
            msssim = ops.image_quality_finish(sums.cpu().numpy(), counts, single)
        rd_loss, metrics = self._finish_metrics(pending["shape"], host[0], host[1], host[2], msssim)
        metrics.record_image("reconstruction", pending["recon"])
        return rd_loss, metrics

    def _msssim_applies(self, h, w):
        """reference :321-331: (MS-)SSIM of the uint8-quantised images whenever TensorFlow itself can compute it."""
        if self._distortion == "ms_ssim":      # the loss itself: computed wherever the kernels can, ValueError elsewhere
            ops.msssim_scale_sizes(h, w)
            return True
        if not self._quality_metrics or min(h, w) < 11:
            return False
        # the reference switches to ssim_multiscale once either side reaches 160 (:325-329), which TensorFlow itself
        # rejects when the fifth scale is smaller than the 11 x 11 window; report no MS-SSIM instead of failing the step
        return not ((h >= 160 or w >= 160) and min(h, w) < 11 * 16)

    def _msssim(self, x, recon):
        """Per-image (MS-)SSIM of the uint8-quantised images (reference :321-331), or None."""
        h, w = x.shape[1], x.shape[2]
        if not self._msssim_applies(h, w):
            return None
        return ops.image_quality(ops.pixels_float(x, h, w), ops.pixels_float(recon, h, w), 255.0)

    def _finish_metrics(self, x_shape, bits_z, bits_y, sse, msssim=None, sched=None, lams=None, wsse=None):
        """``sched`` = (scheduled_lr, sched_rd_lambda, tau) of the step the numbers belong to, when that is not the current one
        (metrics of an SGA step fetched later).  ``lams``: one lambda per image (SGA at a quantisation step): rd_loss =
        bpp + mean_i(lambda_i D_i); every other scalar is unchanged.  ``wsse``: each image's weighted squared error (SGA on a
        step map): rd_loss = bpp + lambda mean_i(wsse_i / (H W C))."""
        n, h, w, c = x_shape
        num_pixels = np.float32(h * w)                                                  # :302
        bits_z = None if bits_z is None else bits_z.astype(np.float32)
        bits_y = bits_y.astype(np.float32)
        hyper_bpp = np.float32(0.0) if bits_z is None else np.float32(bits_z.mean(dtype=np.float32) / num_pixels)
        latent_bpp = np.float32(bits_y.mean(dtype=np.float32) / num_pixels)           # :306-307
        for name, v in (("hyper_latent_bpp", hyper_bpp), ("latent_bpp", latent_bpp)):
            if not np.isfinite(v):                                                      # check_numerics :308-309
                raise capi.NonFiniteError(capi.ERR_NONFINITE, f"{name} : Tensor had NaN/Inf values")
        bpp = np.float32(hyper_bpp + latent_bpp)
        mses, psnrs = image_utils.mse_psnr_from_sse(sse, h * w * c)                     # :315
        mse, psnr = np.float32(mses.mean(dtype=np.float32)), np.float32(psnrs.mean(dtype=np.float32))
        lam = self._scheduled_rd_lambda if sched is None else sched[1]
        rd_loss = np.float32(bpp + np.float32(lam) * mse)                               # :343
        if self._distortion == "ms_ssim":                                               # bpp + lambda (1 - mean_B q_i)
            if msssim is None:
                raise ValueError("distortion='ms_ssim': no (MS-)SSIM was computed for this frame")
            rd_loss = np.float32(bpp + np.float32(lam) * np.float32(1.0 - np.asarray(msssim, np.float64).mean()))
        if lams is not None:
            d = 1.0 - np.asarray(msssim, np.float64) if self._distortion == "ms_ssim" else mses.astype(np.float64)
            rd_loss = np.float32(bpp + np.float32((np.asarray(lams, np.float64) * d).mean()))
        if wsse is not None:
            rd_loss = np.float32(bpp + np.float32(float(lam) * (np.asarray(wsse, np.float64) / float(h * w * c)).mean()))
        if not np.isfinite(rd_loss):                                                    # :356
            raise capi.NonFiniteError(capi.ERR_NONFINITE, "rd_loss : Tensor had NaN/Inf values")
        metrics = Metrics.make()
        metrics.record_scalar("sched_rd_lambda", lam)
        if self.latent_config["uq"].get("method") == "sga":
            metrics.record_scalar("tau", self.latent_config["uq"]["tau"] if sched is None else sched[2])
        if msssim is not None:                                                          # :321-331
            ms = np.float32(np.asarray(msssim, np.float32).mean(dtype=np.float32))
            with np.errstate(divide="ignore"):
                db = np.float32((-10.0 * np.log10(1.0 - np.asarray(msssim, np.float64))).mean())
            metrics.record_scalars(dict(msssim=float(ms), msssim_db=float(db)))
        metrics.record_scalars(dict(rd_loss=float(rd_loss), bpp=float(bpp), mse=float(mse), psnr=float(psnr),
                                    scheduled_lr=self._scheduled_lr if sched is None else sched[0]))
        if self._profile:                                                               # :350-351
            metrics.record_scalars(dict(getattr(self, "_timing", {})))
        return float(rd_loss), metrics

    def end_to_end_frame_loss(self, image_batch, training):
        latent_rvs = self.infer_latent_rvs(image_batch)
        return self.frame_loss_given_latent_rvs(image_batch, latent_rvs=latent_rvs, training=training)

    def validation_step(self, image_batch, training=False) -> Metrics:
        _, metrics = self.end_to_end_frame_loss(image_batch, training=training)
        return metrics

    def evaluate(self, images, lookahead=3, group=8):
        """Reference :415-433: a [B,H,W,3] tensor is evaluated one [1,H,W,3] image at a time, an
        iterable is taken as is; yields one Metrics per image, in order.

        Same numbers as the reference's loop, image by image and in order, but not its stalls.  One image alone leaves most
        of the GPU idle (a 512 x 768 image is 72 ... 288 workgroups per layer on 256 CUs), so up to ``group`` images OF THE
        SAME SHAPE among the next ``lookahead * group`` are launched as one batch -- every kernel on this path gives an
        image bit-identical results alone or inside any batch -- and up to ``lookahead`` such launches are
        in flight on round-robin HIP streams before the oldest one's results are copied to the host, so the device never
        waits for Python.  lookahead=1 is the strictly serial one-image-per-pass reference behaviour.  (Defaults from
        tools/time_evaluate.py on the Kodak-shaped set: 4 x 4 178, 2 x 8 189, 3 x 8 204 Mpixel/s untuned; the launches of eight
        images fill the quarter-resolution layers' 8 x 32 tiles for one and a half rounds of the device instead of three quarters of one.)"""
        tensor_input = isinstance(images, (torch.Tensor, np.ndarray))
        if tensor_input:
            images = [images[i:i + 1] for i in range(images.shape[0])]
        lookahead, group = max(1, int(lookahead)), max(1, int(group))
        if lookahead == 1:
            for img in images:
                _, metrics = self.end_to_end_frame_loss(img, training=False)
                yield metrics
            return
        if self._profile:
            group = 1                                                 # per-transform times are per pass
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream()
            self._eval_streams = ops.side_streams(lookahead, self.device)      # the library's one pool: a stream per hardware queue
            window = []                  # entries in input order: [x, metrics or None, launched]
            inflight = []                # (stream, pending, entries)
            it = iter(images)
            k = 0
            done = False
            while True:
                while not done and len(window) < lookahead * group:
                    try:
                        window.append([self._as_device_images(next(it)), None, False])
                    except StopIteration:
                        done = True
                while len(inflight) < lookahead:
                    first = next((e for e in window if not e[2]), None)
                    if first is None:
                        break
                    members = [e for e in window if not e[2] and e[0].shape == first[0].shape][:group]
                    if first[0].shape[0] != 1:
                        members = [first]                             # an iterable of batches: each is taken as it is
                    for e in members:
                        e[2] = True
                    st = self._eval_streams[k % lookahead]
                    k += 1
                    st.wait_stream(cur)
                    with torch.cuda.stream(st):
                        x = members[0][0] if len(members) == 1 else torch.cat([e[0] for e in members])
                        inflight.append((st, self._launch_frame(x), members))
                if not inflight:
                    break
                st, pending, members = inflight.pop(0)
                with torch.cuda.stream(st):
                    for e, (_, metrics) in zip(members, self._finish_frames(pending, len(members))):
                        e[1] = metrics
                while window and window[0][1] is not None:
                    yield window.pop(0)[1]
            for st in self._eval_streams:
                cur.wait_stream(st)

    def _finish_frames(self, pending, count):
        """``_finish_frame`` for a launch that holds ``count`` one-image frames: one host copy, then each image's own
        metrics exactly as if it had been launched alone."""
        if count == 1:
            return [self._finish_frame(pending)]
        host = pending["dev"].cpu().numpy()
        ops.check_conv_status()
        msssim = None
        if pending["quality"] is not None:
            sums, counts, single = pending["quality"]
            msssim = ops.image_quality_finish(sums.cpu().numpy(), counts, single)
        out = []
        for i in range(count):
            rd_loss, metrics = self._finish_metrics((1,) + tuple(pending["shape"][1:]), host[0][i:i + 1], host[1][i:i + 1],
                                                    host[2][i:i + 1], None if msssim is None else msssim[i:i + 1])
            metrics.record_image("reconstruction", pending["recon"][i:i + 1])
            out.append((rd_loss, metrics))
        return out

    def evaluate_batched(self, images):
        """Same numbers as ``evaluate`` for same-shaped images, but one launch sequence for the whole
        batch (independent images fill the GPU): returns per-image dicts(bpp, mse, psnr, rd_loss)."""
        x = self._as_device_images(images)
        with torch.cuda.device(self.device):
            r = self._rate_and_reconstruction(self.infer_latent_rvs(x))
            sse, _ = ops.pixels_sse(x, r["recon"])
            host = torch.stack([r["bits_z"], r["bits_y"], sse.to(torch.float64)]).cpu().numpy()
            ops.check_conv_status()
            msssim = self._msssim(x, r["recon"])
        out = []
        for i in range(x.shape[0]):
            _, m = self._finish_metrics((1,) + tuple(x.shape[1:]), host[0][i:i + 1], host[1][i:i + 1], host[2][i:i + 1],
                                        None if msssim is None else msssim[i:i + 1])
            out.append(m.scalars_float)
        return out

    # -- codec regions -------------------------------------------------------------
    def encode(self, x, check=True):
        """x -> (z_hat, symbols int32, bits_z[n], bits_y[n]); needs the hyper-synthesis for mu, sigma.  ``check``: wait for the
        launches and raise if a stream-K hand-off timed out (``ops.check_conv_status``); a caller that keeps several calls in
        flight passes False and checks where it synchronises itself."""
        x = self._as_device_images(x)
        with torch.cuda.device(self.device):
            lat = self.infer_latent_rvs(x)
            z_hat, bits_z = self._get_prior()(lat.uq[0].loc)
            hyper = self._hyper_synthesis(z_hat)
            _, bits_y, sym = ops.entropy_scale_normal(lat.uq[1].loc, hyper, want_symbols=True)
            if check:
                ops.check_conv_status()
        return z_hat, sym, bits_z, bits_y

    def decode(self, z_hat, symbols, image_hw, reference=None, check=True, step=None, step_offsets=None):
        """(z_hat, symbols) -> hyper-synthesis -> y_hat = symbols + mu -> synthesis -> uint8 pixels
        [n, H, W, 3] (and the per-image integer SSE against ``reference`` if given).  ``check`` as in ``encode``.
        ``step``: the ladder index (or one per image) the symbols were quantised with (``compress(step=...)``):
        y_hat = fma(step_size(k), symbols, mu).  ``step_offsets``: the per-position offsets they were quantised with
        (``compress(step_offsets=...)``): k = clip(step + step_offsets) per latent position."""
        self._check_step_arguments("decode", step, step_offsets=step_offsets)
        grid = None
        if step is not None or step_offsets is not None:
            grid = self._get_codec()._grid(step, step_offsets, symbols.shape[0], int(image_hw[0]), int(image_hw[1]))
        with torch.cuda.device(self.device):
            if grid is not None and grid.kind != "unit":
                grid.on(self.device)
                y_hat = grid.dequant(symbols, self._hyper_synthesis.leading_channels(z_hat, symbols.shape[-1]))
            elif self._synthesis.takes_s3(symbols.shape[1], symbols.shape[2]):      # bf16x3: y_hat leaves the dequantisation pre-split
                y_hat = ops.dequant_split3(symbols, self._hyper_synthesis(z_hat))
            else:     # mu only: the last hyper-synthesis layer skips its raw-sigma columns where its plan can, and adds the
                      # symbols in its epilogue (same bits; ops.FUSE_DEQUANT)
                y_hat = self._hyper_synthesis.dequantised(z_hat, symbols)
            out = self._pixels(y_hat, image_hw, reference)
            if check:
                ops.check_conv_status()
            return out

    def decode_set(self, codes, check=True):
        """``decode`` for a SET of batches of different image sizes (the Kodak set's two orientations): ``codes`` =
        [(z_hat, symbols, image_hw[, reference])] -> the list of what ``decode`` returns for each.  The hyper-syntheses and
        dequantisations of the batches run side by side on one stream per batch; a two-layer synthesis then takes ALL batches
        in ONE launch (common/transforms.py ``hidden_many``: per-image geometry inside the kernel), and the output layers
        follow per batch.  Same pixels as one ``decode`` per batch."""
        codes = [tuple(c) + (None,) * (4 - len(c)) for c in codes]
        syn = self._synthesis
        if len(codes) < 2 or len(codes) > 4 or not hasattr(syn, "hidden_many") or self._synthesis.takes_s3(*codes[0][1].shape[1:3]):
            return [self.decode(z, s, hw, reference=r, check=check) for z, s, hw, r in codes]
        with torch.cuda.device(self.device):
            cur, lanes = ops.lanes(len(codes), self.device)
            y_hats = []
            for st, (z_hat, sym, _hw, _r) in zip(lanes, codes):
                with ops.fork(cur, st):
                    y_hats.append(self._hyper_synthesis.dequantised(z_hat, sym))
            for st, y_hat in zip(lanes, y_hats):
                ops.join(cur, st, made=(y_hat,))
            hidden = syn.hidden_many(y_hats)
            outs = []
            if hidden is None:
                for y_hat, (_z, _s, hw, ref) in zip(y_hats, codes):
                    outs.append(self._pixels(y_hat, hw, ref))
            else:
                for st, hid, (_z, _s, hw, ref) in zip(lanes, hidden, codes):
                    with ops.fork(cur, st, reads=(hid,)):
                        px, sse = syn.pixels_from_hidden(hid, hw[0], hw[1], ref)
                    outs.append(px if ref is None else (px, sse))
                for st, out in zip(lanes, outs):
                    ops.join(cur, st, made=out if isinstance(out, tuple) else (out,))
            if check:
                ops.check_conv_status()
            return outs

    def _pixels(self, y_hat, image_hw, reference=None):
        """synthesis -> unpad -> floats_to_pixels -> quantize_image (reference :297-317) as uint8 [n, H, W, 3], plus the
        per-image integer SSE when ``reference`` is given.  The two-layer syntheses emit the pixels from their last
        launch; the others go through the float reconstruction."""
        if hasattr(self._synthesis, "forward_pixels"):
            px, sse = self._synthesis.forward_pixels(y_hat, image_hw[0], image_hw[1], reference)
            return px if reference is None else (px, sse)
        recon = self._synthesis(y_hat)
        if reference is None:
            return ops.to_pixels(recon, image_hw[0], image_hw[1])
        sse, px = ops.pixels_sse(reference, recon, want_pixels=True)
        return px, sse

    # -- bitstream (the reference itself only estimates the rate) -----------------------
    def _get_codec(self):
        from ..entropy_coding import Codec
        if getattr(self, "_codec", None) is None:
            self._codec = Codec(self)
        return self._codec

    def compress(self, x, itinf=None, step=None, target_bpp=None, step_offsets=None, target_psnr=None, max_error=None,
                 rdoq=None, tile=None, overlap=16) -> bytes:
        """Images -> self-contained bitstream (rANS over the integer CDF tables of both entropy models).
        ``itinf`` = dict(steps, seed=0, check_every=None): refine the latents of THESE images by SGA iterative inference first
        (``initialize_itinf`` + ``steps`` x ``itinf_train_step(x, seed=seed, fetch=False)`` under the model's own tau / learning-rate
        schedules) and code, per image, the candidate with the smallest exact coded cost J (``coded_cost``) among the encoder's
        own latents (step 0), every ``check_every``-th step if given, and the last step -- so the file is never worse, by J, than
        that of ``compress(x)``.  ``last_compress_report`` then lists, per image, step_chosen, J_start, J_chosen, bits_start,
        bits_chosen, and ``last_compress_latents`` holds what was coded.  Needs latent_config uq.method == 'sga' and precision
        'fp32'; leaves the model in iterative-inference mode, as ``initialize_itinf`` does.
        ``step`` (an index k on the scale ladder, entropy_coding.STEP_MIN .. STEP_MAX, or one per image): quantise y - mu with
        the step entropy_coding.step_size(k) = r^k instead of 1 and code with the tables k places down the ladder -- other rates
        from the same weights; step 0 is the file of ``compress(x)``, byte for byte.
        ``target_bpp`` (a number, or one per image): per image the finest step whose predicted payload fits target_bpp H W bits,
        STEP_MAX where none does; ``last_compress_report`` lists step_chosen, bits_predicted, budget_bits, met.
        An escaped symbol travels in 16 bits: at index k the file clamps |y - mu| beyond 32767 step_size(k) (639 at k = -32),
        while ``coded_cost`` decodes the unclamped symbol -- the known limit of the format, 1 / step_size(k) closer at fine steps.
        Mean-scale hyperprior models in precision 'fp32' only; ``step``, ``target_bpp`` and ``itinf`` exclude each other.
        Refinement AT a step travels inside the dict: ``itinf`` = dict(steps, ..., step=k | [k_i], rd_lambda=None) runs SGA on the
        grid of step_size(k_i) with the rate of the tables k_i places down the ladder, judges the candidates by
        ``coded_cost(x, latents, step=ks)`` and writes ``compress_latents(..., step=ks)``; every index 0 is the file of
        ``itinf=dict(steps, ...)``, byte for byte.  Image i's distortion is weighted with lambda_i = lambda / step_size(k_i)^2
        (``rd_lambda``: a number or one per image instead) in the loss descended and in J_i = bits_i / (H W) + lambda_i D_i, so
        "never a worse file, by J" holds at each image's own step and weight.  ``itinf`` = dict(steps, ..., target_bpp=b | [b_i]):
        the steps are chosen from the ENCODER's latents exactly as ``compress(x, target_bpp=b)`` chooses them, refinement runs at
        those steps, a candidate is eligible only while its bits + the flushed lane states fit the image's budget (where no step
        fits, the candidate with the fewest bits wins), and the steps are NOT chosen again after refinement -- a refined image may
        leave room in its budget that a finer step would have used.  The report then adds quant_step, lam, and with
        ``target_bpp`` budget_bits, met.
        ``step_offsets`` (integers [n, h, w], (h, w) = ``step_offsets_shape(H, W)``, each in [-64, 64]): region-of-interest coding.
        The ladder index of latent position p of image i is clip(step_i + step_offsets[i, p], STEP_MIN, STEP_MAX), shared by
        the position's channels, with step_i the image's ``step`` (default 0) or the index ``target_bpp`` chooses (the report
        then adds map_bits, the 24 bits per run of the map counted in the prediction).  A map that varies inside an image is
        written as wire format 7; a constant one is the file of ``step=`` those indexes and all zeros the file of
        ``compress(x)``, byte for byte.  ``entropy_coding.roi_offsets`` makes offsets from a pixel mask.  Excludes ``itinf`` at
        the top level: refinement ON a map travels inside the dict, as ``step`` does.
        ``itinf`` = dict(steps, ..., step=k | [k_i] | target_bpp=b | [b_i], step_offsets=off): SGA on the map
        K_i[p] = clip(step_i + off[i, p]) -- every position is sampled on its own grid and priced under its own table, and the
        distortion is the weighted MSE Dw_i = sum_pixels omega_i(pixel) (255 (x - x_hat))^2 / (H W C), omega = 1 / step_size(K_i[p])^2
        for the pixels of position p's block (for a constant map this is lambda_i D_i of the paragraph above, and
        it is the same stated modelling choice, not a measured optimum).  The candidates are judged by
        ``coded_cost(x, latents, step=ks, step_offsets=off, weighted=True)`` and the file is
        ``compress_latents(..., step=ks, step_offsets=off)``: never a worse file by that weighted J.  With ``target_bpp`` the base
        indexes are chosen once, from the encoder's latents, over the map.  All-zero offsets are ``itinf=dict(steps, ...)`` and a
        map constant per image is ``itinf=dict(steps, ..., step=those indexes)``, launch for launch and byte for byte.  The report
        adds quant_step, weighted=True, sse_blocks (the chosen candidate's, as ``coded_cost`` returns them) and, with
        ``target_bpp``, budget_bits, met, map_bits; a candidate is then eligible while its bits + the flushed lane states + map_bits
        fit the budget.  MSE only (``distortion="ms_ssim"``
        with a map: NotImplementedError); ``rd_lambda`` with a map: ValueError -- a weight per image and a weight per position are
        not both defined.
        ``target_psnr`` in dB (a number, or one per image): the smallest file that still decodes to at least that PSNR -- per
        image the step of the whole ladder with the fewest predicted bits among those whose decoded uint8 pixels have an integer
        SSE <= 255^2 3 H W / 10^(target / 10), STEP_MIN (met = False) where none has.  The decoded SSE of all 65 steps comes
        from ``rd_curve``'s passes (the candidates decoded as batches, exactly ``coded_cost``'s sse), the bits are those
        ``target_bpp`` compares; the file is that of ``step=`` the chosen indexes, byte for byte (with ``step_offsets`` the
        candidates are bases of the map and map_bits is counted, as for ``target_bpp``).  ``last_compress_report`` lists
        step_chosen, bits_predicted, sse_predicted, psnr_predicted, sse_budget, met.  Excludes ``step``, ``target_bpp`` and
        ``itinf``; inside the ``itinf`` dict it is not implemented.
        ``max_error`` (an int, 0 .. 127): a hard bound on every decoded pixel -- the file of the other arguments, whatever they
        are (``itinf`` included), wrapped in a coded residual layer (wire format 8, ``add_residual``): ``decompress`` then gives
        pixels within max_error of x quantised to uint8, that picture itself at 0.  Byte for byte
        ``add_residual(compress(x, ...), x, max_error)``.  ``last_compress_report`` gains, per image, max_error,
        residual_bits_predicted and residual_tables (a plain ``compress(x, max_error=d)`` reports just these).  Mean-scale
        hyperprior models in precision 'fp32' only.
        ``rdoq`` (True, or dict(strength=1.0, zero=True, gains=None)): rate-distortion optimised quantisation -- one streaming
        pass over the latents (csrc/rdoq.hip) between "round to nearest" and SGA refinement.  Per element whose nearest integer
        s0 is not 0 the symbol is the candidate among s0, s0 - sign(s0) and (``zero``) 0 with the smallest
        w_c (u - s)^2 + cost_q(s): cost_q the exact integer price of the symbol under the element's own table, u = (y - mu) /
        step, w_c = strength 65536 lambda g_c / 3 with lambda the scheduled rd_lambda and g_c = ``gains`` (default
        ``latent_gains()``: what a unit change of channel c does to the SSE of the pixels, a linearisation -- a modelling choice,
        not a measured optimum).  The weight does not depend on the step: image i is judged with lambda_i = lambda /
        step_size(k_i)^2 as ``itinf`` at a step judges (on a step map: the weighted D_w of ``coded_cost(weighted=True)``).  The
        guard is ``itinf``'s: one analysis and one hyper-synthesis, then the plain and the RDOQ candidate go through the exact
        coded cost (``coded_cost``: bits of the coder's tables, integer SSE of the decoded pixels), and image i is coded with
        RDOQ only where J_rdoq < J_plain -- never a worse file, by J, than without it, per image.  The file is ordinary wire
        format 3 / 5 / 7.  ``last_compress_report``: per image rdoq_used, changed (the RDOQ candidate's symbols that are not the
        nearest integer), bits_plain, bits_rdoq, sse_plain, sse_rdoq, J_plain, J_rdoq, J_chosen, lam, quant_step.  Combines
        with ``step``, ``step_offsets`` and ``max_error``; excludes ``itinf``, ``target_bpp`` and ``target_psnr`` (ValueError: the
        ladder kernels price nearest-integer symbols).  Mean-scale hyperprior models in precision 'fp32' with MSE only
        (NotImplementedError).
        ``tile`` = T (a multiple of ``downsample_factor``, T >= 64) with ``overlap`` = O (0 <= O <= T / 4, default 16): a TILED
        file, wire format 9 (entropy_coding.Codec.compress_tiled, DESIGN.md 4.7 "tiled files").  The picture is cut into tiles
        whose cores are T x T (the last of an axis runs to the edge: T .. 2 T - 1) and whose extents reach O pixels into their
        neighbours; the tiles are coded independently, as the images of ordinary batches, and ``decompress`` blends them across
        the 2 O-wide seams with integer weights.  ``decompress(blob, region=(y0, x0, h, w))`` then decodes only the tiles the
        window meets and returns exactly that window of the full decode; ``tile_index(blob)`` lists the tiles.  Only ``step`` (an
        int, or one per image, applied to all of that image's tiles) may accompany ``tile``: ``itinf``, ``target_bpp``,
        ``target_psnr``, ``step_offsets``, ``max_error`` and ``rdoq`` are a ValueError before anything is enqueued, and a
        factorized-prior model refuses ``tile`` (NotImplementedError).  Without ``tile`` nothing changes: the file of today,
        byte for byte."""
        if tile is not None:
            if self.factorized:
                raise NotImplementedError("compress(tile): tiled files hold wire format 3 / 5 inner blobs; mean-scale hyperprior models only")
            from .. import tiling
            tiling.refuse_with_tile(itinf=itinf, target_bpp=target_bpp, target_psnr=target_psnr, step_offsets=step_offsets,
                                    max_error=max_error, rdoq=rdoq)
            tiling.check_tiling(tile, overlap, self.downsample_factor)
            if step is not None:
                self._check_step_arguments("compress", step)
            return self._get_codec().compress(x, step=step, tile=tile, overlap=overlap)
        if max_error is not None:
            self._check_residual_arguments("compress", max_error)
        self._check_step_arguments("compress", step, target_bpp, itinf, step_offsets, target_psnr=target_psnr)
        cfg = None if rdoq is None else self._check_rdoq_arguments("compress", rdoq, itinf, target_bpp, target_psnr)
        if cfg is not None:
            blob = self._compress_rdoq(x, cfg, step, step_offsets)
        elif itinf is not None:
            if "target_psnr" in itinf:
                raise ValueError("compress: target_psnr is not implemented inside itinf")
            blob = self._compress_itinf(x, **itinf)
        elif step is None and target_bpp is None and step_offsets is None and target_psnr is None:
            blob = self._get_codec().compress(x)
        else:
            codec = self._get_codec()
            blob = codec.compress(x, step=step, target_bpp=target_bpp, step_offsets=step_offsets, target_psnr=target_psnr)
            if target_bpp is not None or target_psnr is not None:
                self.last_compress_report = codec.last_report
        if max_error is None:
            return blob
        reported = itinf is not None or target_bpp is not None or target_psnr is not None or cfg is not None
        return self._add_residual(blob, x, max_error, self.last_compress_report if reported else None)

    def _check_rdoq_arguments(self, where, rdoq, itinf=None, target_bpp=None, target_psnr=None):
        """The refusals of ``rdoq`` that need no image, every one before any launch: -> None (off), or the checked
        dict(strength, zero, gains) -- gains float64 [c], or None for ``latent_gains()``."""
        if rdoq is None or rdoq is False:
            return None
        if self.factorized:
            raise NotImplementedError(f"{where}(rdoq): the symbols are priced with the scale ladder's normal tables; mean-scale "
                                      "hyperprior models only, not a factorized-prior model")
        if itinf is not None or target_bpp is not None or target_psnr is not None:
            raise ValueError(f"{where}: rdoq excludes itinf, target_bpp and target_psnr (the ladder kernels price nearest-integer symbols)")
        require_fp32(self._precision, f"{where}(rdoq)")
        if self._distortion == "ms_ssim":
            raise NotImplementedError(f"{where}(rdoq): the weights are those of a squared pixel error, not distortion='ms_ssim'")
        if rdoq is True:
            rdoq = {}
        if not isinstance(rdoq, dict) or set(rdoq) - {"strength", "zero", "gains"}:
            raise ValueError(f"{where}: rdoq is True or dict(strength=1.0, zero=True, gains=None), not {rdoq!r}")
        cfg = dict(strength=rdoq.get("strength", 1.0), zero=bool(rdoq.get("zero", True)), gains=rdoq.get("gains"))
        from ..entropy_coding import rdoq_weights
        c = self._bottleneck_size
        try:
            gains = None if cfg["gains"] is None else np.asarray(cfg["gains"], np.float64)
            cfg["strength"] = float(cfg["strength"])
        except (TypeError, ValueError):
            raise ValueError(f"{where}: rdoq strength a number, gains {c} numbers") from None
        if gains is not None and gains.shape != (c,):
            raise ValueError(f"{where}: rdoq gains must hold one number per latent channel ({c}), not shape {gains.shape}")
        rdoq_weights(1.0, np.zeros(c) if gains is None else gains, cfg["strength"])      # its checks: strength, the gains' values
        cfg["gains"] = gains
        return cfg

    def _rdoq_tool(self, cfg, n):
        """The checked dict of ``rdoq`` -> the ``entropy_coding.Rdoq`` of n images, every image enabled."""
        from ..entropy_coding import rdoq_weights
        gains = self.latent_gains() if cfg["gains"] is None else cfg["gains"]
        weight = rdoq_weights(float(self._scheduled_rd_lambda), gains, cfg["strength"])
        return self._get_codec().rdoq(weight, n, zero=cfg["zero"])

    def latent_gains(self):
        """What a unit change of one latent channel does to the squared error of the pixels: float64 [c], cached per set of
        weights.  g_c = sum over pixels and colours of (255 (syn(e_c) - syn(0)))^2 on the synthesis' float output, before any
        uint8 rounding, e_c a unit impulse in channel c at the centre of a 9 x 9 grid of zero latents; the c impulses and the
        zero grid run as ONE decoder batch of c + 1 latents.  The response must be exactly zero over the outermost ring of
        latent positions -- the impulse response then lies wholly inside the grid -- else RuntimeError.
        A linearisation of the synthesis AT ZERO LATENTS with the cross terms between channels and positions ignored: a stated
        modelling choice for the weights of ``compress(x, rdoq=...)``, not a measured optimum."""
        if getattr(self, "_latent_gains", None) is None:
            c, side = self._bottleneck_size, 9
            y = np.zeros((c + 1, side, side, c), np.float32)
            y[np.arange(c), side // 2, side // 2, np.arange(c)] = 1.0
            with torch.cuda.device(self.device):
                out = self._synthesis(ops.to_device(y, self.device)).cpu().numpy().astype(np.float64)
                ops.check_conv_status()
            if out.shape[1] % side or out.shape[2] % side:
                raise RuntimeError(f"latent_gains: a {out.shape[1]} x {out.shape[2]} picture from {side} x {side} latent positions")
            d = 255.0 * (out[:c] - out[c:])
            bh, bw = out.shape[1] // side, out.shape[2] // side
            ring = d.copy()
            ring[:, bh:-bh, bw:-bw] = 0.0
            if np.any(ring != 0.0):
                raise RuntimeError("latent_gains: the synthesis' impulse response reaches the outermost ring of a 9 x 9 latent grid; "
                                   "the gains would be truncated")
            self._latent_gains = (d * d).reshape(c, -1).sum(axis=1)
        return self._latent_gains.copy()

    def _compress_rdoq(self, x, cfg, step, step_offsets):
        """``compress(x, rdoq=...)``: the plain and the RDOQ candidate judged by exact coded cost, the file coded with RDOQ on
        the images it wins."""
        x = self._as_device_images(x)
        n, H, W = x.shape[0], int(x.shape[1]), int(x.shape[2])
        codec = self._get_codec()
        grid = codec._grid(step, step_offsets, n, H, W)                  # ValueError before any launch
        lam = float(self._scheduled_rd_lambda)
        if grid.kind == "map":                                           # the weight sits on every position's pixels (D_w)
            from ..entropy_coding import check_steps
            ks, lams = check_steps(0 if step is None else step, n), np.full(n, lam)
            cost_kw = dict(step=step, step_offsets=step_offsets, weighted=True, lam=None)
        else:
            ks = grid.steps or [0] * n
            lams = step_lambdas(lam, ks)
            cost_kw = dict(step=ks if any(ks) else None, step_offsets=None, weighted=False, lam=lams)
        tool = self._rdoq_tool(cfg, n)
        with torch.cuda.device(self.device):
            lat = self.infer_latent_rvs(x)
            z, y = lat.uq[0].loc.contiguous(), lat.uq[1].loc.contiguous()
            pre = codec._hyper_of(z)
            plain = self._coded_cost(x, lat, pre=pre, **cost_kw)
            cand = self._coded_cost(x, lat, rdoq=tool, pre=pre, **cost_kw)
            used = cand["J"] < plain["J"]                                # strictly better only: the nearest integers win a tie
            tool.set_enable([int(u) for u in used])
            blob = codec._finish([codec._launch_latents(z, y, (H, W), grid, pre, rdoq=tool if used.any() else None)])[0]
        pick = lambda key, i: float((cand if used[i] else plain)[key][i])
        self.last_compress_report = [
            dict(rdoq_used=bool(used[i]), changed=int(cand["changed"][i]), bits_plain=float(plain["bits"][i]),
                 bits_rdoq=float(cand["bits"][i]), sse_plain=float(plain["sse"][i]), sse_rdoq=float(cand["sse"][i]),
                 J_plain=float(plain["J"][i]), J_rdoq=float(cand["J"][i]), J_chosen=pick("J", i), bits_chosen=pick("bits", i),
                 sse_chosen=pick("sse", i), lam=float(lams[i]), quant_step=int(ks[i])) for i in range(n)]
        return blob

    def _check_residual_arguments(self, where, max_error):
        """The refusals of the residual layer that need no image: every one before any launch."""
        from ..entropy_coding import check_max_error
        if self.factorized:
            raise NotImplementedError(f"{where}(max_error): the residual layer codes with the scale ladder's normal tables; mean-scale "
                                      "hyperprior models only")
        for d in (max_error if isinstance(max_error, (list, tuple, np.ndarray)) else [max_error]):
            check_max_error(d)
        require_fp32(self._precision, f"{where}(max_error)")

    def _add_residual(self, blob, x, max_error, report):
        codec = self._get_codec()
        out = codec.add_residual(blob, x, max_error)
        last = codec.last_residual
        rows = [dict() for _ in last["cost_q"]] if report is None else report
        for i, r in enumerate(rows):
            r.update(max_error=last["max_error"], residual_bits_predicted=float(last["bits_predicted"][i]),
                     residual_tables=[int(t) for t in last["choice"][i]])
        self.last_compress_report = rows
        return out

    def add_residual(self, blob: bytes, x, max_error) -> bytes:
        """A v3 / v5 / v7 bitstream of this model and the images it was made from -> the same file wrapped in a coded residual
        layer (wire format 8; entropy_coding.Codec.add_residual, DESIGN.md 4.7 "residual layer"): every decoded pixel is then
        within ``max_error`` (0 .. 127; 0: lossless) of x quantised to uint8.  A blob that already carries a layer is a
        ValueError: ``entropy_coding.split_residual(blob)[0]`` is its base file.  ``last_compress_report``: per image max_error,
        residual_bits_predicted, residual_tables."""
        self._check_residual_arguments("add_residual", max_error)
        return self._add_residual(blob, x, max_error, None)

    def residual_bits(self, x, blob: bytes, max_error):
        """What the residual layer over ``blob`` would cost per image at ``max_error`` (an int -> float64 [n]; a list of ints ->
        [n, len]), without coding anything: the exact coded cost of the tables ``add_residual`` would choose + 32 bits per
        flushed lane state (entropy_coding.Codec.residual_bits)."""
        self._check_residual_arguments("residual_bits", max_error)
        return self._get_codec().residual_bits(x, blob, max_error)

    def rd_curve(self, x, steps=None, step_offsets=None):
        """The exact rate-distortion ladder of these images: what every ladder index of ``steps`` (None: the whole ladder,
        STEP_MIN .. STEP_MAX) would cost in the file and decode to, from ONE encoder pass, the ladder-cost launches, the
        candidates decoded as batches (``Codec.ladder_distortion``) and one read-back -- not one ``coded_cost`` per step.
        -> dict(steps, bits [n, S] = ``coded_cost(x, step=steps[j], step_offsets=...)["bits"]`` + the flushed lane states (what
        ``target_bpp`` compares), bpp = bits / (H W), sse [n, S] int64 = ``coded_cost``'s, exactly, psnr of it in dB,
        bits_z [n], flushed_bits; with ``step_offsets`` also map_bits [n], the map's records, NOT in bits).
        Mean-scale hyperprior models in precision 'fp32' only."""
        from ..entropy_coding import COST_UNIT, MAP_RECORD_BITS, STEP_MAX, STEP_MIN, check_offsets, check_steps, count_runs, psnr_of_sse
        self._check_step_arguments("rd_curve", 0, step_offsets=step_offsets)
        steps = list(range(STEP_MIN, STEP_MAX + 1)) if steps is None else list(steps)
        steps = check_steps(steps, len(steps))
        if not steps:
            raise ValueError("rd_curve: no candidate step")
        x = self._as_device_images(x)
        n, H, W = x.shape[0], int(x.shape[1]), int(x.shape[2])
        codec = self._get_codec()
        offsets = None if step_offsets is None else check_offsets(step_offsets, n, *codec.latent_shapes(H, W)[4:])
        with torch.cuda.device(self.device):
            lat = self.infer_latent_rvs(x)
            z, y = lat.uq[0].loc.contiguous(), lat.uq[1].loc.contiguous()
            cost_z, cost_y, sse, _ = codec.rd_ladder(z, y, x, steps, offsets)
        flushed = float(codec.flushed_bits(H, W))
        bits = (cost_z[:, None] / float(COST_UNIT) + cost_y / float(COST_UNIT)) + flushed
        out = dict(steps=steps, bits=bits, bpp=bits / float(H * W), sse=sse, psnr=psnr_of_sse(sse, 3 * H * W),
                   bits_z=cost_z / float(COST_UNIT), flushed_bits=flushed)
        if offsets is not None:
            out["map_bits"] = (MAP_RECORD_BITS * count_runs(offsets)).astype(np.float64)
        return out

    def _check_step_arguments(self, where, step, target_bpp=None, itinf=None, step_offsets=None, target_psnr=None):
        """The refusals of the quantisation-step arguments that need no image: every one before any launch."""
        if step is None and target_bpp is None and step_offsets is None and target_psnr is None:
            return
        if self.factorized:
            raise NotImplementedError(f"{where}(step / target_bpp / step_offsets): a factorized-prior model's per-channel tables "
                                      "would have to be rebuilt per step; mean-scale hyperprior models only")
        if step is not None and target_bpp is not None:
            raise ValueError(f"{where}: step and target_bpp exclude each other")
        if target_psnr is not None and (step is not None or target_bpp is not None):
            raise ValueError(f"{where}: target_psnr excludes step and target_bpp")
        if itinf is not None:
            raise ValueError(f"{where}: step / target_bpp / step_offsets and itinf exclude each other at the top level (they travel "
                             "inside the itinf dict)")
        require_fp32(self._precision, f"{where}(step / target_bpp / step_offsets)")

    def step_offsets_shape(self, H, W):
        """(h, w) of ``step_offsets`` for H x W images: the resolution of the latents y (``Codec.latent_shapes``)."""
        if self.factorized:
            raise NotImplementedError("step_offsets_shape: a factorized-prior model takes no step_offsets; mean-scale hyperprior models only")
        return tuple(int(v) for v in self._get_codec().latent_shapes(int(H), int(W))[4:])

    def coded_cost(self, x, latent_rvs=None, step=None, lam=None, step_offsets=None, weighted=False, rdoq=None):
        """Per image, the cost of what ``decompress`` will output for ``latent_rvs`` (None: the encoder's latents of x) coded at
        ``step`` (None: step 1; a ladder index or one per image as in ``compress``), without
        writing a file: dict of float64 arrays [n] -- ``bits_z`` / ``bits_y`` = ``entropy_coding.rans_cost`` of the symbols the
        file would carry (the coder's 16-bit integer tables, ESCAPE + 16 raw bits; the flushed lane states and the coder's
        rounding slack, DESIGN.md 4.7, are not in it), ``bits`` their sum, ``sse`` the integer SSE of the decoded uint8 pixels,
        ``D`` = the MSE of those pixels on the 0-255 scale (``distortion="ms_ssim"``: 1 - (MS-)SSIM of them, and ``msssim``),
        ``J`` = bits / (H W) + ``lam`` * D with ``lam`` the scheduled rd_lambda (``lam`` given: one weight per image instead, as
        ``compress(x, itinf=dict(step=...))`` judges its candidates).  ``step_offsets``: as in ``compress``.  One host read-back.
        ``weighted`` (False: the result above, key for key; True needs ``step`` and / or ``step_offsets``, MSE, and no ``lam``):
        the cost on the map K_i[p] = clip(step_i + step_offsets[i, p]) as ``compress(x, itinf=dict(step_offsets=...))`` judges its
        candidates.  Adds ``sse_blocks`` [n, hb, wb] = the integer squared error of the decoded pixels per B x B pixel block
        (``ops.block_sse``; B pixels per latent position, hb = ceil(H / B); same read-back),
        ``D_w`` = sum_p omega_i(p) sse_blocks[i, p] / (H W C) with omega = ``entropy_coding.position_weights`` (float64, on the
        host), and ``J`` = bits / (H W) + lambda D_w with the scheduled rd_lambda.
        ``sse_blocks`` is also a region-of-interest metric.  The PSNR of the decoded pixels inside a block mask (bool [hb, wb],
        e.g. ``step_offsets[i, :hb, :wb] == inside``; edge blocks hold fewer pixels, so count them):
            rows = np.minimum(B, H - B * np.arange(hb))[:, None]; cols = np.minimum(B, W - B * np.arange(wb))[None, :]
            mse = sse_blocks[i][mask].sum() / (3.0 * (rows * cols)[mask].sum()); psnr = 10 * np.log10(255.0 ** 2 / mse)
        ``rdoq`` (True or dict(strength=1.0, zero=True, gains=None), as in ``compress``): the cost of the RDOQ candidate -- every
        image quantised by rate + weighted squared error (csrc/rdoq.hip) with the weights ``compress`` would use -- plus
        ``changed`` int64 [n], the symbols per image that are not the nearest integer (same read-back)."""
        cfg = None if rdoq is None else self._check_rdoq_arguments("coded_cost", rdoq)
        return self._coded_cost(x, latent_rvs, step, lam, step_offsets, weighted, cfg)

    def _coded_cost(self, x, latent_rvs, step, lam, step_offsets, weighted, rdoq=None, pre=None):
        """``coded_cost``; ``rdoq``: the checked dict of it or a ready ``entropy_coding.Rdoq``, ``pre``: ``Codec._hyper_of`` of
        the latents' z if the caller has it."""
        self._check_step_arguments("coded_cost", step, step_offsets=step_offsets)
        if weighted:                                                  # every refusal before any launch
            if step is None and step_offsets is None:
                raise ValueError("coded_cost(weighted=True) needs step and / or step_offsets: the weights are those of a step map")
            if self._distortion == "ms_ssim":
                raise NotImplementedError("coded_cost(weighted=True): the weighted distortion is MSE, not distortion='ms_ssim'")
            if lam is not None:
                raise ValueError("coded_cost(weighted=True): lam (a weight per image) and a weight per position are not both defined")
        x = self._as_device_images(x)
        n, h, w, c = x.shape
        ssim = self._distortion == "ms_ssim"
        if ssim:
            ops.msssim_scale_sizes(h, w)                              # ValueError before any launch
        codec = self._get_codec()
        kw = {}
        if step is not None or step_offsets is not None:
            kw = dict(step=step, step_offsets=step_offsets)
            grid = codec._grid(step, step_offsets, n, h, w)           # ValueError before any launch
        if weighted:
            block = self._position_block(h, w)
            omega = grid.position_weights(*codec.latent_shapes(h, w)[4:])
        if isinstance(rdoq, dict):
            rdoq = self._rdoq_tool(rdoq, n)
        if rdoq is not None:
            kw = dict(kw, rdoq=rdoq)
        if pre is not None:
            kw = dict(kw, pre=pre)
        with torch.cuda.device(self.device):
            if latent_rvs is None:
                latent_rvs = self.infer_latent_rvs(x)
            cost_z, cost_y, px, sse = codec.latents_cost(*[rv.loc for rv in latent_rvs.uq], x, **kw)
            rows = [torch.zeros_like(cost_y) if cost_z is None else cost_z, cost_y, sse]
            if rdoq is not None:
                rows.append(rdoq.changed.to(cost_y.dtype))
            at = len(rows) * n                                        # where the per-image rows end
            parts = [torch.stack(rows).to(torch.float64).flatten()]   # integers below 2^53: exact
            if weighted:                                              # uint32 -> float64 through int64: exact
                blocks = ops.block_sse(x, px, block)
                parts.append((blocks.view(torch.int32).to(torch.int64) & 0xFFFFFFFF).to(torch.float64).flatten())
            if ssim:
                sums, counts, single = ops.image_quality_launch(ops.pixels_float(x, h, w), px.to(torch.float32), 255.0)
                parts.append(sums.flatten())
            host = torch.cat(parts).cpu().numpy()
            ops.check_conv_status()
        out = dict(bits_z=host[:n] / 65536.0, bits_y=host[n:2 * n] / 65536.0, sse=host[2 * n:3 * n], lam=float(self._scheduled_rd_lambda))
        if lam is not None:
            out["lam"] = step_lambdas(1.0, [0] * n, lam)                   # the checks of rd_lambda: positive, finite, one per image
        if rdoq is not None:
            out["changed"] = np.rint(host[3 * n:4 * n]).astype(np.int64)
        out["bits"] = out["bits_z"] + out["bits_y"]
        out["D"] = out["sse"] / float(h * w * c)
        if ssim:
            out["msssim"] = ops.image_quality_finish(host[at:].reshape(tuple(sums.shape)), counts, single)
            out["D"] = 1.0 - out["msssim"]
        out["J"] = out["bits"] / float(h * w) + out["lam"] * out["D"]
        if weighted:
            out["sse_blocks"] = np.rint(host[at:]).astype(np.int64).reshape(tuple(blocks.shape))
            out["D_w"] = weighted_distortion(out["sse_blocks"], omega, h * w * c)
            out["J"] = out["bits"] / float(h * w) + out["lam"] * out["D_w"]
        return out

    def _position_block(self, H, W):
        """B: the pixels per latent position along each side, the padded image size over the latent size
        (``Codec.latent_shapes``; 16 for the shipped configs).  ValueError where that division is not exact."""
        f = self.downsample_factor
        hp, wp = -(-int(H) // f) * f, -(-int(W) // f) * f
        lh, lw = self._get_codec().latent_shapes(int(H), int(W))[4:]
        if hp % lh or wp % lw or hp // lh != wp // lw:
            raise ValueError(f"a {hp} x {wp} padded image over {lh} x {lw} latent positions: no whole, square pixel block per position")
        return hp // lh

    def _compress_itinf(self, x, steps, seed=0, check_every=None, step=None, rd_lambda=None, target_bpp=None, step_offsets=None):
        if self._latent_config["uq"].get("method", "unoise") != "sga":       # every refusal before any launch
            raise NotImplementedError("itinf_train_step implements latent_config uq.method == 'sga'")
        require_fp32(self._precision, "compress(itinf=...)")
        steps = int(steps)
        if steps < 0 or (check_every is not None and int(check_every) < 1):
            raise ValueError("compress(itinf=...): steps >= 0, check_every None or >= 1")
        stepped = step_offsets is not None or step is not None or target_bpp is not None or rd_lambda is not None
        shape = tuple(x.shape)
        n = 1 if len(shape) == 3 else int(shape[0])
        budgets = q = None
        if stepped:
            from ..entropy_coding import check_budgets
            q = self._itinf_grid_of(shape, step, rd_lambda, step_offsets, target_bpp)
            if target_bpp is not None:
                budgets = check_budgets(target_bpp, n)
        x = self._as_device_images(x)
        if self._distortion == "ms_ssim":
            ops.msssim_scale_sizes(x.shape[1], x.shape[2])
        codec = self._get_codec()
        mapped = False
        if not stepped:
            self.initialize_itinf(x)
            cost_kw = lat_kw = {}
            flushed = 0.0
        else:
            H, W = int(x.shape[1]), int(x.shape[2])
            flushed = float(codec.flushed_bits(H, W))
            self.initialize_itinf(x)
            control = None
            if budgets is not None:             # the steps of compress(x, target_bpp=b): chosen from the encoder's latents, once
                budgets = budgets * float(H * W)
                offs = None if q is None else q["offsets"]
                offs = offs if offs is not None and offs.any() else None      # all zero: today's rate control
                with torch.cuda.device(self.device):
                    control = codec._rate_control(*[rv.loc.contiguous() for rv in self.latent_rvs.uq], H, W, budgets, offs)[0]
                q = self._itinf_grid_of(shape, [r["step_chosen"] for r in control], rd_lambda, step_offsets)
            self._set_itinf_grid(q)
            mapped = q is not None and q["grid"].kind == "map"      # only a map that varies inside an image is a map
            if mapped:
                ks = q["steps"]
                lat_kw = dict(step=ks, step_offsets=q["offsets"])
                cost_kw = dict(lat_kw, weighted=True)                         # J with the weight on every position's pixels
            else:
                ks = [0] * n if q is None else q["grid"].steps
                lams = step_lambdas(self._rd_lambda, ks, rd_lambda)
                lat_kw = dict(step=ks) if any(ks) else {}
                cost_kw = dict(lat_kw, lam=lams)                              # J at each image's own step and weight

        def cost_of(latents):
            return self.coded_cost(x, latents, **cost_kw)

        with torch.cuda.device(self.device):
            start = cost_of(self.latent_rvs)
            best = [rv.loc.clone() for rv in self.latent_rvs.uq]
            j_best, bits_best, step_best = start["J"].copy(), start["bits"].copy(), np.zeros(n, np.int64)
            blocks_best = start["sse_blocks"].copy() if mapped else None
            met = None if budgets is None else np.array([r["met"] for r in control], bool)
            room = budgets                      # what a candidate's bits + flushed states may reach: the budget less the map's records
            if budgets is not None and "map_bits" in control[0]:
                room = budgets - np.array([r["map_bits"] for r in control], np.float64)
            for done in range(1, steps + 1):
                self.itinf_train_step(x, seed=seed, fetch=False)
                if done != steps and (check_every is None or done % int(check_every)):
                    continue
                cand = cost_of(self.latent_rvs)
                # strictly better only: the encoder's latents win a tie
                for i in np.nonzero(candidate_wins(cand["J"], cand["bits"], j_best, bits_best, room, flushed, met))[0]:
                    for keep, rv in zip(best, self.latent_rvs.uq):
                        keep[i].copy_(rv.loc[i])
                    j_best[i], bits_best[i], step_best[i] = cand["J"][i], cand["bits"][i], done
                    if blocks_best is not None:
                        blocks_best[i] = cand["sse_blocks"][i]
            blob = codec.compress_latents(*best, x.shape[1:3], **lat_kw)
        self.last_compress_latents = LatentRVCollection(uq=tuple(UQLatentRV(t) for t in best))
        self.last_compress_report = [dict(step_chosen=int(step_best[i]), J_start=float(start["J"][i]), J_chosen=float(j_best[i]),
                                          bits_start=float(start["bits"][i]), bits_chosen=float(bits_best[i])) for i in range(n)]
        if stepped:
            for i, r in enumerate(self.last_compress_report):
                if mapped:
                    r.update(quant_step=int(ks[i]), weighted=True, sse_blocks=blocks_best[i].copy())
                else:
                    r.update(quant_step=int(ks[i]), lam=float(lams[i]))
                if budgets is not None:
                    r.update(budget_bits=float(budgets[i]), met=bool(met[i]))
                    if "map_bits" in control[i]:
                        r.update(map_bits=float(control[i]["map_bits"]))
        return blob

    def compress_many(self, xs):
        """Several batches (e.g. one per image size of a set) -> their bitstreams; the batches' launches run side by side and
        the set costs two host synchronisations (entropy_coding.Codec.compress_many).  Same bytes as one ``compress`` per batch."""
        return self._get_codec().compress_many(list(xs))

    def decompress(self, blob: bytes, region=None):
        """Bitstream -> uint8 pixels [n, H, W, 3]; bit-identical to ``decode(encode(x))``.  A tiled file (wire format 9,
        ``compress(x, tile=...)``) decodes to its tiles blended across their seams.  ``region`` = (y0, x0, h, w), tiled files
        only: -> uint8 [n, h, w, 3], exactly that window of the full decode, from the tiles whose extents meet it alone -- the
        other inner blobs are never uploaded; ValueError on an untiled file or a window that leaves the picture.
        ``last_decompress_report``: dict(tiles_total, tiles_decoded, bytes_total, bytes_read) after a tiled file, None after
        any other."""
        codec = self._get_codec()
        self.last_decompress_report = None
        if region is None:
            out = codec.decompress(blob)
        elif self.factorized:
            raise ValueError("decompress: region needs a tiled file; a factorized-prior model writes none")
        else:
            out = codec.decompress(blob, region=region)
        self.last_decompress_report = getattr(codec, "last_decompress_report", None)
        return out

    def tile_index(self, blob: bytes):
        """The grid of a tiled file and, per tile, its extent, inner blob and index within it (``tiling.tile_index``); host only."""
        from ..tiling import tile_index
        return tile_index(blob)

    def decompress_many(self, blobs):
        """Several bitstreams -> their pixel batches; the entropy-decoding launches of all of them run side by side
        (entropy_coding.Codec.decompress_many).  Same pixels as one ``decompress`` per blob.  Tiled files (wire format 9) may be
        mixed in freely; ``last_decompress_report`` is then a LIST with one dict(tiles_total, tiles_decoded, bytes_total,
        bytes_read) per tiled file of the call, in order, and None where the call held none."""
        codec = self._get_codec()
        self.last_decompress_report = None
        out = codec.decompress_many(list(blobs))
        self.last_decompress_report = getattr(codec, "last_decompress_report", None)
        return out

    def transcode(self, blob: bytes, shift=None, target_bpp=None) -> bytes:
        """A bitstream of this model -> the bitstream of a coarser quantisation step, from the file alone: no pixels, no analysis,
        no synthesis (entropy_coding.Codec.transcode_many, DESIGN.md 4.7 "transcode").  ``shift`` = d (an int, or one per image,
        0 <= d <= STEP_MAX - STEP_MIN): every latent position moves from its ladder index k0 to clip(k0 + d, STEP_MIN, STEP_MAX);
        the file's integers are dequantised as ``decompress`` would and requantised with the coarser step, the z stream is
        copied.  The result is ``compress_latents(z_hat, y_hat0, (H, W), ...)`` of the source's decoded latents at the new
        indexes, byte for byte, in wire format 3, 5 or 7.  It is NOT the file of ``compress(x, step=k0 + d)``: the second
        rounding starts from y_hat0, not from y (DESIGN.md 4.7 has the measured price).  A negative shift is a ValueError: the
        finer symbols are not in the file.  ``target_bpp`` (a number, or one per image): per image the smallest d whose exact
        coded cost fits target_bpp H W, counted as ``compress(target_bpp=)`` counts; ``last_compress_report`` lists step_chosen
        (= d), bits_predicted, budget_bits, met[, map_bits].  Exactly one of the two.  Mean-scale hyperprior models in precision
        'fp32' only."""
        self._check_transcode_arguments(shift, target_bpp)
        codec = self._get_codec()
        out = codec.transcode(blob, shift=shift, target_bpp=target_bpp)
        if target_bpp is not None:
            self.last_compress_report = codec.last_report[0]
        return out

    def transcode_many(self, blobs, shift=None, target_bpp=None):
        """``transcode`` for several bitstreams -> theirs, in order, byte for byte what one ``transcode`` per blob returns; the
        blobs' entropy-decoding launches run side by side as in ``decompress_many``.  ``shift`` / ``target_bpp``: one value for
        every blob, or a sequence with one entry per blob (each a value, or one per image of that blob).  With ``target_bpp``
        ``last_compress_report`` holds one report per blob."""
        self._check_transcode_arguments(shift, target_bpp)
        codec = self._get_codec()
        out = codec.transcode_many(list(blobs), shift=shift, target_bpp=target_bpp)
        if target_bpp is not None and out:
            self.last_compress_report = codec.last_report
        return out

    def _check_transcode_arguments(self, shift, target_bpp):
        """The refusals of ``transcode`` that need no bitstream; the per-image checks follow the header parse, before any launch."""
        if (shift is None) == (target_bpp is None):
            raise ValueError("transcode: exactly one of shift and target_bpp")
        if self.factorized:
            raise NotImplementedError("transcode: a factorized-prior model's per-channel tables would have to be rebuilt per step; "
                                      "mean-scale hyperprior models only")
        require_fp32(self._precision, "transcode(shift / target_bpp)")

        def walk(v):                          # every shift, whatever the nesting per blob / per image: an int in range
            if isinstance(v, (list, tuple, np.ndarray)):
                for u in v:
                    walk(u)
            else:
                check_shifts(v, 1)
        if shift is not None:
            walk(shift)

    # -- training (reference :375-383) -----------------------------------------------------------------------
    def train_step(self, image_batch):
        """One optimizer step on ``image_batch`` (tape.gradient of end_to_end_frame_loss(training=True) + Adam,
        reference :375-383); returns Metrics with the reference's scalar keys.  The training state (flat parameter /
        gradient / moment buffers, adjoint plans) lives in ``shallow_ntc_amd.train.Trainer`` and is created on first
        use; ``self.trainer.sync_model()`` loads the trained variables back into the inference path."""
        if self._distortion != "mse":
            raise NotImplementedError("train_step optimises bpp + lambda * MSE only: distortion='ms_ssim' drives SGA iterative inference")
        if getattr(self, "trainer", None) is None:
            from ..train import Trainer
            self.trainer = Trainer(self, seed=self._seed)
        d = self.trainer.train_step(image_batch)
        metrics = Metrics.make()
        metrics.record_scalars({k: d[k] for k in ("rd_loss", "bpp", "mse", "psnr", "scheduled_lr", "sched_rd_lambda")})
        return metrics

    # -- iterative inference (reference :389-413, common/itinf_lib.py:26-93) ----------------------------
    def initialize_itinf(self, image_batch, step=None, rd_lambda=None, step_offsets=None):
        """latent_rvs = trainable copy of the encoder's latents; fresh Adam state (:389-395).
        ``step`` (a ladder index, or one per image) / ``rd_lambda`` (a number, or one per image; default
        lambda / step_size(k_i)^2): the steps that follow descend the loss at those quantisation steps,
        mean_B(bits_i) / (H W) + (1 / n) sum_i lambda_i D_i (sga.SGAEngine.loss_and_grads(grid=...)).  Every index 0
        and no ``rd_lambda``: the steps of before, launch for launch.
        ``step_offsets`` (integers [n, h, w] as in ``compress``): the steps that follow descend the loss on the map
        K_i[p] = clip(step_i + step_offsets[i, p]), mean_B(bits_i) / (H W) + (lambda / n) sum_i Dw_i with the weight
        1 / step_size(K_i[p])^2 on the pixels of position p (sga.SGAEngine.loss_and_grads(grid=...)); MSE only,
        and ``rd_lambda`` is refused with it.  All-zero offsets are the steps of before and a map constant per image those of
        ``step`` = its indexes, launch for launch; only a map that varies inside an image takes the map kernels."""
        from ..sga import SGAEngine
        if self._optimizer_config.get("global_clipnorm") is not None:
            raise NotImplementedError("gradient clipping is not used by the reference's itinf config")
        q = self._itinf_grid_of(tuple(image_batch.shape), step, rd_lambda, step_offsets)     # every refusal before any launch
        if self._distortion == "ms_ssim":                               # ValueError where the loss is not computable
            ops.msssim_scale_sizes(*tuple(image_batch.shape)[1:3])
        self.latent_rvs = self.infer_latent_rvs(image_batch).get_trainable_copy()
        self._sga = getattr(self, "_sga", None) or SGAEngine(self)
        self._adam = [dict(m=torch.zeros_like(rv.loc), v=torch.zeros_like(rv.loc)) for rv in self.latent_rvs.uq]
        self.itinf = True
        self._itinf_step = 0
        self._itinf_pending = None
        self._set_itinf_grid(q)

    def _itinf_grid_of(self, shape, step, rd_lambda, step_offsets, target_bpp=None):
        """The host half of SGA on a quantisation grid (``initialize_itinf(step=, rd_lambda=, step_offsets=)``, ``compress(itinf=
        dict(...))``): every refusal, before any launch, then ``StepGrid.resolve``'s routing.  -> None (step 1 and the model's lambda
        for every image: the kernels of before) or dict(grid, steps = the n base indexes, offsets = int8 [n, h, w] or None,
        lam = each image's lambda (None on a map), block = pixels per position (with offsets))."""
        if step is None and rd_lambda is None and step_offsets is None and target_bpp is None:
            return None
        from ..entropy_coding import check_offsets, check_steps
        if self.factorized:
            raise NotImplementedError("SGA at a quantisation step (step / rd_lambda / step_offsets): mean-scale hyperprior models only")
        require_fp32(self._precision, "SGA at a quantisation step")
        if step_offsets is not None and self._distortion == "ms_ssim":
            raise NotImplementedError("SGA on a step map descends the weighted MSE: distortion='ms_ssim' with step_offsets is not implemented")
        if step_offsets is not None and rd_lambda is not None:
            raise ValueError("rd_lambda and step_offsets exclude each other: a weight per image and a weight per position are not both defined")
        if step is not None and target_bpp is not None:
            raise ValueError("compress(itinf=...): step and target_bpp exclude each other")
        n = 1 if len(shape) == 3 else int(shape[0])
        ks = check_steps(0 if step is None else step, n)
        if step_offsets is None:                                        # a per-image lambda keeps the per-image kernels at step 0
            lams = step_lambdas(self._rd_lambda, ks, rd_lambda)         # iterative inference runs at the model's own lambda
            return dict(grid=StepGrid.image(ks), steps=ks, offsets=None, lam=lams, block=None) if any(ks) or rd_lambda is not None else None
        H, W = int(shape[-3]), int(shape[-2])
        h, w = self._get_codec().latent_shapes(H, W)[4:]
        offs = check_offsets(step_offsets, n, h, w)
        block = self._position_block(H, W)
        grid = StepGrid.resolve(ks, offs, n, h, w)
        if grid.kind == "unit":
            return None
        lams = None if grid.kind == "map" else step_lambdas(self._rd_lambda, grid.steps)
        return dict(grid=grid, steps=ks, offsets=offs, lam=lams, block=block)

    def _set_itinf_grid(self, q):
        """``q`` of ``_itinf_grid_of``: what the SGA kernels read goes up (one small upload each), with the distortion weight
        that goes with the grid -- a map: (the float32 position weights, block); else dweight = lambda_i / lambda, the distortion
        gradient being launched with the scalar lambda."""
        if q is not None:
            with torch.cuda.device(self.device):
                q["grid"].on(self.device)
                if q["grid"].kind == "map":
                    q["weight"] = (ops.to_device(q["grid"].position_weights(), self.device), int(q["block"]))
                else:
                    q["weight"] = ops.to_device(q["lam"] / float(self._rd_lambda), self.device)
        self._itinf_grid = q

    @property
    def itinf_trainable_variables(self):
        return self.latent_rvs.trainable_variables

    def itinf_train_step(self, image_batch, noise=None, seed=0, fetch=True):
        """One SGA step: loss = bpp + lambda * MSE(unrounded 0-255 floats), gradients to [z_loc, y_loc] only,
        Keras-Adam update (:397-408).  With ``distortion="ms_ssim"`` the loss is bpp + lambda * (1 - mean_B (MS-)SSIM) of the
        same floats; the metrics then add ``msssim`` / ``msssim_db`` and ``rd_loss`` follows that definition.  ``noise`` = (gumbel_z, gumbel_y) makes the step deterministic.
        ``fetch`` False: the step's three scalars stay on the device and nothing synchronises (the reference's step is a
        tf.function whose metrics are only converted where the loop logs them, common/itinf_lib.py:67-75); returns None, and
        ``itinf_last_metrics()`` fetches the most recent step's metrics when the caller wants them."""
        x = self._as_device_images(image_batch)
        cfg = self.latent_config["uq"]
        if cfg.get("method") != "sga":
            raise NotImplementedError("itinf_train_step implements latent_config uq.method == 'sga'")
        if self._distortion == "ms_ssim":                               # never a silent fall-back to MSE: refuse before any launch
            ops.msssim_scale_sizes(x.shape[1], x.shape[2])
        tau = cfg["tau"]
        lr = self._scheduled_lr
        locs = [rv.loc for rv in self.latent_rvs.uq]                     # (z_loc, y_loc); the factorized model: (y_loc,)
        q = getattr(self, "_itinf_grid", None)
        with torch.cuda.device(self.device):
            quant = {} if q is None else dict(grid=q["grid"], weight=q["weight"])
            r = self._sga.loss_and_grads(x, locs[0] if len(locs) == 2 else None, locs[-1], tau, self._scheduled_rd_lambda,
                                         step=self._itinf_step, seed=seed,
                                         noise_z=None if noise is None else noise[0],
                                         noise_y=None if noise is None else noise[-1], **quant)
            t = self._itinf_step + 1
            grads = [r["g_z"], r["g_y"]] if len(locs) == 2 else [r["g_y"]]
            for p, g, st in zip(locs, grads, self._adam):
                ops.adam_step(p, g, st["m"], st["v"], lr, t, self._optimizer_config.get("beta_1", 0.9),
                              self._optimizer_config.get("beta_2", 0.999), self._optimizer_config.get("epsilon", 1e-7))
            # the metrics depend on (step, lr, lambda, tau) of THIS step: keep them with the device scalars
            rows = [r["bits_z"], r["bits_y"], r["sse"]] + ([r["msssim"]] if "msssim" in r else []) + ([r["wsse"]] if "wsse" in r else [])
            self._itinf_pending = dict(dev=torch.stack(rows), shape=tuple(x.shape), two=len(locs) == 2,
                                       scalars=(self._scheduled_lr, self._scheduled_rd_lambda, tau),
                                       lams=None if q is None else q["lam"], weighted="wsse" in r)
        self._itinf_step += 1
        self.last_grads = tuple(grads)
        return self.itinf_last_metrics() if fetch else None

    def itinf_last_metrics(self):
        """Metrics of the most recent ``itinf_train_step`` (one device -> host copy; raises if a stream-K launch since the last
        check was flagged).  On a step map (``initialize_itinf(step_offsets=)``) rd_loss = bpp + lambda mean_i(Dw_i), the loss
        descended; mse / psnr stay unweighted and every other key is unchanged."""
        pend = getattr(self, "_itinf_pending", None)
        if pend is None:
            raise RuntimeError("no SGA step has run since initialize_itinf")
        with torch.cuda.device(self.device):
            host = pend["dev"].cpu().numpy()
            ops.check_conv_status()
        wsse = host[-1] if pend.get("weighted") else None               # the last row; (MS-)SSIM and a map exclude each other
        _, metrics = self._finish_metrics(pend["shape"], host[0] if pend["two"] else None, host[1], host[2],
                                          msssim=host[3] if len(host) > 3 and wsse is None else None, sched=pend["scalars"],
                                          lams=pend.get("lams"), wsse=wsse)
        return metrics

    def itinf_validation_step(self, image_batch, training=False) -> Metrics:
        _, metrics = self.frame_loss_given_latent_rvs(image_batch, latent_rvs=self.latent_rvs, training=training)
        return metrics
