"""Bitstream for the mean-scale hyperprior codec: integer CDF tables + rANS on the GPU.

The reference never produces a bitstream (``compression=False`` everywhere, mshyper/models.py:246-251): its
bpp is -sum log2 p.  This module makes ``decode`` a real codec: ``Model.compress(x) -> bytes`` and
``Model.decompress(bytes) -> uint8 pixels``, with ``8 * len(bytes) / pixels`` within a few percent of the estimate.

Tables (host, float64, 16-bit precision: frequencies sum to 65536, every symbol >= 1, last symbol = ESCAPE):
  * y: 64 tables, one per integer scale index k = round(clamp(exp(raw), 0, 63)), sigma_k = SCALE_FN(k)
    (mshyper/models.py:28-32; rounding the index is what TFC's compress() path does), pmf(v) = Phi((v+.5)/s) - Phi((v-.5)/s)
    on |v| <= L_k = the symbols with pmf >= 2^-17; rarer values are escaped.
  * z: one table per channel from the deep-factorized prior, pmf(v) = sigmoid(L(v+.5)) - sigmoid(L(v-.5)).
Wire format v3 (little endian): b"SNTC" u16 version (low byte 3; high byte = arithmetic of the transforms that rebuild mu / sigma:
  0 fp32, 1 bf16x3 -- a decoder of the other arithmetic refuses the stream instead of decoding garbage) | u16 n | u32 H | u32 W | u16 C | u16 Cz | u16 hz | u16 wz | u16 h | u16 w |
  u16 segments_z | u16 segments_y | u8 lanes_z | u8 lanes_y | u32 len_words[n * segments_z] | u32 len_words[n * segments_y] |
  z payload | y payload; a stream (one per image and segment) = the lane states (8 .. 64 of them, fewer on short streams)
  + the interleaved 16-bit words (csrc/rans.hip).
The decoder rebuilds mu / scale indexes with the same hyper-synthesis kernels (deterministic, batch-invariant), so
encoder and decoder agree bit for bit.
Wire format v5 = v3 with version byte 5 and, between the header and the length fields, n signed bytes: per image the index k of its
  quantisation step on the scale ladder (``step_size``; STEP_MIN <= k <= STEP_MAX).  y - mu is quantised with the step r^k,
  r = exp(SCALE_FACTOR), and coded with the table k places down the ladder (sigma_i / r^k = sigma_(i-k): the same 64 tables serve every
  step; csrc/quant_step.hip).  Written only when some index is non-zero: all zero is the v3 blob, byte for byte.
Wire format v7 = v3 with version byte 7 and, between the header and the length fields, u32 record count | the records: the ladder
  index of EVERY latent position (all C channels of a position share it; region-of-interest coding, csrc/quant_step.hip) as
  maximal runs in raster order, image after image, a record = i8 index | u16 run length 1 .. 65535 (``pack_runs``); a run never
  crosses an image boundary.  Written only when some image's map really varies: constant maps are the v5 / v3 blob of those
  indexes, byte for byte -- a file has one spelling.  Version 6 is not assigned and stays refused.
Wire format v8 = a v3 / v5 / v7 blob wrapped in a coded pixel residual layer (csrc/residual.hip, DESIGN.md 4.7 "residual layer"):
  b"SNTC" u16 version (low byte 8; high byte = the base's arithmetic tag) | u8 max_error (0 .. 127) | u8 levels (8) | u32 base_len |
  the base file, complete and unchanged | u16 segments | u8 lanes | u8 0 | u8 choice[n * 24] | u32 len_words[n * segments] | payload.
  The payload codes, per pixel value, q = sgn(r) ((|r| + max_error) div (2 max_error + 1)), r = the uint8 original - the decoded base
  pixel, in the streams of v3 cut every 2^16 values, under ONE of the 64 y tables per (image, class) -- the table of smallest exact
  coded cost, ``choice`` -- where the class of a value is its channel and the local activity of the decoded base picture, which the
  decoder has.  The decoder adds q (2 max_error + 1) to the base and clips: every pixel within max_error of the original, the
  original itself at 0.  ``split_residual(blob)[0]`` is the base file; a nested v8 base and a v4 base are refused.

Wire format v9 = a TILED file (tiling.py, csrc/tiles.hip, DESIGN.md 4.7 "tiled files"): the picture cut into overlapping tiles that
  are coded as the images of ordinary v3 / v5 batches, so a reader decodes only the tiles a window needs:
  b"SNTC" u16 version (low byte 9; high byte = the arithmetic tag) | u16 n | u32 H | u32 W | u16 tile | u16 overlap | u16 nblobs |
  nblobs x (u16 th, u16 tw, u32 count, u32 bytes) | the inner blobs, each a complete v3 / v5 file of ``count`` images of th x tw.
  Tiles in (image, row, column) order, grouped by shape in order of first appearance, 256 to an inner blob at the most; the
  parser recomputes the whole table from (n, H, W, tile, overlap) (``tiling.parse_v9``).  Written only by ``compress(x, tile=...)``.

The factorized-prior model (factorized/models.py) has ONE latent and no hyper-synthesis: ``FactorizedCodec``, wire format v4
  b"SNTC" u16 version (low byte 4; high byte = the arithmetic tag, as above) | u16 n | u32 H | u32 W | u16 C | u16 h | u16 w |
  u16 segments | u8 lanes | u8 0 | u32 len_words[n * segments] | payload
with one table per channel of y (``factorized_tables`` on the model's prior) and the channel-indexed coder of
csrc/rans_channels.hip, which reads the float latents and writes float y_hat in one launch, without a table-id or int32
tensor (the decoder always; the encoder where it is the faster side, ``FUSED_CHANNEL_ENCODE``).
The streams themselves are those of v3 (same words as ``rans_encode`` with ``channel_table_ids``).  A v3 blob is refused by
a factorized model and a v4 blob by a hyperprior model.
"""
from __future__ import annotations

import ctypes as C
import math
import struct

import numpy as np
import torch

from . import _capi as capi
from . import ops
from . import tiling
from .tiling import VERSION_TILED, select_images, tile_index      # wire format 9: the host half

PRECISION = 16
TOTAL = 1 << PRECISION
MAGIC = b"SNTC"
VERSION = 3
VERSION_FACTORIZED = 4                    # FactorizedCodec: one latent, table = channel
ARITH = {"fp32": 0, "bf16x3": 1}          # Model(precision=...): high byte of the version word
SCALE_MIN, SCALE_MAX, NUM_SCALES = 0.11, 256.0, 64
SCALE_FACTOR = (math.log(SCALE_MAX) - math.log(SCALE_MIN)) / (NUM_SCALES - 1.0)
VERSION_STEP = 5                          # v3 + one signed byte per image: its quantisation step's index on the scale ladder
STEP_MIN, STEP_MAX = -32, 32              # ladder indexes a file may carry (checked here; the kernels' id clamp absorbs any shift)
LADDER_MAX = 16                           # candidate steps of one sntc_step_ladder_cost launch
LADDER_DECODE_BYTES = 1 << 30             # candidate latents (y_hat) one decoder batch of ``Codec.ladder_distortion`` holds at the most
VERSION_MAP = 7                           # v3 + the ladder index of every latent position, run-length coded
OFFSET_MIN, OFFSET_MAX = -64, 64          # ``step_offsets`` a caller may pass: enough to cross the whole ladder either way
RUN_MAX = 65535                           # positions one record of a v7 map covers at the most
RUN_RECORD = np.dtype([("k", "i1"), ("run", "<u2")])      # "<bH", 3 bytes
MAP_RECORD_BITS = 8 * RUN_RECORD.itemsize


def step_size(k):
    """The quantisation step of ladder index k, exp(k SCALE_FACTOR) = (sigma_(i+k) / sigma_i of the scale ladder), computed in
    float64 and rounded ONCE to float32 -- the value the kernels multiply with (returned as a Python float holding it).
    ``step_size(-k)`` is the inverse step the encoder multiplies with.  step_size(0) == 1.0."""
    k = int(k)
    if not STEP_MIN <= k <= STEP_MAX:
        raise ValueError(f"ladder index {k} outside [{STEP_MIN}, {STEP_MAX}]")
    return float(np.float32(math.exp(k * SCALE_FACTOR)))


def check_steps(step, n):
    """``step`` (an int, or a sequence of n ints) -> list of n ladder indexes; ValueError on anything else."""
    if isinstance(step, (int, np.integer)) and not isinstance(step, bool):
        ks = [int(step)] * n
    else:
        try:
            ks = list(step)
        except TypeError:
            raise ValueError(f"step must be an int or a sequence of {n} ints, not {step!r}") from None
        if len(ks) != n:
            raise ValueError(f"{len(ks)} steps for {n} images")
        if not all(isinstance(k, (int, np.integer)) and not isinstance(k, bool) for k in ks):
            raise ValueError(f"steps must be ints (indexes on the scale ladder), not {ks!r}")
        ks = [int(k) for k in ks]
    for k in ks:
        if not STEP_MIN <= k <= STEP_MAX:
            raise ValueError(f"ladder index {k} outside [{STEP_MIN}, {STEP_MAX}]")
    return ks


def check_shifts(shift, n):
    """``shift`` of ``transcode`` (an int, or a sequence of n ints: how many places up the ladder each image's file moves) -> list
    of n ints in [0, STEP_MAX - STEP_MIN]; ValueError on anything else.  A negative shift is refused: the symbols of a finer
    step are not in the file."""
    if isinstance(shift, (int, np.integer)) and not isinstance(shift, bool):
        ds = [int(shift)] * n
    else:
        try:
            ds = list(shift)
        except TypeError:
            raise ValueError(f"shift must be an int or a sequence of {n} ints, not {shift!r}") from None
        if len(ds) != n:
            raise ValueError(f"{len(ds)} shifts for {n} images")
        if not all(isinstance(d, (int, np.integer)) and not isinstance(d, bool) for d in ds):
            raise ValueError(f"shifts must be ints (places on the scale ladder), not {ds!r}")
        ds = [int(d) for d in ds]
    for d in ds:
        if d < 0:
            raise ValueError(f"shift {d} is negative: a file holds the symbols of its own step, the finer ones are not in it")
        if d > STEP_MAX - STEP_MIN:
            raise ValueError(f"shift {d} outside [0, {STEP_MAX - STEP_MIN}]")
    return ds


def check_budgets(target_bpp, n):
    """``target_bpp`` (a number, or a sequence of n numbers) -> float64 [n]; ValueError on anything else."""
    t = np.asarray(target_bpp, np.float64)
    if t.ndim == 0:
        t = np.full(n, float(t))
    if t.shape != (n,) or not np.isfinite(t).all():
        raise ValueError(f"target_bpp must be a finite number or {n} of them, not {target_bpp!r}")
    return t


def select_steps(bits, budget_bits, steps, map_bits=None):
    """The rate-control rule, a pure function: ``bits`` [n, len(steps)] = what image i would pay at ladder index steps[j],
    ``budget_bits`` [n].  Per image the SMALLEST index (the finest step) whose bits fit the budget -- not the first fit found
    walking down from a coarse step: a row need not be monotone -- and STEP_MAX, met = False, where none fits.
    ``map_bits`` [n] (rate control over ``step_offsets``): what image i's map of ladder indexes costs in the file, the same at
    every candidate; it is added to every entry of the row before the comparison and reported.
    -> list of dict(step_chosen, bits_predicted, budget_bits, met[, map_bits])."""
    bits = np.asarray(bits, np.float64)
    steps = [int(k) for k in steps]
    if bits.ndim != 2 or bits.shape[1] != len(steps) or len(budget_bits) != bits.shape[0]:
        raise ValueError("select_steps: bits [n, len(steps)] and n budgets")
    if map_bits is not None:
        map_bits = np.asarray(map_bits, np.float64)
        if map_bits.shape != (bits.shape[0],):
            raise ValueError("select_steps: one map_bits per image")
        bits = bits + map_bits[:, None]
    out = []
    for i, (row, budget) in enumerate(zip(bits, budget_bits)):
        fits = [k for k, b in zip(steps, row) if b <= budget]
        k = min(fits) if fits else STEP_MAX
        pred = float(row[steps.index(k)]) if k in steps else float("nan")
        out.append(dict(step_chosen=k, bits_predicted=pred, budget_bits=float(budget), met=bool(fits)))
        if map_bits is not None:
            out[-1]["map_bits"] = float(map_bits[i])
    return out


def check_quality(target_psnr, n):
    """``target_psnr`` in dB (a number, or a sequence of n numbers) -> float64 [n]; ValueError on anything else."""
    try:
        t = np.asarray(target_psnr, np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"target_psnr must be a finite number or {n} of them, not {target_psnr!r}") from None
    if t.ndim == 0:
        t = np.full(n, float(t))
    if t.shape != (n,) or not np.isfinite(t).all():
        raise ValueError(f"target_psnr must be a finite number or {n} of them, not {target_psnr!r}")
    return t


def quality_budgets(targets, H, W):
    """PSNR targets in dB (``check_quality``) -> the largest squared error of the decoded uint8 pixels of an H x W RGB image
    that still meets them, float64: 255^2 3 H W / 10^(target / 10).  Compared against the INTEGER SSE: sse <= budget."""
    return 255.0 ** 2 * 3.0 * float(H) * float(W) / 10.0 ** (np.asarray(targets, np.float64) / 10.0)


def psnr_of_sse(sse, elements):
    """PSNR in dB of a squared error over ``elements`` = 3 H W pixel values on the 0-255 scale, float64 (inf at sse 0)."""
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(255.0 ** 2 * float(elements) / np.asarray(sse, np.float64))


def select_quality(bits, sse, sse_budget, steps, elements=None):
    """The quality-target rule, a pure function: ``bits`` [n, len(steps)] = what image i would pay at ladder index steps[j],
    ``sse`` [n, len(steps)] = the integer squared error it would decode to there, ``sse_budget`` [n] (``quality_budgets``).
    Per image, among the candidates with sse <= budget, the one with the FEWEST bits -- not the coarsest that qualifies: neither
    row need be monotone -- and on equal bits the larger ladder index; STEP_MIN, met = False, where none qualifies.
    ``elements`` (3 H W, if the caller has it): psnr_predicted of the chosen candidate's sse, else None.
    -> list of dict(step_chosen, bits_predicted, sse_predicted, psnr_predicted, sse_budget, met)."""
    bits, sse = np.asarray(bits, np.float64), np.asarray(sse, np.float64)
    steps = [int(k) for k in steps]
    if bits.ndim != 2 or bits.shape[1] != len(steps) or sse.shape != bits.shape or len(sse_budget) != bits.shape[0]:
        raise ValueError("select_quality: bits and sse [n, len(steps)] and n budgets")
    out = []
    for brow, srow, budget in zip(bits, sse, sse_budget):
        ok = [j for j in range(len(steps)) if srow[j] <= budget]
        j = min(ok, key=lambda j: (brow[j], -steps[j])) if ok else (steps.index(STEP_MIN) if STEP_MIN in steps else None)
        k = steps[j] if ok else STEP_MIN
        b, e = (float(brow[j]), float(srow[j])) if j is not None else (float("nan"), float("nan"))
        psnr = None if elements is None else float(psnr_of_sse(e, elements))
        out.append(dict(step_chosen=k, bits_predicted=b, sse_predicted=e, psnr_predicted=psnr, sse_budget=float(budget), met=bool(ok)))
    return out


def check_offsets(step_offsets, n, h, w):
    """``step_offsets`` of the public entry points -> C-contiguous int8 [n, h, w] (h, w: the latent resolution,
    ``Codec.latent_shapes``); ValueError on a wrong shape, non-integers, bools, or values outside [OFFSET_MIN, OFFSET_MAX]."""
    if isinstance(step_offsets, torch.Tensor):
        step_offsets = step_offsets.detach().cpu().numpy()
    a = np.asarray(step_offsets)
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"step_offsets must be integers (offsets on the scale ladder), not {a.dtype}")
    if a.shape != (n, h, w):
        raise ValueError(f"step_offsets of shape {a.shape}: one offset per latent position, {(n, h, w)}")
    if a.size and not (OFFSET_MIN <= int(a.min()) and int(a.max()) <= OFFSET_MAX):
        raise ValueError(f"step_offsets outside [{OFFSET_MIN}, {OFFSET_MAX}]")
    return np.ascontiguousarray(a, dtype=np.int8)


def index_map(steps, offsets):
    """K[i, p] = clip(step_i + step_offsets[i, p], STEP_MIN, STEP_MAX): the absolute ladder index of every position, int8 like
    ``offsets`` ([n, h, w], ``check_offsets``); ``steps``: n ladder indexes."""
    base = np.asarray(steps, np.int64).reshape(-1, 1, 1)
    return np.clip(base + offsets.astype(np.int64), STEP_MIN, STEP_MAX).astype(np.int8)


def position_weights(kmap):
    """The weight of every latent position's pixels in the distortion of SGA on a step map, a pure function: absolute ladder
    indexes K int8 [n, h, w] (``index_map``) -> float64 [n, h, w], omega = 1 / step_size(K)^2 -- what ``step_lambdas(1.0, [k])``
    gives an image whose every position is k (the same modelling choice).  The device copy is this rounded once
    to float32."""
    K = np.asarray(kmap)
    if K.dtype != np.int8 or K.ndim != 3:
        raise ValueError("position_weights: absolute ladder indexes, int8 [n, h, w]")
    if K.size and not (STEP_MIN <= int(K.min()) and int(K.max()) <= STEP_MAX):
        raise ValueError(f"ladder index outside [{STEP_MIN}, {STEP_MAX}]")
    table = np.array([1.0 / step_size(k) ** 2 for k in range(STEP_MIN, STEP_MAX + 1)], np.float64)
    return table[K.astype(np.int64) - STEP_MIN]


def uniform_steps(kmap):
    """The per-image ladder indexes of a map whose every image is constant (the file is then v5 / v3), else None."""
    flat = kmap.reshape(kmap.shape[0], -1)
    return flat[:, 0].astype(np.int64).tolist() if (flat == flat[:, :1]).all() else None


def count_runs(a):
    """Maximal runs of equal values per image of ``a`` [n, ...], raster order -> int64 [n]."""
    flat = np.asarray(a).reshape(len(a), -1)
    return 1 + (flat[:, 1:] != flat[:, :-1]).sum(axis=1).astype(np.int64)


def pack_runs(K) -> bytes:
    """The absolute maps K (int8 [n, h w], raster order, image-major) as records ``<bH`` = (ladder index, run length 1 .. 65535).
    Runs are maximal (neighbouring equal values merge) but never cross an image boundary; a run above 65535 is split into full
    records and a remainder.  One spelling per map."""
    K = np.asarray(K)
    if K.ndim != 2 or K.dtype != np.int8 or K.shape[1] < 1:
        raise ValueError("pack_runs: int8 [n, h * w]")
    if K.size and not (STEP_MIN <= int(K.min()) and int(K.max()) <= STEP_MAX):
        raise ValueError(f"ladder index outside [{STEP_MIN}, {STEP_MAX}]")
    ks, runs = [], []
    hw = K.shape[1]
    for row in K:
        starts = np.concatenate([[0], np.flatnonzero(row[1:] != row[:-1]) + 1])
        lens = np.diff(np.concatenate([starts, [hw]]))
        pieces = -(-lens // RUN_MAX)                                  # records per run
        k = np.repeat(row[starts], pieces)
        r = np.full(len(k), RUN_MAX, np.int64)
        r[np.cumsum(pieces) - 1] = lens - (pieces - 1) * RUN_MAX      # the last record of each run takes the remainder
        ks.append(k)
        runs.append(r)
    rec = np.empty(sum(len(k) for k in ks), RUN_RECORD)
    rec["k"], rec["run"] = np.concatenate(ks), np.concatenate(runs)
    return rec.tobytes()


def parse_runs(buf, n, hw):
    """The records of ``pack_runs`` -> K int8 [n, hw].  Refused (ERR_BAD_SHAPE): an index outside the ladder, a zero run, a run
    crossing an image boundary, records that do not sum to hw for every image."""
    bad = lambda what: capi.SntcError(capi.ERR_BAD_SHAPE, f"bitstream header: step map {what}")
    if len(buf) % RUN_RECORD.itemsize:
        raise bad("is not a whole number of records")
    rec = np.frombuffer(buf, RUN_RECORD)
    k, run = rec["k"], rec["run"].astype(np.int64)
    if len(rec) and not (STEP_MIN <= int(k.min()) and int(k.max()) <= STEP_MAX):
        raise bad(f"holds a quantisation step index outside [{STEP_MIN}, {STEP_MAX}]")
    if (run == 0).any():
        raise bad("holds a run of length 0")
    ends = np.cumsum(run)
    if not len(rec) or int(ends[-1]) != n * hw:
        raise bad(f"covers {int(ends[-1]) if len(rec) else 0} positions, the latents have {n} x {hw}")
    if not np.isin(np.arange(1, n + 1, dtype=np.int64) * hw, ends).all():
        raise bad("has a run that crosses an image boundary")
    return np.repeat(k, run).reshape(n, hw)


def roi_offsets(mask, factor, inside=0, outside=12, grow=1, latent_hw=None):
    """A boolean pixel mask [n, H, W] (True = region of interest) -> ``step_offsets`` int8 [n, h, w]: ``inside`` where the
    position's factor x factor block of the padded image meets the mask, after the inside set has been dilated by ``grow``
    positions (8-neighbourhood: the synthesis reads neighbouring positions), ``outside`` elsewhere.  The image is padded
    bottom / right and the padding is cropped after decoding, so the mask is False there.  ``factor``: pixels per latent
    position (16 for the models here); ``latent_hw`` = ``Model.step_offsets_shape(H, W)`` where the model pads the image beyond the
    next multiple of ``factor`` (default: ceil(H / factor), ceil(W / factor))."""
    mask = np.asarray(mask)
    factor, grow = int(factor), int(grow)
    if mask.ndim != 3 or mask.dtype != np.bool_ or factor < 1 or grow < 0:
        raise ValueError("roi_offsets: a boolean mask [n, H, W], factor >= 1, grow >= 0")
    for v in (inside, outside):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not OFFSET_MIN <= int(v) <= OFFSET_MAX:
            raise ValueError(f"roi_offsets: inside / outside are ints in [{OFFSET_MIN}, {OFFSET_MAX}]")
    n, H, W = mask.shape
    h, w = (-(-H // factor), -(-W // factor)) if latent_hw is None else (int(latent_hw[0]), int(latent_hw[1]))
    if h * factor < H or w * factor < W:
        raise ValueError(f"roi_offsets: {h} x {w} positions of {factor} pixels do not cover a {H} x {W} image")
    padded = np.zeros((n, h * factor, w * factor), np.bool_)
    padded[:, :H, :W] = mask
    roi = padded.reshape(n, h, factor, w, factor).any(axis=(2, 4))
    for _ in range(grow):
        wide = np.zeros((n, h + 2, w + 2), np.bool_)
        for dy in range(3):
            for dx in range(3):
                wide[:, dy:dy + h, dx:dx + w] |= roi
        roi = wide[:, 1:-1, 1:-1]
    return np.where(roi, np.int8(inside), np.int8(outside)).astype(np.int8)


def quantize_pmf(pmf, escape_mass):
    """pmf (float64, symbols in value order) + escape -> integer frequencies, each >= 1, summing to 65536."""
    p = np.concatenate([np.maximum(np.asarray(pmf, np.float64), 0.0), [max(float(escape_mass), 0.0)]])
    p = p / p.sum()
    n = len(p)
    if n > TOTAL // 2:
        raise ValueError("table too wide for 16-bit precision")
    f = 1 + np.floor(p * (TOTAL - n)).astype(np.int64)
    f[np.argmax(p)] += TOTAL - int(f.sum())            # the leftover (< n) goes to the most probable symbol
    assert f.min() >= 1 and int(f.sum()) == TOTAL
    return f


def _ndtr(x):
    return 0.5 * math.erfc(-x / math.sqrt(2.0))


def normal_tables(min_pmf=2.0 ** -17, max_half_width=4095):
    """64 tables; table k spans |v| <= L_k, the symbols whose probability is worth a frequency count of its own
    (pmf >= 2^-17, i.e. >= 1/2 count at 16-bit precision).  Rarer values go through ESCAPE (~32 bits against an
    ideal > 17): the extra cost is bounded by 15 bits x 2^-17 per symbol."""
    tabs = []
    for k in range(NUM_SCALES):
        sigma = math.exp(math.log(SCALE_MIN) + SCALE_FACTOR * k)
        pmf_at = lambda t: _ndtr((t + 0.5) / sigma) - _ndtr((t - 0.5) / sigma) if t <= 0 else _ndtr(-(t - 0.5) / sigma) - _ndtr(-(t + 0.5) / sigma)
        L = 0
        while L < max_half_width and pmf_at(L + 1) >= min_pmf:
            L += 1
        v = np.arange(-L, L + 1)
        pmf = np.array([pmf_at(int(t)) for t in v])
        tabs.append((-L, quantize_pmf(pmf, 2.0 * _ndtr(-(L + 0.5) / sigma))))
    return tabs


def _df_logits(x, mats, biases, factors):
    """Host float64 mirror of tfc.DeepFactorized._logits_cumulative for ONE channel; x: [n]."""
    h = np.asarray(x, np.float64)[None, :]
    nl = len(mats)
    for k in range(nl):
        h = np.logaddexp(0.0, mats[k]) @ h + biases[k][:, None]
        if k < nl - 1:
            h = h + np.tanh(factors[k])[:, None] * np.tanh(h)
    return h[0]


def factorized_tables(prior_weights, num_layers, tail_mass=2.0 ** -12, max_half_width=2047):
    c = prior_weights["prior/matrix_0"].shape[0]
    tabs = []
    for ch in range(c):
        mats = [prior_weights[f"prior/matrix_{k}"][ch].astype(np.float64) for k in range(num_layers)]
        bs = [prior_weights[f"prior/bias_{k}"][ch].astype(np.float64) for k in range(num_layers)]
        fs = [prior_weights[f"prior/factor_{k}"][ch].astype(np.float64) for k in range(num_layers - 1)]
        edges = np.arange(-max_half_width - 0.5, max_half_width + 1.0)           # v - .5 for v = -L..L+1
        cdf = 1.0 / (1.0 + np.exp(-_df_logits(edges, mats, bs, fs)))
        pmf = np.diff(cdf)                                                        # pmf[i] for v = -max + i
        keep = np.nonzero(pmf > tail_mass / 64.0)[0]
        lo, hi = (int(keep[0]), int(keep[-1])) if len(keep) else (max_half_width, max_half_width)
        tabs.append((lo - max_half_width, quantize_pmf(pmf[lo:hi + 1], cdf[lo] + (1.0 - cdf[hi + 1]))))
    return tabs


def decoder_entries(tabs):
    """(cdf[s] << 16) | (freq[s] - 1) for every symbol of every table, three 0xffffffff after each table, padded to a multiple
    of four entries."""
    out = []
    for _, f in tabs:
        f = np.asarray(f, np.int64)
        cdf = np.concatenate([[0], np.cumsum(f)[:-1]])
        assert len(f) >= 2 and f.min() >= 1 and f.max() <= 65535
        out.append(((cdf << 16) | (f - 1)).astype(np.uint32))
        out.append(np.full(3, 0xFFFFFFFF, np.uint32))
    flat = np.concatenate(out)
    pad = -len(flat) % 4
    return np.concatenate([flat, np.full(pad, 0xFFFFFFFF, np.uint32)]) if pad else flat


def start_tables(cdfs, bits):
    """Per table the decoder's start table: entry b of 2^bits = the largest symbol s with cdf[s] <= b << (16 - bits).
    -> (uint16 entries of all tables, padded to a multiple of eight; uint32 (offset << 5) | bits per table)."""
    luts, lmeta, pos = [], [], 0
    for cdf, b in zip(cdfs, bits):
        base = np.arange(1 << b, dtype=np.int64) << (16 - b)
        lut = np.searchsorted(cdf.astype(np.int64), base, side="right") - 1
        assert lut.min() >= 0 and lut.max() < len(cdf)
        luts.append(lut.astype(np.uint16))
        lmeta.append((pos << 5) | b)
        pos += len(lut)
    flat = np.concatenate(luts)
    pad = -len(flat) % 8
    if pad:
        flat = np.concatenate([flat, np.zeros(pad, np.uint16)]).astype(np.uint16)
    return flat, np.asarray(lmeta, np.uint32)


COST_UNIT = 1 << 16                      # ``rans_cost`` counts in 2^-16 bit
RANS_COST_THREADS, RANS_COST_VEC = 1024, 4      # csrc/rans_cost.hip: a workgroup takes 1024 elements per pass, 4096 where the
                                                # image's element count is a multiple of 4 (tests place sizes around both)


def cost_table(tabs):
    """What a symbol of each table costs the rANS coder, in units of 2^-16 bit: entry s of table t = rint((16 - log2 f_s) * 65536)
    with f_s the integer frequency the coder uses; the last entry of every table (ESCAPE) carries the 16 raw bits of the
    escaped value on top.  -> uint32, one entry per cdf entry, tables back to back (the offsets of ``DeviceTables.cdf``)."""
    out = []
    for _, f in tabs:
        c = np.rint((PRECISION - np.log2(np.asarray(f, np.float64))) * COST_UNIT).astype(np.int64)
        c[-1] += 16 * COST_UNIT
        out.append(c)
    return np.concatenate(out).astype(np.uint32)


class DeviceTables:
    """Concatenated uint16 CDFs (cdf[n] = 65536 implicit) + packed per-table descriptors on the device."""

    def __init__(self, tabs, device):
        cdfs, meta = [], []
        pos = 0
        for lo, f in tabs:
            cdf = np.concatenate([[0], np.cumsum(f)[:-1]]).astype(np.uint16)     # cdf of symbols 0..n-1
            if not -32768 <= lo <= 32767 or len(f) > 32768:
                raise ValueError("table outside the 16-bit descriptor range")
            meta.append((pos, (len(f) << 16) | (lo & 0xFFFF)))
            cdfs.append(cdf)
            pos += len(cdf)
        flat = np.concatenate(cdfs)
        if len(flat) % 2:
            flat = np.concatenate([flat, [0]]).astype(np.uint16)                  # kernels copy 32 bits at a time
        self.host = tabs
        self.ntables, self.total = len(tabs), pos
        self.cdf = torch.from_numpy(flat.view(np.int16).copy()).to(device)
        self.meta = torch.from_numpy(np.asarray(meta, np.uint32).view(np.int32).copy()).to(device)
        self.cost_q = torch.from_numpy(cost_table(tabs).view(np.int32).copy()).to(device)      # sntc_rans_cost: same offsets as cdf
        # the decoder's own view of the tables (include/sntc.h, sntc_rans_decode): packed (start, frequency - 1) entries with
        # three sentinels per table, and start tables of about one entry per symbol -- a table of n symbols gets 2^ceil(log2 n)
        # buckets, one bit more where the CU's LDS has the room, fewer where it has not
        budget = int(capi.load().sntc_rans_lut_budget(self.ntables, self.total))
        self.dec, self.lut, self.lut_meta, self.lut_total, self.lut_bits = None, None, None, 0, None
        for extra in (1, 0, -1, -2, -3, -4, -5, -6):
            bits = [min(16, max(0, int(np.ceil(np.log2(max(len(f), 1)))) + extra)) for _, f in tabs]
            if -(-sum(1 << b for b in bits) // 8) * 8 <= budget:
                lut, lmeta = start_tables(cdfs, bits)
                dec = decoder_entries(tabs)
                self.lut_bits, self.lut_total = bits, len(lut)
                self.dec = torch.from_numpy(dec.view(np.int32).copy()).to(device)
                self.lut = torch.from_numpy(lut.view(np.int16).copy()).to(device)
                self.lut_meta = torch.from_numpy(lmeta.view(np.int32).copy()).to(device)
                break


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


PIPELINE_BLOBS = True           # decompress_many: blobs pipelined largest first (False: round 4's two-phase schedule; same pixels)
USE_START_TABLES = True         # decoder: its own tables in LDS, DeviceTables.dec / .lut (False: binary search of cdf; same values)

FUSED_CHANNEL_ENCODE = False    # FactorizedCodec's encoder: False = round_to_int + channel_table_ids + rans_encode, True = the one
                                # launch of sntc_rans_encode_channels.  Same bytes.  On the latents of 18 / 1 images of 512 x 768
                                # at C = 256 the three launches measured about 1.1 ms, the one launch 1.2 - 1.4 ms, so the faster
                                # side is called; the decoder's one launch measured 2.5 - 2.6 ms against 3.0 - 3.1 ms for its
                                # composition and is always used (profiles/factorized_codec.json).

ELEMS_PER_SEGMENT = 1 << 18     # one rANS stream (= one wave of coding parallelism, 256 bytes of flushed lane states) per
                                # this many latent elements: ~0.008 bit / element of overhead; a Kodak image = 1 z + 2 y streams


def _segments(elems, segments=None):
    if segments is None:
        segments = -(-elems // ELEMS_PER_SEGMENT)
    return max(1, min(int(segments), -(-elems // 64)))


def _lanes(elems_per_stream, lanes=None):
    """Lane states flushed per stream (4 bytes each): all 64 on long streams, fewer on short ones (the hyper-latents of a
    small image would otherwise pay 256 bytes of states for a few hundred bytes of payload)."""
    if lanes is not None:
        return int(lanes)
    return 64 if elems_per_stream >= 16384 else 32 if elems_per_stream >= 6144 else 16 if elems_per_stream >= 2048 else 8


def _encode_scratch(x, segments, lanes):
    """What both encoder launches set up for the tensor ``x`` [n, ...] they code: the stream geometry and a ``cap``-word scratch
    row + a length per stream.  -> (n, E, segments, lanes, cap, scratch int16 [streams, cap], lens int32 [streams])."""
    n = x.shape[0]
    E = x.numel() // n
    segments = _segments(E, segments)
    lanes = _lanes(-(-E // segments), lanes)
    cap = int(capi.load().sntc_rans_cap_words(E, segments))
    scratch = torch.empty((n * segments, cap), dtype=torch.int16, device=x.device)
    lens = torch.empty((n * segments,), dtype=torch.int32, device=x.device)
    return n, E, segments, lanes, cap, scratch, lens


def rans_encode_launch(values, table_ids, tables: DeviceTables, segments=None, lanes=None):
    """The device half of ``rans_encode``: every stream coded into its own ``cap``-word scratch row, no host synchronisation.
    -> (scratch int16 [streams, cap], lens int32 [streams]) for ``rans_encode_finish``."""
    n, E, segments, lanes, cap, scratch, lens = _encode_scratch(values, segments, lanes)
    capi.call("sntc_rans_encode", _p(values), _p(table_ids), n, E, segments, lanes, _p(tables.cdf), _p(tables.meta), tables.ntables,
              tables.total, cap, _p(scratch), _p(lens), ops._stream())
    return scratch, lens


def rans_encode_finish(scratch, lens, lens_h):
    """The streams of ``rans_encode_launch`` packed back to back: ``lens_h`` = ``lens`` on the host (int64).  -> payload (device)."""
    dev = scratch.device
    offsets = np.concatenate([[0], np.cumsum(lens_h)]).astype(np.int64)
    payload = torch.empty((int(offsets[-1]),), dtype=torch.int16, device=dev)
    offs_d = torch.from_numpy(offsets).to(dev)
    capi.call("sntc_rans_compact", _p(scratch), scratch.shape[1], _p(lens), _p(offs_d), scratch.shape[0], _p(payload), ops._stream())
    return payload


def rans_encode(values, table_ids, tables: DeviceTables, segments=None, lanes=None):
    """values int32 [n, ...], table_ids uint16 (int16 storage) same shape -> (payload int16-storage words on the
    device, len_words int64[n * segments])."""
    scratch, lens = rans_encode_launch(values, table_ids, tables, segments, lanes)
    lens_h = lens.cpu().numpy().astype(np.int64)
    return rans_encode_finish(scratch, lens, lens_h), lens_h


def _decode_setup(shape, out_dtype, payload, lens_h, tables, segments, lanes, bad, offsets):
    """What both decoders set up before their launch: the stream geometry of ``shape`` [n, ...], the offsets on the device, the
    output tensor, the counter of malformed streams (``bad``, or a fresh one) and the decoder's own tables where they are used.
    -> (n, E, segments, lanes, offsets, out, bad, (dec, lut, lut_meta, lut_total) as call arguments)."""
    n = shape[0]
    E = int(np.prod(shape)) // n
    segments = _segments(E, segments)
    lanes = _lanes(-(-E // segments), lanes)
    if len(lens_h) != n * segments:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "stream count does not match the image / segment counts")
    dev = payload.device
    if offsets is None:        # ``offsets``: the exclusive prefix sum of lens_h already on the device (int64 [streams + 1])
        offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lens_h)]).astype(np.int64)).to(dev)
    out = torch.empty(tuple(shape), dtype=out_dtype, device=dev)
    if bad is None:
        bad = torch.zeros((1,), dtype=torch.int32, device=dev)
    fast = USE_START_TABLES and tables.dec is not None
    dec = (_p(tables.dec if fast else None), _p(tables.lut if fast else None), _p(tables.lut_meta if fast else None),
           tables.lut_total if fast else 0)
    return n, E, segments, lanes, offsets, out, bad, dec


def _raise_if_bad(nbad, streams, nres=None):
    """The one refusal of a corrupt payload: ``nbad`` of ``streams`` rANS streams ended in a state no encoder leaves (host ints,
    read back where the caller synchronises anyway); ``nres`` (a layered file): the residual values outside what an encoder writes."""
    if nbad or nres:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, f"bitstream corrupt: {nbad} of {streams} rANS streams did not terminate cleanly" +
                             ("" if nres is None else f", {nres} residual values lie outside what an encoder writes"))


def pack_upload(arrays, device):
    """ONE upload for several host arrays: packed in the order given into one uint8 buffer, each at an offset aligned to its item
    size (padded where the order does not give that), one copy to ``device``.  -> (the buffer on the device -- what a caller
    names to ``ops.fork`` where a lane reads the views --, the arrays as flat device tensors of their dtypes: views of it)."""
    arrays = [np.asarray(a).reshape(-1) for a in arrays]
    at, pos = [], 0
    for a in arrays:
        pos += -pos % a.itemsize
        at.append(pos)
        pos += a.nbytes
    host = np.empty(pos, np.uint8)
    for a, o in zip(arrays, at):
        assert o % a.itemsize == 0
        host[o:o + a.nbytes].view(a.dtype)[:] = a
    up = torch.from_numpy(host).to(device) if pos else torch.empty(0, dtype=torch.uint8, device=device)      # (numpy's empty: stride 0)
    return up, [up[o:o + a.nbytes].view(torch.from_numpy(np.empty(0, a.dtype)).dtype) for a, o in zip(arrays, at)]


def finish_streams(jobs):
    """The two read-backs that end every encode, for ALL blobs at once: ``jobs`` = per blob the (scratch, lens) groups of its
    ``rans_encode_launch`` calls -> per blob, per group, (lens on the host int64, the group's streams packed back to back as
    int16 words on the host).  The stream lengths come back in one copy, the packed payloads in another; then
    ``ops.check_conv_status()``: the copies synchronised the stream, a flagged stream-K launch raises here, not a wrong file."""
    groups = [g for job in jobs for g in job]
    cat = lambda ts: ts[0] if len(ts) == 1 else torch.cat(ts)
    lens_h = cat([lens for _, lens in groups]).cpu().numpy().astype(np.int64)                                   # read-back 1 of 2
    cuts = np.cumsum([0] + [lens.numel() for _, lens in groups])
    lens_h = [lens_h[a:b] for a, b in zip(cuts, cuts[1:])]
    words = cat([rans_encode_finish(s, lens, lh) for (s, lens), lh in zip(groups, lens_h)]).cpu().numpy()        # read-back 2 of 2
    ops.check_conv_status()
    cuts = np.cumsum([0] + [int(lh.sum()) for lh in lens_h])
    done = iter([(lh, words[a:b]) for lh, a, b in zip(lens_h, cuts, cuts[1:])])
    return [[next(done) for _ in job] for job in jobs]


def _compress_many(codec, xs):
    """``compress_many`` of both codecs: ``codec._launch(x)`` per batch, each on a lane of its own (``ops.lanes``), its stream
    groups handed to the caller's stream, ``codec._finish`` for the set."""
    m = codec.m
    xs = [m._as_device_images(x) for x in xs]
    if not xs:
        return []
    with torch.cuda.device(m.device):
        main, lanes = ops.lanes(len(xs), m.device)
        jobs = []
        for st, x in zip(lanes, xs):
            with ops.fork(main, st, reads=(x,)):
                jobs.append(codec._launch(x))
        for st, j in zip(lanes, jobs):
            ops.join(main, st, made=[t for g in j["groups"] for t in g])
        return codec._finish(jobs)


def rans_decode(payload, lens_h, table_ids, shape, tables: DeviceTables, segments=None, lanes=None, bad=None, offsets=None):
    """-> int32 values of ``shape`` [n, ...]; raises on a malformed stream.  ``bad`` (an int32 device tensor [1]): count the
    malformed streams there instead of reading the count back here -- the caller checks it where it
    synchronises anyway (a decoder that keeps several batches in flight).  The decoder's start tables are used where
    ``DeviceTables`` could place them (``tables.dec``); else the binary search of ``cdf``."""
    n, E, segments, lanes, offsets, values, count, dec = _decode_setup(shape, torch.int32, payload, lens_h, tables, segments, lanes, bad, offsets)
    capi.call("sntc_rans_decode", _p(payload), _p(offsets), _p(table_ids), n, E, segments, lanes, _p(tables.cdf), _p(tables.meta),
              tables.ntables, tables.total, *dec, _p(values), _p(count), ops._stream())
    if bad is None:
        _raise_if_bad(int(count.item()), n * segments)
    return values


def rans_cost(values, table_ids, tables: DeviceTables):
    """What ``rans_encode`` would pay for the symbols of ``values`` (int32 [n, ...], ``table_ids`` as there), without coding
    them: -> int64 [n] on the device, in units of 2^-16 bit (divide by ``COST_UNIT`` for bits), the exact integer sum of
    ``tables.cost_q`` over each image's symbols.  No host synchronisation.  The flushed lane states and the coder's
    renormalisation slack come on top in the file."""
    if values.dtype != torch.int32 or table_ids.dtype != torch.int16 or not values.is_contiguous() or not table_ids.is_contiguous() \
            or values.numel() != table_ids.numel():
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "rans_cost: values int32 and table_ids int16 (uint16 storage), contiguous, of one size")
    n = values.shape[0]
    cost = torch.empty((n,), dtype=torch.int64, device=values.device)
    capi.call("sntc_rans_cost", _p(values), _p(table_ids), n, values.numel() // n, _p(tables.meta), tables.ntables, tables.total,
              _p(tables.cost_q), _p(cost), ops._stream())
    return cost


def rans_encode_channels_launch(y, tables: DeviceTables, segments=None, lanes=None, want_y_hat=False):
    """``rans_encode_launch`` for float latents ``y`` [n, ..., C] whose table is their channel (``tables``: one per channel):
    rounded (half to even) and coded in ONE launch, no id tensor.  -> (scratch, lens, y_hat or None); y_hat = the rounded
    latents as floats when asked for."""
    if y.dtype != torch.float32 or not y.is_contiguous():
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "rans_encode_channels: y must be a contiguous float32 tensor")
    n, c = y.shape[0], y.shape[-1]
    if c != tables.ntables:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, f"rans_encode_channels: {c} channels, {tables.ntables} tables")
    n, E, segments, lanes, cap, scratch, lens = _encode_scratch(y, segments, lanes)
    y_hat = torch.empty_like(y) if want_y_hat else None
    capi.call("sntc_rans_encode_channels", _p(y), n, E, c, segments, lanes, _p(tables.cdf), _p(tables.meta), tables.total, cap,
              _p(scratch), _p(lens), _p(y_hat), ops._stream())
    return scratch, lens, y_hat


def rans_encode_channels(y, tables: DeviceTables, segments=None, lanes=None, want_y_hat=False):
    """-> (payload, len_words int64[n * segments], y_hat or None): the words of ``rans_encode(round_to_int(y),
    channel_table_ids(y.shape), ...)``."""
    scratch, lens, y_hat = rans_encode_channels_launch(y, tables, segments, lanes, want_y_hat)
    lens_h = lens.cpu().numpy().astype(np.int64)
    return rans_encode_finish(scratch, lens, lens_h), lens_h, y_hat


def rans_decode_channels(payload, lens_h, shape, tables: DeviceTables, segments=None, lanes=None, bad=None, offsets=None):
    """``rans_decode`` for a latent whose table is its channel -> the values as float32 of ``shape`` [n, ..., C] (what the
    synthesis consumes).  ``bad`` / ``offsets`` as in ``rans_decode``.  The decoder's start tables are used where
    ``DeviceTables`` could place them (``tables.dec``); else the binary search of ``cdf``."""
    c = shape[-1]
    if c != tables.ntables:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, f"rans_decode_channels: {c} channels, {tables.ntables} tables")
    n, E, segments, lanes, offsets, y_hat, count, dec = _decode_setup(shape, torch.float32, payload, lens_h, tables, segments, lanes, bad, offsets)
    capi.call("sntc_rans_decode_channels", _p(payload), _p(offsets), n, E, c, segments, lanes, _p(tables.cdf), _p(tables.meta),
              tables.total, *dec, _p(y_hat), _p(count), ops._stream())
    if bad is None:
        _raise_if_bad(int(count.item()), n * segments)
    return y_hat


def scale_table_ids(hyper):
    n, h, w, c2 = hyper.shape
    tid = torch.empty((n, h, w, c2 // 2), dtype=torch.int16, device=hyper.device)
    capi.call("sntc_scale_table_ids", _p(hyper), n * h * w, c2 // 2, _p(tid), ops._stream())
    return tid


def step_tensors(steps, device):
    """Ladder indexes -> what the step kernels read, on ``device``: (step float32, inv_step float32, shift int32), one entry
    per index (``step_size``: float64, rounded once)."""
    ks = [int(k) for k in steps]
    host = np.empty((3, len(ks)), np.float32)                      # ONE upload; the third row holds the int32 shifts' bits
    host[0] = [step_size(k) for k in ks]
    host[1] = [step_size(-k) for k in ks]
    host[2].view(np.int32)[:] = ks
    t = torch.from_numpy(host).to(device)
    return t[0], t[1], t[2].view(torch.int32)


def step_table_ids(base_ids, shift):
    """``scale_table_ids`` shifted down the ladder: clamp(id - shift[image], 0, 63) (int16 storage of uint16, shape kept);
    ``shift`` int32 [n] on the device.  What the decoder of a v5 blob indexes its tables with."""
    n = base_ids.shape[0]
    if base_ids.dtype != torch.int16 or not base_ids.is_contiguous() or shift.dtype != torch.int32 or shift.numel() != n:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "step_table_ids: contiguous int16 (uint16 storage) ids and one int32 shift per image")
    out = torch.empty_like(base_ids)
    capi.call("sntc_step_table_ids", _p(base_ids), n, base_ids.numel() // n, _p(shift), _p(out), ops._stream())
    return out


def _check_ladder_latents(y, hyper, base_ids, what):
    c = y.shape[-1]
    if y.dtype != torch.float32 or hyper.dtype != torch.float32 or base_ids.dtype != torch.int16 or y.dim() != 4 or hyper.dim() != 4 \
            or tuple(hyper.shape[:3]) != tuple(y.shape[:3]) or hyper.shape[-1] not in (c, 2 * c) or tuple(base_ids.shape) != tuple(y.shape) \
            or not (y.is_contiguous() and hyper.is_contiguous() and base_ids.is_contiguous()):
        raise capi.SntcError(capi.ERR_BAD_SHAPE, f"{what}: y float32 [n, h, w, c], hyper [n, h, w, c or 2 c], ids int16 like y, contiguous")


def _ladder_cost_chunks(y, count, launch):
    """int64 [n, count] on y's device from launches of at most ``LADDER_MAX`` candidates: ``launch(lo, k, part)`` prices candidates
    lo ... lo + k - 1 into ``part`` int64 [n, k]."""
    n = y.shape[0]
    cost = torch.empty((n, count), dtype=torch.int64, device=y.device)
    for lo in range(0, count, LADDER_MAX):
        k = min(LADDER_MAX, count - lo)
        part = cost if k == count else torch.empty((n, k), dtype=torch.int64, device=y.device)
        launch(lo, k, part)
        if part is not cost:
            cost[:, lo:lo + k] = part
    return cost


def step_ladder_cost(y, hyper, base_ids, steps, tables: DeviceTables, tensors=None):
    """``rans_cost`` of the symbols and ids an image ``StepGrid`` would form at EVERY ladder index of ``steps`` (shared by the
    batch), without forming them: one pass over y / mu / ids per launch of at most ``LADDER_MAX`` candidates.
    -> int64 [n, len(steps)] on the device, 2^-16 bit.  ``tensors``: ``step_tensors(steps, device)`` if the caller keeps them."""
    _check_ladder_latents(y, hyper, base_ids, "step_ladder_cost")
    steps = check_steps(list(steps), len(steps))
    if not steps:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "step_ladder_cost: no candidate step")
    n, hw, c = y.shape[0], y.shape[1] * y.shape[2], y.shape[3]
    _, inv, sh = step_tensors(steps, y.device) if tensors is None else tensors

    def launch(lo, k, part):
        capi.call("sntc_step_ladder_cost", _p(y), _p(hyper), n, hw, c, hyper.shape[-1], _p(base_ids), _p(inv[lo:lo + k]), _p(sh[lo:lo + k]),
                  k, _p(tables.meta), tables.ntables, tables.total, _p(tables.cost_q), _p(part), ops._stream())
    return _ladder_cost_chunks(y, len(steps), launch)


def step_lut(device):
    """What the step-map kernels (csrc/quant_step.hip) look steps up in: float32 [2, 65] on ``device``, row 0 =
    step_size(k), row 1 = step_size(-k), column k - STEP_MIN (``step_size``: float64, rounded once)."""
    ks = range(STEP_MIN, STEP_MAX + 1)
    return torch.from_numpy(np.array([[step_size(k) for k in ks], [step_size(-k) for k in ks]], np.float32)).to(device)


def require_fp32(precision, what):
    """The refusal every quantisation-step entry point shares, raised before anything is enqueued."""
    if precision != "fp32":
        raise NotImplementedError(f"{what} runs in precision 'fp32', not {precision!r}: the pre-split dequantisation is not extended")


RDOQ_TRY_ZERO = 1                         # flags bit 0 of the RDOQ kernels: also try the symbol 0 (csrc/rdoq_rules.h)


def rdoq_weights(lam, gains, strength=1.0):
    """The per-channel weight of the RDOQ kernels, a pure function: -> float32 [c] = strength * COST_UNIT * lam * gains / 3, in
    cost_q units (2^-16 bit) per squared symbol-unit error.  J = bits / (H W) + lam * SSE / (3 H W) times COST_UNIT H W is
    cost_q + COST_UNIT lam SSE / 3, and a symbol-unit error e in channel c moves the SSE by about gains[c] e^2 step^2
    (``Model.latent_gains``: a linearisation at zero latents, cross terms ignored); with lam_i = lam / step_i^2 (``step_lambdas``)
    the step cancels, so one weight serves every step.  ValueError: a strength or lam that is not positive and finite, gains
    that are not a vector of finite non-negative numbers."""
    s, l = float(strength), float(lam)
    if not (np.isfinite(s) and s > 0):
        raise ValueError(f"rdoq: strength must be positive and finite, not {strength!r}")
    if not (np.isfinite(l) and l > 0):
        raise ValueError(f"rdoq: lambda must be positive and finite, not {lam!r}")
    g = np.asarray(gains, np.float64)
    if g.ndim != 1 or not g.size or not np.isfinite(g).all() or (g < 0).any():
        raise ValueError("rdoq: gains must be a vector of finite, non-negative numbers, one per latent channel")
    with np.errstate(over="ignore"):
        return (s * float(COST_UNIT) * l * g / 3.0).astype(np.float32)


class Rdoq:
    """What ``StepGrid.symbols`` needs to choose symbols by rate + weighted squared error instead of by distance (csrc/rdoq.hip,
    DESIGN.md 4.7 "RDOQ"): ``weight`` float32 [c] (``rdoq_weights``), ``enable`` one 0 / 1 per image (None: every image), ``zero``
    (also try the symbol 0), ``tables`` the coder's ``DeviceTables`` of the scale ladder.  Host state; the two small arrays go up
    on first use (``on``) in ONE copy.  ``changed``: int32 [n] on the device after a launch, the elements per image that were
    not written as their nearest integer."""

    def __init__(self, weight, n, tables, enable=None, zero=True):
        self.weight = np.ascontiguousarray(weight, np.float32)
        if self.weight.ndim != 1:
            raise ValueError("Rdoq: weight float32 [c], one per latent channel")
        self.n, self.tables, self.zero, self.changed, self._on = int(n), tables, bool(zero), None, None
        self.enable = check_enable(enable, self.n)

    @property
    def flags(self):
        return RDOQ_TRY_ZERO if self.zero else 0

    def set_enable(self, enable):
        """Another per-image enable list (``check_enable``); the next launch uploads it."""
        enable = check_enable(enable, self.n)
        if enable != self.enable:
            self.enable, self._on = enable, None
        return self

    def on(self, device):
        """-> (weight float32 [c], enable int32 [n]) on ``device``, uploaded once."""
        device = torch.device(device)
        if self._on is None or self._on[0] != device:
            self._on = (device, tuple(pack_upload([self.weight, np.asarray(self.enable, np.int32)], device)[1]))
        return self._on[1]


def check_enable(enable, n):
    """A per-image enable list of the RDOQ kernels -> [0 | 1] * n (None: all ones).  ValueError on another length or value."""
    if enable is None:
        return [1] * n
    vals = list(enable)
    if len(vals) != n or any(not isinstance(v, (bool, int, np.integer, np.bool_)) or int(v) not in (0, 1) for v in vals):
        raise ValueError(f"rdoq: enable must hold one 0 / 1 per image ({n}), not {enable!r}")
    return [int(v) for v in vals]


class StepGrid:
    """How y - mu of a batch of n images is quantised (csrc/quant_step.hip): ``kind`` "unit" (step 1, wire format
    3), "image" (``steps``: one ladder index per image, format 5) or "map" (``kmap``: the absolute index of every latent position,
    int8 [n, h, w], format 7).  Host state; what the kernels read goes up on first use (``on``) and stays with the object.  Every
    operation picks its kernel here, once."""

    def __init__(self, kind, n=None, steps=None, kmap=None):
        self.kind, self.n, self.steps, self.kmap, self._on = kind, n, steps, kmap, None

    @classmethod
    def image(cls, steps):
        """One ladder index per image, on the per-image kernels even where every index is 0 (a per-image ``rd_lambda``)."""
        return cls("image", len(steps), steps=[int(k) for k in steps])

    @classmethod
    def resolve(cls, step, step_offsets, n, h=None, w=None):
        """``step`` / ``step_offsets`` of the public entry points -> the grid of K = clip(step_i + step_offsets[i], STEP_MIN,
        STEP_MAX): unit where every index is 0 (or nothing is given), image where every image's K is constant, else map.
        ValueError on what ``check_steps`` / ``check_offsets`` refuse.  (h, w): the latent resolution, read with offsets only."""
        offs = None if step_offsets is None else check_offsets(step_offsets, n, h, w)
        ks = check_steps(0 if step is None else step, n)
        if offs is not None:
            kmap = index_map(ks, offs)
            ks = uniform_steps(kmap)
            if ks is None:
                return cls("map", n, kmap=kmap)
        return cls.image(ks) if any(ks) else cls("unit", n)

    @classmethod
    def from_header(cls, hd):
        """The grid a parsed header (``parse_v3`` / ``parse_v7``) announces."""
        if hd.get("kmap") is not None:
            return cls("map", hd["n"], kmap=hd["kmap"])
        return cls("unit", hd["n"]) if hd["steps"] is None else cls.image(hd["steps"])

    def indexes(self, h, w):
        """The absolute ladder index of every latent position, int8 [n, h, w]: the map, or a unit / image grid broadcast over the
        (h, w) positions it is given."""
        if self.kind == "map":
            return self.kmap
        return index_map(self.steps or [0] * self.n, np.zeros((self.n, h, w), np.int8))

    def shifted(self, d):
        """The grid of clip(k + d_i, STEP_MIN, STEP_MAX): what a file on this grid becomes when image i is requantised ``d`` =
        d_i >= 0 places up the ladder (``check_shifts``: an int or one per image).  A pure function; it collapses the way
        ``resolve`` does -- a map that comes out constant per image is an image grid, all zeros the unit grid -- so the file
        stays wire format 3, 5 or 7."""
        ds = check_shifts(d, self.n)
        if self.kind == "map":
            kmap = index_map(ds, self.kmap)
            ks = uniform_steps(kmap)
            if ks is None:
                return StepGrid("map", self.n, kmap=kmap)
        else:
            ks = [min(max(k + dd, STEP_MIN), STEP_MAX) for k, dd in zip(self.steps or [0] * self.n, ds)]
        return StepGrid.image(ks) if any(ks) else StepGrid("unit", self.n)

    def on(self, device):
        """What the kernels read, on ``device`` (one small upload, kept): image -> ``step_tensors`` = (step, inv_step, shift);
        map -> (kmap int8 [n, h, w], ``cached_step_lut``); unit -> ()."""
        device = torch.device(device)
        if self._on is None or self._on[0] != device:
            t = () if self.kind == "unit" else tuple(step_tensors(self.steps, device)) if self.kind == "image" else \
                (torch.from_numpy(self.kmap).to(device), cached_step_lut(device))
            self._on = (device, t)
        return self._on[1]

    def symbols(self, y, hyper, rdoq=None):
        """-> (y's symbols int32, their table ids).  ``rdoq`` (an ``Rdoq``): the images it enables take, per element, the
        candidate with the smallest rate + weighted squared error (csrc/rdoq.hip) and ``rdoq.changed`` counts them; the others,
        and every image without it, the nearest integer.  A unit grid then goes through the per-image kernel at step 1, shift 0."""
        if rdoq is not None:
            w, en = rdoq.on(y.device)
            if self.kind == "map":
                out = ops.rdoq_map_symbols(y, hyper, scale_table_ids(hyper), *self.on(y.device), w, en, rdoq.flags, rdoq.tables)
            else:
                t = self.on(y.device) if self.kind == "image" else self._unit_steps(y.device)
                out = ops.rdoq_symbols(y, hyper, scale_table_ids(hyper), t[1], t[2], w, en, rdoq.flags, rdoq.tables)
            rdoq.changed = out[2]
            return out[:2]
        if self.kind == "unit":
            sym = ops.entropy_scale_normal(y, hyper, want_symbols=True)[2]
            return sym, scale_table_ids(hyper)
        t = self.on(y.device)
        if self.kind == "image":
            return ops.step_symbols(y, hyper, scale_table_ids(hyper), t[1], t[2])
        return ops.step_map_symbols(y, hyper, scale_table_ids(hyper), *t)

    def _unit_steps(self, device):
        """``step_tensors`` of a unit grid (step 1, shift 0 per image), for the one kernel that has no unit form (RDOQ); kept."""
        device = torch.device(device)
        if getattr(self, "_unit_on", None) is None or self._unit_on[0] != device:
            self._unit_on = (device, tuple(step_tensors([0] * self.n, device)))
        return self._unit_on[1]

    def table_ids(self, base_ids):
        """The decoder's table ids from ``scale_table_ids``: the tables K places down the ladder, its start tables unchanged."""
        if self.kind == "unit":
            return base_ids
        t = self.on(base_ids.device)
        return step_table_ids(base_ids, t[2]) if self.kind == "image" else step_map_table_ids(base_ids, t[0])

    def dequant(self, sym, hyper, s3=False):
        """y_hat = mu + step * symbols.  ``s3`` (unit only): the synthesis takes y_hat pre-split (``takes_s3``)."""
        if self.kind == "unit":
            return ops.dequant_split3(sym, hyper) if s3 else ops.dequant_scale_normal(sym, hyper)
        t = self.on(sym.device)
        return ops.dequant_step(sym, hyper, t[0]) if self.kind == "image" else ops.dequant_step_map(sym, hyper, *t)

    def sga_fwd(self, y_loc, hyper, tau, noise, seed, step):
        if self.kind == "unit":
            return ops.sga_normal_fwd(y_loc, hyper, tau, noise, seed, step)
        t = self.on(y_loc.device)
        if self.kind == "image":
            return ops.sga_normal_step_fwd(y_loc, hyper, tau, t, noise, seed, step)
        return ops.sga_normal_step_map_fwd(y_loc, hyper, tau, *t, noise, seed, step)

    def sga_bwd(self, g_yt, sp, dv, dr, weight, dweight=None):
        """``dweight`` float32 [n] on the device (image only): what multiplies each image's distortion gradient."""
        if self.kind == "unit":
            return ops.sga_normal_bwd(g_yt, sp, dv, dr, weight)
        t = self.on(g_yt.device)
        if self.kind == "image":
            return ops.sga_normal_step_bwd(g_yt, sp, dv, dr, weight, t + (dweight,))
        return ops.sga_normal_step_map_bwd(g_yt, sp, dv, dr, weight, *t)

    def pack(self, *fields) -> bytes:
        """Everything of the blob in front of the payload; ``fields``: ``pack_v3``'s, up to the stream lengths."""
        return pack_v7(*fields, self.kmap) if self.kind == "map" else pack_v3(*fields, self.steps)

    def position_weights(self, h=None, w=None):
        """omega of ``coded_cost(weighted=True)``, float64 [n, h, w]: ``position_weights`` of the map; a unit or image grid
        broadcasts its indexes over the (h, w) positions it is given."""
        if self.kind == "map":
            return position_weights(self.kmap)
        return position_weights(index_map(self.steps or [0] * self.n, np.zeros((self.n, h, w), np.int8)))


_step_luts = {}


def cached_step_lut(device):
    """``step_lut`` on ``device``, uploaded once."""
    device = torch.device(device)
    return _step_luts[device] if device in _step_luts else _step_luts.setdefault(device, step_lut(device))


def _check_map(kmap, like, what):
    n, h, w = like.shape[:3]
    if not isinstance(kmap, torch.Tensor) or kmap.dtype != torch.int8 or tuple(kmap.shape) != (n, h, w) or not kmap.is_contiguous() \
            or kmap.device != like.device:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, f"{what}: one int8 ladder index per latent position, [{n}, {h}, {w}] on the latents' device")


def _check_lut(lut, like, what):
    if not isinstance(lut, torch.Tensor) or lut.dtype != torch.float32 or tuple(lut.shape) != (2, STEP_MAX - STEP_MIN + 1) \
            or not lut.is_contiguous() or lut.device != like.device:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, f"{what}: lut = step_lut(device)")


def step_map_table_ids(base_ids, kmap):
    """``scale_table_ids`` shifted down the ladder per POSITION: clamp(id - kmap[image, position], 0, 63); ``base_ids`` int16
    storage [n, h, w, c], ``kmap`` int8 [n, h, w] on the device.  What the decoder of a v7 blob indexes its tables with."""
    if base_ids.dtype != torch.int16 or base_ids.dim() != 4 or not base_ids.is_contiguous():
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "step_map_table_ids: contiguous int16 (uint16 storage) ids [n, h, w, c]")
    _check_map(kmap, base_ids, "step_map_table_ids")
    n, h, w, c = base_ids.shape
    out = torch.empty_like(base_ids)
    capi.call("sntc_step_map_table_ids", _p(base_ids), n, h * w, c, _p(kmap), _p(out), ops._stream())
    return out


def step_map_ladder_cost(y, hyper, base_ids, offsets, bases, tables: DeviceTables, lut=None, bases_d=None):
    """``step_ladder_cost`` over a map: candidate j prices position p at the ladder index clip(bases[j] + offsets[image, p],
    STEP_MIN, STEP_MAX); ``offsets`` int8 [n, h, w] on the device, ``bases`` ladder indexes shared by the batch.
    -> int64 [n, len(bases)] on the device, 2^-16 bit.  ``lut``: ``step_lut(device)``, ``bases_d``: ``bases`` as int32 on the device,
    if the caller keeps them (else one small upload each)."""
    _check_ladder_latents(y, hyper, base_ids, "step_map_ladder_cost")
    _check_map(offsets, y, "step_map_ladder_cost")
    bases = check_steps(list(bases), len(bases))
    if not bases:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "step_map_ladder_cost: no candidate step")
    lut = step_lut(y.device) if lut is None else lut
    _check_lut(lut, y, "step_map_ladder_cost")
    n, hw, c = y.shape[0], y.shape[1] * y.shape[2], y.shape[3]
    base_d = torch.tensor(bases, dtype=torch.int32).to(y.device) if bases_d is None else bases_d
    if base_d.dtype != torch.int32 or tuple(base_d.shape) != (len(bases),) or not base_d.is_contiguous() or base_d.device != y.device:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "step_map_ladder_cost: bases_d = the candidates as int32 on the latents' device")

    def launch(lo, k, part):
        capi.call("sntc_step_map_ladder_cost", _p(y), _p(hyper), n, hw, c, hyper.shape[-1], _p(base_ids), _p(offsets), _p(lut),
                  _p(base_d[lo:lo + k]), k, _p(tables.meta), tables.ntables, tables.total, _p(tables.cost_q), _p(part), ops._stream())
    return _ladder_cost_chunks(y, len(bases), launch)


def step_requant_ladder_cost(symbols, hyper, base_ids, src_map, shifts, tables: DeviceTables, lut=None):
    """``step_map_ladder_cost`` of a file's symbols requantised up the ladder, without y: ``symbols`` int32 [n, h, w, c] were
    quantised at the ladder indexes ``src_map`` int8 [n, h, w] (on the device); candidate j prices position p at
    clip(src_map[image, p] + shifts[j], STEP_MIN, STEP_MAX) -- ``step_map_ladder_cost(dequant_step_map(symbols, ...), ...,
    offsets=src_map, bases=shifts)``, exactly, in one pass per launch of at most ``LADDER_MAX`` candidates and without the y_hat
    tensor (csrc/quant_step.hip).  -> int64 [n, len(shifts)] on the device, 2^-16 bit."""
    shifts = check_shifts(list(shifts), len(shifts))
    if not shifts:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "step_requant_ladder_cost: no candidate shift")
    lut = cached_step_lut(symbols.device) if lut is None else lut
    shifts_d = torch.tensor(shifts, dtype=torch.int32).to(symbols.device)

    def launch(lo, k, part):
        ops.step_requant_ladder_cost(symbols, hyper, base_ids, src_map, lut, shifts_d[lo:lo + k], tables, out=part)
    return _ladder_cost_chunks(symbols, len(shifts), launch)


def channel_table_ids(shape, device):
    n, h, w, c = shape
    tid = torch.empty((n, h, w, c), dtype=torch.int16, device=device)
    capi.call("sntc_channel_table_ids", n * h * w, c, _p(tid), ops._stream())
    return tid


def round_to_int(x):
    out = torch.empty(x.shape, dtype=torch.int32, device=x.device)
    capi.call("sntc_round_to_int", _p(x), x.numel(), _p(out), ops._stream())
    return out


def int_to_float(x):
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    capi.call("sntc_int_to_float", _p(x), x.numel(), _p(out), ops._stream())
    return out


# -- wire formats v3 / v5 / v7: pure host functions (numbers in, numbers out; no device) ----------------------------------------
HEAD_V3 = "<HHIIHHHHHHHHBB"               # version | n | H | W | C | Cz | hz | wz | h | w | segments_z | segments_y | lanes_z | lanes_y


def pack_v3(arith, n, H, W, dims, sz, sy, lz, ly, zl, yl, steps=None) -> bytes:
    """Everything of a hyperprior blob in front of the payload.  ``dims`` = (C, Cz, hz, wz, h, w); ``steps``: one ladder index
    per image, or None.  With every index 0 (or None) this is the v3 header; else version 5: the same header with version
    byte 5, then the n indexes as signed bytes, then the length fields."""
    c, cz, hz, wz, h, w = dims
    steps = [0] * n if steps is None else check_steps(list(steps), n)
    stepped = any(steps)
    head = MAGIC + struct.pack(HEAD_V3, (VERSION_STEP if stepped else VERSION) | (arith << 8), n, H, W, c, cz, hz, wz, h, w, sz, sy, lz, ly)
    if stepped:
        head += np.asarray(steps, np.int8).tobytes()
    return head + np.asarray(zl, np.int64).astype("<u4").tobytes() + np.asarray(yl, np.int64).astype("<u4").tobytes()


def _parse_head(blob, precision, latent_shapes, versions):
    """The checks every hyperprior format shares, up to the end of the fixed header: magic, version (one of ``versions``),
    arithmetic, and every dimension recomputed from (H, W) and the decoding model.  -> (version byte, dict of the fields, pos)."""
    if blob[:4] != MAGIC:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "not an SNTC bitstream")
    pos = 4 + struct.calcsize(HEAD_V3)
    if len(blob) < pos:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "bitstream truncated")
    ver, n, H, W, c, cz, hz, wz, h, w, sz, sy, lz, ly = struct.unpack_from(HEAD_V3, blob, 4)
    arith, ver = ver >> 8, ver & 0xff
    if ver not in versions:
        raise capi.SntcError(capi.ERR_UNSUPPORTED, f"bitstream version {ver}")
    if arith != ARITH[precision]:
        names = {v: k for k, v in ARITH.items()}
        raise capi.SntcError(capi.ERR_UNSUPPORTED, f"bitstream was written by a {names.get(arith, arith)!r} model, this model "
                             f"computes in {precision!r}: mu / sigma would not be reproduced bit for bit")
    # Every dimension is recomputed from (H, W) and THIS model, so a corrupt or crafted blob cannot size an allocation or
    # index a table-id tensor beyond what the model itself would produce.
    if not (1 <= n <= Codec.MAX_IMAGES and 1 <= H <= Codec.MAX_SIDE and 1 <= W <= Codec.MAX_SIDE):
        raise capi.SntcError(capi.ERR_BAD_SHAPE, f"bitstream header: implausible batch / image size n={n} H={H} W={W}")
    want = tuple(int(v) for v in latent_shapes(H, W))
    if (c, cz, hz, wz, h, w) != want:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, f"bitstream header (C, Cz, hz, wz, h, w) = {(c, cz, hz, wz, h, w)} does not match "
                             f"this model's latents for a {H} x {W} image: {want}")
    ez, ey = hz * wz * cz, h * w * c
    if (sz, sy) != (_segments(ez), _segments(ey)) or (lz, ly) != (_lanes(-(-ez // sz)), _lanes(-(-ey // sy))):
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "bitstream header: segment / lane counts do not match the latent sizes")
    return ver, dict(n=n, H=H, W=W, c=c, cz=cz, hz=hz, wz=wz, h=h, w=w, sz=sz, sy=sy, lz=lz, ly=ly), pos


def _parse_lengths(blob, hd, pos):
    """The length fields at ``pos`` and the payload they announce: the blob must end where its streams do.  Fills zl, yl, pos
    (= payload offset), zw, yw of ``hd``."""
    nz, ny = hd["n"] * hd["sz"], hd["n"] * hd["sy"]
    if len(blob) < pos + 4 * (nz + ny):
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "bitstream truncated")
    zl = np.frombuffer(blob, "<u4", nz, pos).astype(np.int64)
    yl = np.frombuffer(blob, "<u4", ny, pos + 4 * nz).astype(np.int64)
    pos += 4 * (nz + ny)
    zw, yw = int(zl.sum()), int(yl.sum())
    if len(blob) != pos + 2 * (zw + yw):
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "bitstream truncated")
    hd.update(zl=zl, yl=yl, pos=pos, zw=zw, yw=yw)
    return hd


def parse_v3(blob: bytes, precision, latent_shapes):
    """Header and stream lengths of one v3 / v5 blob, checked against the decoding model: ``precision`` its arithmetic,
    ``latent_shapes(H, W) -> (C, Cz, hz, wz, h, w)`` its latents for an H x W image.  -> dict(..., steps = the n ladder indexes of
    a v5 blob or None, pos = payload offset)."""
    ver, hd, pos = _parse_head(blob, precision, latent_shapes, (VERSION, VERSION_STEP))
    n = hd["n"]
    steps = None
    if ver == VERSION_STEP:
        if len(blob) < pos + n:
            raise capi.SntcError(capi.ERR_BAD_SHAPE, "bitstream truncated")
        steps = np.frombuffer(blob, np.int8, n, pos).astype(np.int64).tolist()
        pos += n
        if not all(STEP_MIN <= k <= STEP_MAX for k in steps):
            raise capi.SntcError(capi.ERR_BAD_SHAPE, f"bitstream header: quantisation step index outside [{STEP_MIN}, {STEP_MAX}]")
    hd = _parse_lengths(blob, hd, pos)
    hd["steps"] = steps
    return hd


def pack_v7(arith, n, H, W, dims, sz, sy, lz, ly, zl, yl, kmap) -> bytes:
    """Everything of a hyperprior blob in front of the payload when the ladder index varies per position: ``kmap`` int8
    [n, h, w], absolute indexes.  Wire format 7 = the v3 header with version byte 7 | u32 record count | the records of
    ``pack_runs`` | the v3 length fields.  The writer is canonical: where every image's map is constant this is ``pack_v3`` of
    those indexes (v5; v3 if all are 0), byte for byte -- version 7 appears only for a map that really varies."""
    c, cz, hz, wz, h, w = dims
    kmap = np.asarray(kmap)
    if kmap.dtype != np.int8 or kmap.shape != (n, h, w):
        raise ValueError(f"pack_v7: kmap int8 {(n, h, w)}")
    records = pack_runs(kmap.reshape(n, h * w))                      # ValueError on an index outside the ladder
    steps = uniform_steps(kmap)
    if steps is not None:
        return pack_v3(arith, n, H, W, dims, sz, sy, lz, ly, zl, yl, steps)
    head = MAGIC + struct.pack(HEAD_V3, VERSION_MAP | (arith << 8), n, H, W, c, cz, hz, wz, h, w, sz, sy, lz, ly)
    head += struct.pack("<I", len(records) // RUN_RECORD.itemsize) + records
    return head + np.asarray(zl, np.int64).astype("<u4").tobytes() + np.asarray(yl, np.int64).astype("<u4").tobytes()


def parse_v7(blob: bytes, precision, latent_shapes):
    """``parse_v3`` for a v7 blob: the same header, arithmetic and shape checks, then the step map.  Refused with ERR_BAD_SHAPE:
    a record count above n h w, a short blob ("truncated"), and what ``parse_runs`` refuses.  -> the ``parse_v3`` dict with
    steps = None and kmap = int8 [n, h, w]."""
    _, hd, pos = _parse_head(blob, precision, latent_shapes, (VERSION_MAP,))
    n, h, w = hd["n"], hd["h"], hd["w"]
    if len(blob) < pos + 4:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "bitstream truncated")
    (count,) = struct.unpack_from("<I", blob, pos)
    pos += 4
    if count > n * h * w:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, f"bitstream header: step map of {count} records for {n * h * w} positions")
    size = count * RUN_RECORD.itemsize
    if len(blob) < pos + size:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "bitstream truncated")
    kmap = parse_runs(blob[pos:pos + size], n, h * w).reshape(n, h, w)
    hd = _parse_lengths(blob, hd, pos + size)
    hd.update(steps=None, kmap=np.ascontiguousarray(kmap))
    return hd


# -- the coded pixel residual layer, wire format 8 (csrc/residual.hip, DESIGN.md 4.7 "residual layer") ---------------------------
VERSION_RESIDUAL = 8                      # a complete v3 / v5 / v7 blob + the coded residual of its decoded picture
RESIDUAL_LEVELS, RESIDUAL_BINS, RESIDUAL_MAX_ERROR = 8, 511, 127
RESIDUAL_CHANNELS = 3                     # the pictures a file holds are RGB: 8 levels x 3 channels = 24 classes per image
RESIDUAL_ELEMS_PER_SEGMENT = 1 << 16      # one rANS stream per this many pixel values: 256 bytes of lane states = 0.03 bit / value,
                                          # and 1024 decode steps per stream instead of the latents' 4096 (a step is a latency)
RESIDUAL_MAX_ELEMS = (1 << 31) - 1        # values of one image the kernels index with 32 bits
RESIDUAL_THREADS, RESIDUAL_VEC, RESIDUAL_GRID = 256, 4, 768   # csrc/residual.hip: a workgroup takes 256 units of 4 values (1 where
                                          # a pointer or the image size is not a multiple of 4) per pass, about 768 workgroups a launch
HEAD_V8 = "<HBBI"                         # version | max_error | levels | base_len
TAIL_V8 = "<HBB"                          # segments | lanes | 0


def check_max_error(max_error):
    """``max_error`` of the public entry points -> int in [0, RESIDUAL_MAX_ERROR]; ValueError on anything else."""
    if isinstance(max_error, bool) or not isinstance(max_error, (int, np.integer)) or not 0 <= int(max_error) <= RESIDUAL_MAX_ERROR:
        raise ValueError(f"max_error must be an int in [0, {RESIDUAL_MAX_ERROR}], not {max_error!r}")
    return int(max_error)


def residual_streams(H, W, c=RESIDUAL_CHANNELS):
    """(segments, lanes) of the residual streams of one H x W image: cut every ``RESIDUAL_ELEMS_PER_SEGMENT`` values."""
    e = int(H) * int(W) * int(c)
    segments = _segments(e, -(-e // RESIDUAL_ELEMS_PER_SEGMENT))
    return segments, _lanes(-(-e // segments))


def residual_prices(tabs):
    """What q = -255 .. 255 costs under each of the first 64 tables of ``tabs``: int64 [64, 511] in 2^-16 bit, entry [t, q + 255] =
    ``cost_table`` at the symbol the encoder codes (q - lo where that is a real symbol of the table, else ESCAPE)."""
    q = np.arange(-(RESIDUAL_BINS // 2), RESIDUAL_BINS // 2 + 1, dtype=np.int64)
    out = np.empty((NUM_SCALES, RESIDUAL_BINS), np.int64)
    for t, (lo, f) in enumerate(tabs[:NUM_SCALES]):
        cost = cost_table([(lo, f)]).astype(np.int64)
        sym = q - int(lo)
        out[t] = cost[np.where((sym < 0) | (sym >= len(f) - 1), len(f) - 1, sym)]
    return out


def residual_choice(hist, tabs):
    """The table of every (image, class), a pure function: ``hist`` [n, classes, 511] = how many values of the class took
    q = bin - 255 (``sntc_residual_quantize``), ``tabs`` the model's normal tables (``normal_tables()``).  Per (image, class) the
    table with the smallest exact coded cost of the class's values (``residual_prices``: the encoder's ESCAPE rule), the lower
    index on a tie, table 0 for an empty class.  -> (choice uint8 [n, classes], cost_q int64 [n] = the chosen tables' cost summed
    over the image's classes, 2^-16 bit: what ``rans_cost`` returns for the image's q under the ids of the choice)."""
    h = np.asarray(hist)
    if h.ndim != 3 or h.shape[2] != RESIDUAL_BINS or not np.issubdtype(h.dtype, np.integer) or len(tabs) < NUM_SCALES:
        raise ValueError(f"residual_choice: integer counts [n, classes, {RESIDUAL_BINS}] and the {NUM_SCALES} normal tables")
    total = h.astype(np.int64) @ residual_prices(tabs).T             # [n, classes, 64], exact: integer matmul
    choice = total.argmin(axis=2)                                    # the first minimum: the lower index on a tie
    return choice.astype(np.uint8), total.min(axis=2).sum(axis=1).astype(np.int64)


def _base_dims(base_blob):
    """(version byte, arithmetic tag, n, H, W) of a hyperprior blob's fixed header; the blob is at least that long."""
    word, n, H, W = struct.unpack_from("<HHII", base_blob, 4)
    return word & 0xff, word >> 8, n, H, W


def pack_v8(arith, max_error, base_blob, segments, lanes, choice, len_words) -> bytes:
    """Everything of a v8 blob in front of its payload: b"SNTC" | u16 version (low byte 8, high byte the arithmetic tag) |
    u8 max_error | u8 levels = 8 | u32 base_len | the base file, a complete v3 / v5 / v7 blob, unchanged | u16 segments | u8 lanes |
    u8 0 | choice[n 8 3] | u32 len_words[n segments].  ValueError on what ``split_residual`` would refuse in the result."""
    max_error = check_max_error(max_error)
    base_blob = bytes(base_blob)
    if len(base_blob) < 4 + struct.calcsize(HEAD_V3) or base_blob[:4] != MAGIC:
        raise ValueError("pack_v8: the base is not an SNTC bitstream")
    ver, tag, n, H, W = _base_dims(base_blob)
    if ver not in (VERSION, VERSION_STEP, VERSION_MAP) or tag != arith:
        raise ValueError(f"pack_v8: the base must be a v3 / v5 / v7 blob of the same arithmetic, not version {ver} tag {tag}")
    choice = np.asarray(choice)
    len_words = np.asarray(len_words, np.int64)
    if choice.dtype != np.uint8 or choice.shape != (n, RESIDUAL_LEVELS * RESIDUAL_CHANNELS) or (choice.size and int(choice.max()) >= NUM_SCALES):
        raise ValueError(f"pack_v8: choice uint8 {(n, RESIDUAL_LEVELS * RESIDUAL_CHANNELS)} of table indexes below {NUM_SCALES}")
    if (segments, lanes) != residual_streams(H, W) or len(len_words) != n * segments:
        raise ValueError("pack_v8: segment / lane / stream counts do not match the image size")
    return MAGIC + struct.pack(HEAD_V8, VERSION_RESIDUAL | (arith << 8), max_error, RESIDUAL_LEVELS, len(base_blob)) + base_blob + \
        struct.pack(TAIL_V8, segments, lanes, 0) + choice.tobytes() + len_words.astype("<u4").tobytes()


def is_residual(blob) -> bool:
    """Whether ``blob`` announces wire format 8 (its version byte; nothing else is checked)."""
    return len(blob) > 4 and blob[:4] == MAGIC and blob[4] == VERSION_RESIDUAL


def split_residual(blob):
    """A v8 blob -> (its base file, a complete v3 / v5 / v7 blob, byte for byte; info = dict(arith, max_error, n, H, W, segments,
    lanes, choice uint8 [n, 24], lens int64 [n segments], pos = payload offset, words)).  A pure host function: n, H, W come
    from the base header, segments and lanes are recomputed from them and compared, the total length must match exactly; no
    header field sizes an allocation.  Refused (SntcError): a choice byte >= 64, max_error > 127, levels != 8, a nested v8 base,
    a v4 base, a short blob, a trailing byte.  The base's own checks are its decoder's (``parse_v3`` / ``parse_v7``)."""
    bad = lambda what: capi.SntcError(capi.ERR_BAD_SHAPE, f"bitstream header: residual layer {what}")
    blob = bytes(blob)
    if blob[:4] != MAGIC:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "not an SNTC bitstream")
    pos = 4 + struct.calcsize(HEAD_V8)
    if len(blob) < pos:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "bitstream truncated")
    word, max_error, levels, base_len = struct.unpack_from(HEAD_V8, blob, 4)
    if word & 0xff != VERSION_RESIDUAL:
        raise capi.SntcError(capi.ERR_UNSUPPORTED, f"bitstream version {word & 0xff}: split_residual reads version {VERSION_RESIDUAL}")
    if max_error > RESIDUAL_MAX_ERROR:
        raise bad(f"max_error {max_error} above {RESIDUAL_MAX_ERROR}")
    if levels != RESIDUAL_LEVELS:
        raise bad(f"of {levels} levels, not {RESIDUAL_LEVELS}")
    if base_len < 4 + struct.calcsize(HEAD_V3) or len(blob) < pos + base_len + struct.calcsize(TAIL_V8):
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "bitstream truncated")
    base_blob = blob[pos:pos + base_len]
    pos += base_len
    if base_blob[:4] != MAGIC:
        raise bad("holds no SNTC bitstream as its base")
    ver, tag, n, H, W = _base_dims(base_blob)
    if ver not in (VERSION, VERSION_STEP, VERSION_MAP):
        raise capi.SntcError(capi.ERR_UNSUPPORTED, f"bitstream header: residual layer over a version {ver} base; a base is version "
                             f"{VERSION}, {VERSION_STEP} or {VERSION_MAP}")
    if tag != word >> 8:
        raise bad("and its base name different arithmetics")
    if not (1 <= n <= Codec.MAX_IMAGES and 1 <= H <= Codec.MAX_SIDE and 1 <= W <= Codec.MAX_SIDE) or H * W * RESIDUAL_CHANNELS > RESIDUAL_MAX_ELEMS:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, f"bitstream header: implausible batch / image size n={n} H={H} W={W}")
    segments, lanes, zero = struct.unpack_from(TAIL_V8, blob, pos)
    pos += struct.calcsize(TAIL_V8)
    if (segments, lanes) != residual_streams(H, W) or zero != 0:
        raise bad("segment / lane counts do not match the image size")
    ncls, ns = n * RESIDUAL_LEVELS * RESIDUAL_CHANNELS, n * segments
    if len(blob) < pos + ncls + 4 * ns:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "bitstream truncated")
    choice = np.frombuffer(blob, np.uint8, ncls, pos).reshape(n, -1).copy()        # ncls bytes the blob was just found to hold
    if int(choice.max()) >= NUM_SCALES:
        raise bad(f"names table {int(choice.max())}; the model has {NUM_SCALES}")
    lens = np.frombuffer(blob, "<u4", ns, pos + ncls).astype(np.int64)
    pos += ncls + 4 * ns
    words = int(lens.sum())
    if len(blob) != pos + 2 * words:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "bitstream truncated" if len(blob) < pos + 2 * words else
                             "bitstream header: residual layer is followed by bytes it does not announce")
    return base_blob, dict(arith=tag, max_error=max_error, n=n, H=H, W=W, segments=segments, lanes=lanes, choice=choice, lens=lens,
                           pos=pos, words=words)


def parse_v8(blob: bytes, precision, latent_shapes):
    """``split_residual`` + the base's own parse against the decoding model (``parse_v3`` / ``parse_v7``: arithmetic, every
    dimension recomputed).  -> (base_blob, the base's header dict, the layer's info dict)."""
    base_blob, info = split_residual(blob)
    mapped = base_blob[4] == VERSION_MAP
    return base_blob, (parse_v7 if mapped else parse_v3)(base_blob, precision, latent_shapes), info


def _check_residual_images(base, what, other=None, dtype=None):
    """The checks the three kernels' wrappers share: ``base`` uint8 [n, h, w, c] contiguous; ``other`` of ``dtype`` like it."""
    if not isinstance(base, torch.Tensor) or base.dtype != torch.uint8 or base.dim() != 4 or not base.is_contiguous():
        raise capi.SntcError(capi.ERR_BAD_SHAPE, f"{what}: base is a contiguous uint8 tensor [n, h, w, c]")
    if other is not None and (not isinstance(other, torch.Tensor) or other.dtype != dtype or tuple(other.shape) != tuple(base.shape)
                              or not other.is_contiguous() or other.device != base.device):
        raise capi.SntcError(capi.ERR_BAD_SHAPE, f"{what}: a contiguous {dtype} tensor of base's shape {tuple(base.shape)} on its device")


def residual_quantize(x, base, max_error):
    """``sntc_residual_quantize``: x float32 [n, h, w, c] (image values, -0.5 .. 0.5), base uint8 like it -> (q int32 like x,
    hist int32 storage of uint32 [n, 8 c, 511]: the counts of q + 255 per (image, class)).  No host synchronisation."""
    _check_residual_images(base, "residual_quantize", x, torch.float32)
    n, h, w, c = base.shape
    q = torch.empty(tuple(base.shape), dtype=torch.int32, device=base.device)
    hist = torch.empty((n, RESIDUAL_LEVELS * c, RESIDUAL_BINS), dtype=torch.int32, device=base.device)
    capi.call("sntc_residual_quantize", _p(x), _p(base), n, h, w, c, int(max_error), _p(q), _p(hist), ops._stream())
    return q, hist


def residual_table_ids(base, choice):
    """``sntc_residual_table_ids``: base uint8 [n, h, w, c], choice uint8 [n, 8 c] on its device -> ids int16 storage of uint16
    like base: the chosen table of every value's class."""
    _check_residual_images(base, "residual_table_ids")
    n, h, w, c = base.shape
    if not isinstance(choice, torch.Tensor) or choice.dtype != torch.uint8 or tuple(choice.shape) != (n, RESIDUAL_LEVELS * c) \
            or not choice.is_contiguous() or choice.device != base.device:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, f"residual_table_ids: choice uint8 {(n, RESIDUAL_LEVELS * c)} on base's device")
    ids = torch.empty(tuple(base.shape), dtype=torch.int16, device=base.device)
    capi.call("sntc_residual_table_ids", _p(base), _p(choice), n, h, w, c, _p(ids), ops._stream())
    return ids


def residual_apply(base, q, max_error, count=None):
    """``sntc_residual_apply``: base uint8 [n, h, w, c], q int32 like it -> (x~ uint8 like base, count int32 [1] on the device:
    the values of q no encoder writes at this ``max_error``; ``count``: where to leave it, zeroed by the call).  No host
    synchronisation."""
    _check_residual_images(base, "residual_apply", q, torch.int32)
    n, h, w, c = base.shape
    if count is None:
        count = torch.empty((1,), dtype=torch.int32, device=base.device)
    out = torch.empty_like(base)
    capi.call("sntc_residual_apply", _p(base), _p(q), n, h, w, c, int(max_error), _p(out), _p(count), ops._stream())
    return out, count


class Codec:
    """compress / decompress for a mean-scale hyperprior ``Model``."""

    HEAD = HEAD_V3
    MAX_IMAGES, MAX_SIDE = 4096, 1 << 16

    def __init__(self, model):
        self.m = model
        self.last_decompress_report = None
        dev = model.device
        nl = len(model._prior_num_filters) + 1
        with torch.cuda.device(dev):
            self.y_tables = DeviceTables(normal_tables(), dev)
            self.z_tables = DeviceTables(factorized_tables(model._prior_weights, nl), dev)

    def latent_shapes(self, H, W):
        """(C, Cz, hz, wz, h, w) of this model's latents for an H x W image (pad to the downsample factor, then the
        transforms' own shape arithmetic)."""
        m = self.m
        f = m.downsample_factor
        hp, wp = -(-H // f) * f, -(-W // f) * f
        h, w = m._analysis.out_hw(hp, wp)
        hz, wz = m._hyper_analysis.out_hw(h, w)
        return (m._bottleneck_size, m._hyper_bottleneck_size, hz, wz, h, w)

    def _check_latents(self, z, y, image_hw):
        H, W = int(image_hw[0]), int(image_hw[1])
        c, cz, hz, wz, h, w = self.latent_shapes(H, W)
        n = z.shape[0]
        if tuple(z.shape) != (n, hz, wz, cz) or tuple(y.shape) != (n, h, w, c):
            raise capi.SntcError(capi.ERR_BAD_SHAPE, f"latents {tuple(z.shape)} / {tuple(y.shape)} are not this model's for {n} images of "
                                 f"{H} x {W}: {(n, hz, wz, cz)} / {(n, h, w, c)}")
        return n, H, W

    def _grid(self, step, step_offsets, n, H, W):
        """``step`` / ``step_offsets`` of the public entry points -> their ``StepGrid`` (``StepGrid.resolve`` at this model's latent
        resolution).  Every refusal here: before anything is enqueued."""
        h, w = (None, None) if step_offsets is None else self.latent_shapes(H, W)[4:]
        grid = StepGrid.resolve(step, step_offsets, n, h, w)
        if step is not None or step_offsets is not None:
            require_fp32(self.m._precision, "a quantisation step")
        return grid

    def _hyper_of(self, z):
        """z_loc -> (zi int32, the hyper-synthesis of it): what every step shares."""
        zi = round_to_int(z)
        return zi, self.m._hyper_synthesis(int_to_float(zi))

    def _symbols(self, z, y, grid, pre=None, rdoq=None):
        """(z_loc, y_loc) -> what the file carries: (zi int32, z's table ids, y symbols int32, y's table ids, hyper).
        ``grid``: the ``StepGrid`` y - mu is quantised on; ``pre``: ``_hyper_of(z)`` if the caller has it; ``rdoq``: an ``Rdoq``
        (``self.rdoq``) -- the images it enables are quantised by rate + distortion (``StepGrid.symbols``)."""
        m = self.m
        grid.on(m.device)                                          # its upload, if any, before anything is enqueued
        if rdoq is not None:
            rdoq.on(m.device)
            if grid.kind == "unit":
                grid._unit_steps(m.device)
        zi, hyper = self._hyper_of(z) if pre is None else pre
        ztid = channel_table_ids(z.shape, m.device)
        sym, ytid = grid.symbols(y, hyper) if rdoq is None else grid.symbols(y, hyper, rdoq)
        return zi, ztid, sym, ytid, hyper

    def rdoq(self, weight, n, enable=None, zero=True):
        """The ``Rdoq`` of this codec's y tables for a batch of n images: ``weight`` float32 [C] (``rdoq_weights``), ``enable``
        one 0 / 1 per image (None: all), ``zero``: also try the symbol 0.  ValueError on a weight that is not one per channel."""
        r = Rdoq(weight, n, self.y_tables, enable, zero)
        if r.weight.shape != (self.m._bottleneck_size,):
            raise ValueError(f"rdoq: {r.weight.shape} weights for {self.m._bottleneck_size} latent channels")
        return r

    def _rdoq_of(self, rdoq, rdoq_enable, n):
        """``rdoq`` / ``rdoq_enable`` of the public entry points -> the ``Rdoq`` to launch with, or None.  Every refusal here:
        before anything is enqueued."""
        if rdoq is None:
            if rdoq_enable is not None:
                raise ValueError("rdoq_enable needs rdoq")
            return None
        if not isinstance(rdoq, Rdoq) or rdoq.n != n:
            raise ValueError(f"rdoq: an entropy_coding.Rdoq for {n} images (Codec.rdoq)")
        require_fp32(self.m._precision, "rate-distortion optimised quantisation")
        return rdoq if rdoq_enable is None else rdoq.set_enable(rdoq_enable)

    def _launch_latents(self, z, y, image_hw, grid, pre=None, rdoq=None):
        """The device half of ``compress_latents`` on the current stream, no host synchronisation.  ``grid`` travels in the
        file; ``rdoq`` as in ``_symbols``: nothing of it travels, the file is that of its symbols."""
        n, H, W = self._check_latents(z, y, image_hw)
        zi, ztid, sym, ytid, _ = self._symbols(z, y, grid, pre, rdoq)
        sz, sy = _segments(zi[0].numel()), _segments(sym[0].numel())
        lz, ly = _lanes(-(-zi[0].numel() // sz)), _lanes(-(-sym[0].numel() // sy))
        dims = (y.shape[-1], z.shape[-1], z.shape[1], z.shape[2], y.shape[1], y.shape[2])
        groups = [rans_encode_launch(zi, ztid, self.z_tables, sz, lz), rans_encode_launch(sym, ytid, self.y_tables, sy, ly)]
        return dict(n=n, H=H, W=W, dims=dims, sz=sz, sy=sy, lz=lz, ly=ly, groups=groups, grid=grid)

    def _launch(self, x):
        """analysis -> ``_launch_latents`` on the unit grid."""
        lat = self.m.infer_latent_rvs(x)
        return self._launch_latents(lat.uq[0].loc, lat.uq[1].loc, x.shape[1:3], StepGrid("unit", x.shape[0]))

    def _finish(self, jobs):
        """Launched jobs -> their blobs (``finish_streams``: two read-backs for all of them).  ``dims``: the header's (C, Cz, hz,
        wz, h, w).  A job of ``transcode_many`` has one coded group, y: its z streams are copied -- ``copied`` = (their lengths,
        their words) as the source blob holds them."""
        out = []
        for j, done in zip(jobs, finish_streams([j["groups"] for j in jobs])):
            (zl, zwords), (yl, ywords) = [j["copied"]] + done if "copied" in j else done
            fields = (ARITH[self.m._precision], j["n"], j["H"], j["W"], j["dims"], j["sz"], j["sy"], j["lz"], j["ly"], zl, yl)
            out.append(j["grid"].pack(*fields) + zwords.tobytes() + ywords.tobytes())
        return out

    def compress_latents(self, z_loc, y_loc, image_hw, step=None, step_offsets=None, rdoq=None, rdoq_enable=None) -> bytes:
        """Latents of this model for images of ``image_hw`` = (H, W) -- the encoder's, or ones refined by iterative inference --
        -> the bitstream ``decompress`` reads: z is rounded, the hyper-synthesis gives mu / the scale indexes, y - mu is rounded,
        both are coded.  ``compress(x)`` is this on ``infer_latent_rvs(x)``.  ``step``: an index on the scale ladder, or one per
        image: y - mu is quantised with the step ``step_size(k)`` and coded with the tables k places down the ladder (wire
        format 5; with every index 0 the v3 blob of ``step=None``, byte for byte).  ``step_offsets``: integers [n, h, w] at latent
        resolution, added to the image's step per position and clipped to the ladder (wire format 7 where the result varies
        inside an image; a constant result is the v5 / v3 blob of those indexes, byte for byte).  ``rdoq`` (``self.rdoq(...)``):
        the symbols of the images it enables are chosen by rate + weighted squared error (csrc/rdoq.hip) -- the same wire
        format, read by the same decoder; ``rdoq_enable``: one 0 / 1 per image instead of its own list.  ``rdoq.changed``
        then counts, per image, the symbols that are not the nearest integer."""
        m = self.m
        grid = self._grid(step, step_offsets, z_loc.shape[0], int(image_hw[0]), int(image_hw[1]))
        rdoq = self._rdoq_of(rdoq, rdoq_enable, z_loc.shape[0])
        with torch.cuda.device(m.device):
            return self._finish([self._launch_latents(z_loc.contiguous(), y_loc.contiguous(), image_hw, grid, rdoq=rdoq)])[0]

    def latents_cost(self, z_loc, y_loc, x, step=None, step_offsets=None, rdoq=None, rdoq_enable=None, pre=None):
        """What ``compress_latents`` would write for these latents and what ``decompress`` would make of it, without writing it:
        -> (cost_z, cost_y int64 [n] in 2^-16 bit (``rans_cost``), uint8 pixels, integer SSE [n] against ``x``), all on the
        device, no host synchronisation.  ``step`` / ``step_offsets`` / ``rdoq`` / ``rdoq_enable`` as in ``compress_latents``
        (``rdoq.changed``: int32 [n] on the device afterwards).  ``pre``: ``_hyper_of(z_loc)`` if the caller has it."""
        m = self.m
        n, H, W = self._check_latents(z_loc, y_loc, x.shape[1:3])
        grid = self._grid(step, step_offsets, n, H, W)
        rdoq = self._rdoq_of(rdoq, rdoq_enable, n)
        zi, ztid, sym, ytid, hyper = self._symbols(z_loc.contiguous(), y_loc.contiguous(), grid, pre, rdoq)
        cost_z, cost_y = rans_cost(zi, ztid, self.z_tables), rans_cost(sym, ytid, self.y_tables)
        y_hat = grid.dequant(sym, hyper, m._synthesis.takes_s3(sym.shape[1], sym.shape[2]))
        px, sse = m._pixels(y_hat, (H, W), x)                     # the decoder's own steps from the symbols on
        return cost_z, cost_y, px, sse

    def _ladder(self, z, y, steps, pre=None, offsets=None):
        dev = self.m.device
        zi, hyper = self._hyper_of(z) if pre is None else pre
        cost_z = rans_cost(zi, channel_table_ids(z.shape, dev), self.z_tables)
        if offsets is None:
            cost_y = step_ladder_cost(y, hyper, scale_table_ids(hyper), steps, self.y_tables, step_tensors(steps, dev))
        else:
            cost_y = step_map_ladder_cost(y, hyper, scale_table_ids(hyper), torch.from_numpy(offsets).to(dev), steps, self.y_tables,
                                          cached_step_lut(dev))
        return cost_z, cost_y

    def ladder_cost(self, z_loc, y_loc, image_hw, steps, step_offsets=None):
        """``latents_cost``'s (cost_z, cost_y) at EVERY ladder index of ``steps`` without forming a symbol tensor: -> (cost_z
        int64 [n], cost_y int64 [n, len(steps)]) in 2^-16 bit on the device, no host synchronisation.  y, mu and the scale
        indexes are read once per launch of at most ``LADDER_MAX`` candidates (csrc/quant_step.hip).  ``step_offsets`` (integers
        [n, h, w]): candidate j prices position p at clip(steps[j] + step_offsets[i, p]) -- what ``latents_cost(step=steps[j],
        step_offsets=...)`` returns (csrc/quant_step.hip)."""
        steps = check_steps(list(steps), len(steps))
        if not steps:
            raise ValueError("ladder_cost: no candidate step")
        require_fp32(self.m._precision, "a quantisation step")
        n, H, W = self._check_latents(z_loc, y_loc, image_hw)
        offsets = None if step_offsets is None else check_offsets(step_offsets, n, *y_loc.shape[1:3])
        with torch.cuda.device(self.m.device):
            return self._ladder(z_loc.contiguous(), y_loc.contiguous(), steps, offsets=offsets)

    def ladder_distortion(self, z_loc, y_loc, x, steps, step_offsets=None, chunk_bytes=LADDER_DECODE_BYTES, pre=None):
        """``latents_cost``'s integer SSE at EVERY ladder index of ``steps``: -> int64 [n, len(steps)] on the device, no host
        synchronisation; column j is what ``latents_cost(z_loc, y_loc, x, step=steps[j], step_offsets=...)`` returns, exactly
        (decoding is batch-invariant and the step rule is one header: the decoded SSE of a candidate is a well-defined integer).
        The hyper-synthesis runs once; the candidates go through in chunks of min(LADDER_MAX, max(1, ``chunk_bytes`` // the
        bytes of one candidate's y_hat)): per chunk ONE launch of csrc/quant_step.hip writes the dequantised latents of
        its candidates, candidate-major, and ONE decoder batch of chunk n latents decodes them against the images repeated on
        the device.  ``chunk_bytes`` bounds memory only: the result does not depend on it.  ``pre``: ``_hyper_of(z_loc)`` if
        the caller has it."""
        m = self.m
        steps = check_steps(list(steps), len(steps))
        if not steps:
            raise ValueError("ladder_distortion: no candidate step")
        require_fp32(m._precision, "a quantisation step")
        n, H, W = self._check_latents(z_loc, y_loc, x.shape[1:3])
        offsets = None if step_offsets is None else check_offsets(step_offsets, n, *y_loc.shape[1:3])
        with torch.cuda.device(m.device):
            y = y_loc.contiguous()
            _, hyper = self._hyper_of(z_loc.contiguous()) if pre is None else pre
            chunk = min(LADDER_MAX, max(1, int(chunk_bytes) // (4 * y.numel())))
            if offsets is None:
                st, inv, _ = step_tensors(steps, m.device)
            else:
                off_d, bases = torch.from_numpy(offsets).to(m.device), torch.tensor(steps, dtype=torch.int32).to(m.device)
                lut = cached_step_lut(m.device)
            sse = torch.empty((n, len(steps)), dtype=torch.int64, device=m.device)
            for lo in range(0, len(steps), chunk):
                k = min(chunk, len(steps) - lo)
                if offsets is None:
                    y_hat = ops.step_ladder_dequant(y, hyper, inv[lo:lo + k], st[lo:lo + k])
                else:
                    y_hat = ops.step_map_ladder_dequant(y, hyper, off_d, lut, bases[lo:lo + k])
                _, part = m._pixels(y_hat.view((k * n,) + tuple(y.shape[1:])), (H, W), x.repeat(k, 1, 1, 1))
                sse[:, lo:lo + k] = part.view(k, n).t()
            return sse

    def rd_ladder(self, z, y, x, steps, offsets=None):
        """Rate and distortion of every ladder index of ``steps`` for given latents: the ladder-cost launches, ``ladder_distortion``
        and ONE read-back -> (cost_z int64 [n], cost_y int64 [n, S] in 2^-16 bit, sse int64 [n, S] as host arrays, ``_hyper_of(z)``
        for the coding launches).  ``offsets`` (``check_offsets``): the candidates are bases of the map clip(base + offsets)."""
        pre = self._hyper_of(z)
        cost_z, cost_y = self._ladder(z, y, steps, pre, offsets)
        sse = self.ladder_distortion(z, y, x, steps, offsets, pre=pre)
        host = torch.cat([cost_z[:, None], cost_y, sse], dim=1).cpu().numpy()                                    # the one read-back
        ops.check_conv_status()
        S = len(steps)
        return host[:, 0], host[:, 1:1 + S], host[:, 1 + S:], pre

    def _quality_control(self, z, y, x, H, W, sse_budget, offsets=None):
        """The pass of ``compress(x, target_psnr=...)`` on given latents: the whole ladder priced and decoded (``rd_ladder``), the
        flushed lane states and the map's records counted as ``_rate_control`` counts them, ``select_quality``.
        -> (the per-image report, ``_hyper_of(z)`` for the coding launches)."""
        ladder = list(range(STEP_MIN, STEP_MAX + 1))
        cost_z, cost_y, sse, pre = self.rd_ladder(z, y, x, ladder, offsets)
        bits = (cost_z[:, None] + cost_y) / float(COST_UNIT) + float(self.flushed_bits(H, W))
        map_bits = None if offsets is None else MAP_RECORD_BITS * count_runs(offsets)
        if map_bits is not None:
            bits = bits + map_bits.astype(np.float64)[:, None]
        report = select_quality(bits, sse, sse_budget, ladder, elements=3 * H * W)
        if map_bits is not None:
            for r, b in zip(report, map_bits):
                r["map_bits"] = float(b)
        return report, pre

    def flushed_bits(self, H, W):
        """The lane states every image's streams flush, in bits: 32 per lane and stream (in the file, not in ``rans_cost``)."""
        c, cz, hz, wz, h, w = self.latent_shapes(H, W)
        ez, ey = hz * wz * cz, h * w * c
        sz, sy = _segments(ez), _segments(ey)
        return 32 * (sz * _lanes(-(-ez // sz)) + sy * _lanes(-(-ey // sy)))

    def compress(self, x, step=None, target_bpp=None, step_offsets=None, target_psnr=None, tile=None, overlap=16) -> bytes:
        """``step`` / ``step_offsets``: as in ``compress_latents``; with ``target_bpp`` the offsets are added to the index rate
        control chooses, the candidates are priced over the map (``ladder_cost(..., step_offsets=...)``), and each image's
        prediction counts ``map_bits`` = 24 per maximal run of its offsets (an upper bound on the records written: clipping
        can only merge runs).  ``target_bpp`` (a number, or one per image): rate control -- per image the
        finest step of the whole ladder whose predicted bits (``ladder_cost`` + the flushed lane states; header and length
        fields not counted) are within target_bpp H W, STEP_MAX where none is.  One encoder pass, the ladder launches, one
        read-back, the coding launches.  ``last_report``: per image step_chosen, bits_predicted, budget_bits, met.
        ``target_psnr`` in dB (a number, or one per image): the opposite question -- per image the step of the whole ladder
        with the FEWEST predicted bits among those whose decoded pixels reach the target (integer SSE <= 255^2 3 H W /
        10^(target / 10), ``ladder_distortion``: exactly what ``decompress`` will give, the 16-bit escape aside), STEP_MIN where
        none does (``select_quality``).  One encoder pass, the ladder launches of both sides, one read-back, the coding launches;
        the file is that of ``step=`` the chosen indexes.  ``last_report``: ``select_quality``'s rows (+ map_bits with offsets).
        ``tile`` = T (with ``overlap``, default 16): a tiled file, wire format 9 (``compress_tiled``); only ``step`` may accompany it."""
        m = self.m
        if tile is not None:
            tiling.refuse_with_tile(target_bpp=target_bpp, target_psnr=target_psnr, step_offsets=step_offsets)
            return self.compress_tiled(x, tile, overlap, step)
        x = m._as_device_images(x)
        n, H, W = x.shape[0], int(x.shape[1]), int(x.shape[2])
        if sum(v is not None for v in (step, target_bpp, target_psnr)) > 1:
            raise ValueError("compress: step, target_bpp and target_psnr exclude each other")
        grid = self._grid(step, step_offsets, n, H, W)
        budgets, offsets = None, None
        if target_bpp is not None or target_psnr is not None:
            if target_psnr is not None:
                budgets = quality_budgets(check_quality(target_psnr, n), H, W)
            else:
                budgets = check_budgets(target_bpp, n) * float(H * W)
            require_fp32(m._precision, "a quantisation step")
            if step_offsets is not None:
                offsets = check_offsets(step_offsets, n, *self.latent_shapes(H, W)[4:])
                offsets = offsets if offsets.any() else None          # all zero: today's rate control, launch for launch
        with torch.cuda.device(m.device):
            lat = m.infer_latent_rvs(x)
            z, y = lat.uq[0].loc.contiguous(), lat.uq[1].loc.contiguous()
            if budgets is None:
                return self._finish([self._launch_latents(z, y, (H, W), grid)])[0]
            if target_psnr is not None:
                self.last_report, pre = self._quality_control(z, y, x, H, W, budgets, offsets)
            else:
                self.last_report, pre = self._rate_control(z, y, H, W, budgets, offsets)
            chosen = [r["step_chosen"] for r in self.last_report]
            return self._finish([self._launch_latents(z, y, (H, W), self._grid(chosen, offsets, n, H, W), pre)])[0]

    def _rate_control(self, z, y, H, W, budget_bits, offsets=None):
        """The rate-control pass of ``compress(x, target_bpp=...)`` on given latents: the whole ladder priced in one pass, the
        flushed lane states counted, ``select_steps``.  ``offsets`` (``check_offsets``): the candidates are bases of the map
        clip(base + offsets), and 24 bits per maximal run of an image's offsets are counted for its map.
        -> (the per-image report, ``_hyper_of(z)`` for the coding launches)."""
        self._check_latents(z, y, (H, W))
        ladder = list(range(STEP_MIN, STEP_MAX + 1))
        pre = self._hyper_of(z)
        cost_z, cost_y = self._ladder(z, y, ladder, pre, offsets)
        host = torch.cat([cost_z[:, None], cost_y], dim=1).cpu().numpy()                                         # the one read-back
        bits = (host[:, :1] + host[:, 1:]) / float(COST_UNIT) + float(self.flushed_bits(H, W))
        map_bits = None if offsets is None else MAP_RECORD_BITS * count_runs(offsets)
        return select_steps(bits, budget_bits, ladder, map_bits), pre

    def check_tiling(self, tile, overlap):
        """``tile`` / ``overlap`` of the public entry points -> (T, O) as ints; ValueError unless T is a multiple of the model's
        downsample factor with T >= 64 and 0 <= O <= T / 4."""
        return tiling.check_tiling(tile, overlap, self.m.downsample_factor)

    def compress_tiled(self, x, tile, overlap=16, step=None) -> bytes:
        """``compress(x, tile=T, overlap=O, step=...)``: the tiled file of x, wire format 9.  The picture is cut into the tiles of
        ``tiling.tile_plan`` (extents of T + up to 2 O pixels; the last of an axis up to 2 T - 1 + O), each inner blob of at most
        ``tiling.TILE_BATCH`` same-shaped tiles is one extract launch (``ops.tiles_extract``) and one ``_launch_latents`` on a
        lane of its own, and ONE ``_finish`` -- two read-backs -- ends all of them, as in ``compress_many``.  Every inner blob is,
        byte for byte, ``compress(those tiles, step=...)``.  ``step``: an int, or one per image, applied to all of that image's
        tiles (inner blobs of wire format 5).  Every refusal comes before anything is enqueued, the upload of a host ``x``
        included.  The inner blobs share the pool's first ``ops.SIDE_POOL_MIN`` lanes in turn -- a large picture has hundreds of
        them, and a stream each would only share hardware queues --; the tiles and latents of ALL of them are resident until
        the one ``_finish``, about the footprint of ``compress(x)`` itself plus the extracted tiles."""
        m = self.m
        T, O = self.check_tiling(tile, overlap)
        shape = tuple(int(v) for v in getattr(x, "shape", ()))
        if len(shape) not in (3, 4):
            raise ValueError(f"compress: images [n, H, W, 3] or [H, W, 3], not shape {shape}")
        n, H, W = (1,) * (4 - len(shape)) + shape[:len(shape) - 1]
        if not (1 <= n <= self.MAX_IMAGES and 1 <= H <= self.MAX_SIDE and 1 <= W <= self.MAX_SIDE):
            raise ValueError(f"compress: {n} images of {H} x {W} are beyond what a file holds")
        steps = None if step is None else check_steps(step, n)
        g, plan, _ = tiling.tile_plan(n, H, W, T, O)
        if len(plan) > 0xffff or max(b["th"] for b in plan) > 0xffff or max(b["tw"] for b in plan) > 0xffff:
            raise ValueError("compress: the tile plan is beyond what a tiled file holds")
        grids = [self._grid(None if steps is None else [steps[i] for i, _, _ in b["tiles"]], None, len(b["tiles"]), b["th"], b["tw"])
                 for b in plan]
        x = m._as_device_images(x)
        assert tuple(x.shape[:3]) == (n, H, W)
        with torch.cuda.device(m.device):
            main, pool = ops.lanes(min(len(plan), ops.SIDE_POOL_MIN), m.device)
            lanes = [pool[k % len(pool)] for k in range(len(plan))]
            jobs = []
            for st, b, grid in zip(lanes, plan, grids):
                rects = [(i, g["rows"][r][2], g["cols"][c][2]) for i, r, c in b["tiles"]]
                with ops.fork(main, st, reads=(x,)):
                    lat = m.infer_latent_rvs(ops.tiles_extract(x, rects, b["th"], b["tw"]))
                    jobs.append(self._launch_latents(lat.uq[0].loc.contiguous(), lat.uq[1].loc.contiguous(), (b["th"], b["tw"]), grid))
            for st, j in zip(lanes, jobs):
                ops.join(main, st, made=[t for grp in j["groups"] for t in grp])
            inner = self._finish(jobs)
        return tiling.pack_v9(ARITH[m._precision], n, H, W, T, O, inner)

    def _refuse_tiled(self, blobs, what):
        for b in blobs:
            if tiling.is_tiled(b):
                raise capi.SntcError(capi.ERR_UNSUPPORTED, f"{what}: the bitstream is a tiled file (wire format {VERSION_TILED}); {what} reads "
                                     "untiled files -- decompress it and compress the pixels again")

    def _decompress_tiled(self, blobs, regions):
        """``decompress_many`` with tiled files among ``blobs``; ``regions[k]``: the window (y0, x0, h, w) of tiled blob k, or
        None.  The inner blobs that hold a needed tile -- cut down to the needed tiles with ``select_images`` where only some
        are -- and the untiled files go through ONE ``decompress_many`` call, whose pipelining then applies to all of them; one
        assemble launch per tiled file follows (``ops.tiles_assemble``; its count of missing pixels is read back once per
        file).  Fills ``last_decompress_report``: one dict(tiles_total, tiles_decoded, bytes_total, bytes_read) per tiled file."""
        arith = ARITH[self.m._precision]
        self.last_decompress_report = None                         # a refused file leaves no earlier call's report behind
        flat, plans = [], []
        for blob, region in zip(blobs, regions):
            if not tiling.is_tiled(blob):
                if region is not None:
                    raise ValueError("decompress: region needs a tiled file (compress(x, tile=...)); this bitstream is not tiled")
                plans.append(len(flat))
                flat.append(blob)
                continue
            blob = bytes(blob)
            hd = tiling.parse_v9(blob, arith)
            g = hd["grid"]
            window = (0, 0, hd["H"], hd["W"]) if region is None else tuple(int(v) for v in region)
            need = set(tiling.region_tiles(g, window))                         # ValueError on a window outside the picture
            at, read = {}, hd["head_bytes"]
            for b in hd["blobs"]:
                keep = [j for j, (_, r, c) in enumerate(b["tiles"]) if (r, c) in need]
                if not keep:
                    continue                                                   # an untouched inner blob is never uploaded
                part = select_images(blob[b["at"]:b["at"] + b["bytes"]], keep)
                read += len(part)
                for j, k in enumerate(keep):
                    at[b["tiles"][k]] = (len(flat), j)
                flat.append(part)
            plans.append(dict(hd=hd, window=window, at=at, report=dict(tiles_total=hd["n"] * g["R"] * g["C"], tiles_decoded=len(at),
                                                                      bytes_total=len(blob), bytes_read=read)))
        decoded = self.decompress_many(flat)
        out = []
        with torch.cuda.device(self.m.device):
            for p in plans:
                if not isinstance(p, dict):
                    out.append(decoded[p])
                    continue
                hd, g = p["hd"], p["hd"]["grid"]
                tiles = []
                for i in range(hd["n"]):
                    for r in range(g["R"]):
                        for c in range(g["C"]):
                            k, j = p["at"].get((i, r, c), (None, None))
                            tiles.append(None if k is None else decoded[k][j])
                out.append(ops.tiles_assemble(tiles, hd["n"], hd["H"], hd["W"], RESIDUAL_CHANNELS, hd["tile"], hd["overlap"], p["window"]))
        self.last_decompress_report = [p["report"] for p in plans if isinstance(p, dict)]
        return out

    def compress_many(self, xs):
        """``compress`` for several batches (e.g. one per image size of a set) -> their bitstreams, in order, byte for byte what one
        ``compress`` per batch returns.  The batches' transforms and entropy-coding launches run side by side on the library's
        side streams; the stream lengths of ALL batches come back in one copy, the packed payloads in another -- two host
        synchronisations for the set instead of two per batch."""
        return _compress_many(self, xs)

    def _parse(self, blob: bytes):
        """Header and stream lengths of one blob, checked against THIS model: nothing later trusts the header."""
        mapped = len(blob) > 4 and blob[4] == VERSION_MAP          # the version byte: 3 and 5 -> parse_v3, 7 -> parse_v7
        hd = (parse_v7 if mapped else parse_v3)(blob, self.m._precision, self.latent_shapes)
        hd["grid"] = StepGrid.from_header(hd)
        if hd["grid"].kind != "unit" and self.m._precision != "fp32":
            raise capi.SntcError(capi.ERR_UNSUPPORTED, f"bitstream version {blob[4]} (quantisation steps) decodes in precision 'fp32' only")
        return hd

    def decompress(self, blob: bytes, region=None):
        """``region`` = (y0, x0, h, w): that window of a TILED file (wire format 9) -> uint8 [n, h, w, 3], equal to the same window
        of the full decode; only the tiles whose extents meet it are decoded (``_decompress_tiled``).  ValueError on an untiled
        file or a window that leaves the picture.  ``last_decompress_report``: dict(tiles_total, tiles_decoded, bytes_total,
        bytes_read) after a tiled file, None after an untiled one (``decompress_many``: a LIST with one such dict per tiled file
        of the call, in order; None where the call held no tiled file)."""
        out = self.decompress_many([blob], regions=None if region is None else [region])[0]
        if self.last_decompress_report is not None:
            self.last_decompress_report = self.last_decompress_report[0]
        return out

    def decompress_many(self, blobs, regions=None):
        """Several bitstreams (e.g. one per batch shape of a set) -> their pixel batches, in order.  An entropy-decoding launch
        is a handful of lone waves whose time is a latency (one wave per stream, ~0.4 us per step of 64 symbols whatever the
        batch), so the launches of ALL blobs' hyper-latents run side by side on streams of their own; then the blobs are
        pipelined, largest first: blob k's latents decode on its stream while the caller's stream runs blob k + 1's
        hyper-synthesis and, later, blob k - 1's synthesis.  A decoding wave holds ~100 KB of tables in its CU's LDS and a
        stream-K convolution needs every one of its workers resident (round 4 measured what happens when they meet: groups of one
        blob's images pipelined against each other's stream-K convolutions, 9.5 -> 10.9 / 12.7 / 17.6 ms with 2 / 3 / 4 groups),
        so only the FIRST hyper-synthesis -- which meets no decoding wave -- keeps stream-K; the convolutions that may run beside
        decoding waves take the static schedules (``ops.static_schedules``; same bits).  Everything up to the latents' decode is
        ``_decode_front``, shared with ``transcode_many``; the syntheses, the residual layers and the final check are here."""
        m = self.m
        if not blobs:
            return []
        if regions is not None or any(tiling.is_tiled(b) for b in blobs):
            # wire format 9: its inner blobs join the others in ONE call of this function, an assemble launch per tiled file follows
            blobs = list(blobs)
            regions = [None] * len(blobs) if regions is None else list(regions)
            if len(regions) != len(blobs):
                raise ValueError(f"decompress_many: {len(regions)} regions for {len(blobs)} bitstreams")
            return self._decompress_tiled(blobs, regions)
        self.last_decompress_report = None                         # no tiled file in this call (``_decompress_tiled`` sets its own after it)
        # wire format 8: the base file inside goes through the pipeline below unchanged, its residual layer follows the syntheses
        layers = [None] * len(blobs)
        if any(is_residual(b) for b in blobs):
            blobs = list(blobs)
            for k, b in enumerate(blobs):
                if is_residual(b):
                    blobs[k], layers[k] = split_residual(b)
                    layers[k]["blob"] = b
        nlayers = sum(l is not None for l in layers)
        heads = [self._parse(b) for b in blobs]
        with torch.cuda.device(m.device):
            # (a residual layer adds two counters behind the others: its streams', and the out-of-range count of sntc_residual_apply)
            f = self._decode_front(blobs, heads, counters=2 * nlayers)
            main, lanes, bad, order, piped = f["main"], f["lanes"], f["bad"], f["order"], f["piped"]
            # A blob's synthesis runs while the later blobs' latents decode: every synthesis but the last may run beside decoding
            # waves and takes the static schedules.  A/B (PIPELINE_BLOBS = False): every blob's latents first, then the syntheses
            for k in ([] if piped else order):
                ops.join(main, lanes[k])
            out = [None] * len(heads)
            for i, k in enumerate(order):
                hd = heads[k]
                ops.join(main, lanes[k], made=(f["syms"][k],))
                with ops.static_schedules(piped and i + 1 < len(order)):
                    y_hat = hd["grid"].dequant(f["syms"][k], f["hypers"][k], m._synthesis.takes_s3(hd["h"], hd["w"]))
                    out[k] = m._pixels(y_hat, (hd["H"], hd["W"]))
            if nlayers:
                self._apply_layers(layers, out, bad[2 * len(blobs):])
            nbad = int(bad.sum().item())                           # synchronises the stream
            total = sum(hd["n"] * (hd["sz"] + hd["sy"]) for hd in heads) + sum(l["n"] * l["segments"] for l in layers if l is not None)
            nres = int(bad[2 * len(blobs) + 1::2].sum().item()) if nbad and nlayers else None
            _raise_if_bad(nbad - (nres or 0), total, nres)
            ops.check_conv_status()       # wrong pixels never leave without an error
            return out

    def _decode_front(self, blobs, heads, counters=0):
        """The front of ``decompress_many`` and ``transcode_many``: parsed ``heads`` of ``blobs`` -> per blob the y symbols, with
        their decode IN FLIGHT on the blob's lane -- the caller joins lanes[k], naming syms[k], when it consumes blob k, in
        ``order`` --, the hyper-synthesis output and the base table ids (``scale_table_ids``), as a dict of lists indexed by blob
        (+ main, lanes, bad, order, piped, zis).  Everything the blobs need goes up first (``pack_upload``: ONE copy for all words
        and stream offsets; v5 / v7: each grid's step tensors or map, read on the caller's stream only), then nothing waits for
        the host: all z decode side by side and are joined; then the blobs are PIPELINED, largest first (``order``): a blob's
        latents decode on its lane while the caller's stream runs the next blob's hyper-synthesis.  The first hyper-synthesis
        meets no decoding wave and keeps its stream-K launches; every convolution after it may run beside decoding waves and
        takes the static schedules (``ops.static_schedules``: same bits).  A/B (``PIPELINE_BLOBS`` = False), round 4's schedule:
        every hyper-synthesis, then every blob's latents side by side.
        ``bad``: one counter per entropy-decoding launch (the launch zeroes its own) -- blob k's z at 2 k, its y at 2 k + 1, then
        ``counters`` more for the caller -- for ONE read-back where the caller synchronises anyway."""
        m, dev, nb = self.m, self.m.device, len(heads)
        main, lanes = ops.lanes(nb, dev)
        bad = torch.zeros((2 * nb + counters,), dtype=torch.int32, device=dev)
        offs = [np.concatenate([[0], np.cumsum(hd[f])]).astype(np.int64) for hd in heads for f in ("zl", "yl")]
        words = [np.frombuffer(b, "<i2", nw, at) for b, hd in zip(blobs, heads)
                 for nw, at in ((hd["zw"], hd["pos"]), (hd["yw"], hd["pos"] + 2 * hd["zw"]))]
        up, views = pack_upload(offs + words, dev)
        offd, pay = views[:2 * nb], views[2 * nb:]
        for hd in heads:
            hd["grid"].on(dev)
        zis = []
        for k, (hd, st) in enumerate(zip(heads, lanes)):
            shape = (hd["n"], hd["hz"], hd["wz"], hd["cz"])
            with ops.fork(main, st, reads=(up, bad)):
                zis.append(rans_decode(pay[2 * k], hd["zl"], channel_table_ids(shape, dev), shape, self.z_tables, hd["sz"], hd["lz"],
                                       bad=bad[2 * k:2 * k + 1], offsets=offd[2 * k]))
        for st, zi in zip(lanes, zis):
            ops.join(main, st, made=(zi,))
        piped = PIPELINE_BLOBS and len(set(lanes)) > 1             # the blobs have streams of their own
        order = sorted(range(nb), key=lambda k: -(heads[k]["n"] * heads[k]["h"] * heads[k]["w"])) if piped else list(range(nb))
        hypers, bases, tids, syms = [None] * nb, [None] * nb, [None] * nb, [None] * nb

        def launch_latents(k):
            hd = heads[k]
            with ops.fork(main, lanes[k], reads=(up, bad, tids[k])):
                syms[k] = rans_decode(pay[2 * k + 1], hd["yl"], tids[k], (hd["n"], hd["h"], hd["w"], hd["c"]), self.y_tables, hd["sy"],
                                      hd["ly"], bad=bad[2 * k + 1:2 * k + 2], offsets=offd[2 * k + 1])

        for i, k in enumerate(order):
            hd = heads[k]
            with ops.static_schedules(piped and i > 0):
                hypers[k] = m._hyper_synthesis(int_to_float(zis[k]))
            if tuple(hypers[k].shape) != (hd["n"], hd["h"], hd["w"], 2 * hd["c"]):
                raise capi.SntcError(capi.ERR_BAD_SHAPE, f"hyper-synthesis output {tuple(hypers[k].shape)} does not match the latents "
                                     f"{(hd['n'], hd['h'], hd['w'], hd['c'])}")
            bases[k] = scale_table_ids(hypers[k])
            tids[k] = hd["grid"].table_ids(bases[k])
            if piped:
                launch_latents(k)
        for k in ([] if piped else order):
            launch_latents(k)
        return dict(main=main, lanes=lanes, bad=bad, order=order, piped=piped, zis=zis, syms=syms, hypers=hypers, bases=bases)

    def _apply_layers(self, layers, out, bad):
        """The residual layers of ``decompress_many``: ``layers[k]`` = ``split_residual``'s info of blob k or None, ``out[k]`` its
        decoded base picture, already enqueued on the caller's stream.  ONE upload for every layer's words, stream offsets and
        choices; per layer, on a pooled lane (a single layer too), ``residual_table_ids`` -> ``rans_decode`` -> ``residual_apply``
        replaces out[k]; layer j's bad-stream count goes to bad[2 j], its out-of-range count to bad[2 j + 1].  The layers start
        after the last synthesis was enqueued: their decoding waves run side by side with each other, never beside a stream-K
        convolution."""
        ks = [k for k, l in enumerate(layers) if l is not None]
        ls = [layers[k] for k in ks]
        up, views = pack_upload([np.concatenate([[0], np.cumsum(l["lens"])]).astype(np.int64) for l in ls] +
                                [np.frombuffer(l["blob"], "<i2", l["words"], l["pos"]) for l in ls] + [l["choice"] for l in ls], self.m.device)
        main, lanes = ops.lanes(len(ks), self.m.device, alone=True)
        for j, (k, l, st) in enumerate(zip(ks, ls, lanes)):
            base, (off_d, word_d, choice_d) = out[k], views[j::len(ks)]
            shape = (l["n"], l["H"], l["W"], RESIDUAL_CHANNELS)
            if tuple(base.shape) != shape:
                raise capi.SntcError(capi.ERR_BAD_SHAPE, f"decoded base picture {tuple(base.shape)} does not match the residual layer's {shape}")
            with ops.fork(main, st, reads=(base, up, bad)):
                ids = residual_table_ids(base, choice_d.view(l["n"], -1))
                q = rans_decode(word_d, l["lens"], ids, shape, self.y_tables, l["segments"], l["lanes"], bad=bad[2 * j:2 * j + 1], offsets=off_d)
                out[k], _ = residual_apply(base, q, l["max_error"], count=bad[2 * j + 1:2 * j + 2])
        for k, st in zip(ks, lanes):
            ops.join(main, st, made=(out[k],))

    def _refuse_layered(self, blobs, what):
        for b in blobs:
            if is_residual(b):
                raise ValueError(f"{what}: the bitstream carries a residual layer (wire format {VERSION_RESIDUAL}); take its base file with "
                                 "entropy_coding.split_residual(blob)[0] and add a layer to the result with add_residual")

    def _layer(self, base_blob, base, x, delta):
        """The residual layer of ``x`` float32 [n, H, W, 3] over the decoded picture ``base`` of ``base_blob`` -> the v8 blob:
        ``residual_quantize``, ONE read-back of the histogram, ``residual_choice``, ``residual_table_ids``, ``rans_encode`` with the
        model's y tables, ``pack_v8``.  Fills ``last_residual``."""
        _, H, W, c = base.shape
        if tuple(x.shape) != tuple(base.shape) or x.dtype != torch.float32 or c != RESIDUAL_CHANNELS:
            raise ValueError(f"add_residual: images {tuple(x.shape)} are not the {tuple(base.shape)} the bitstream decodes to")
        if H * W * c > RESIDUAL_MAX_ELEMS:
            raise ValueError(f"add_residual: an image of more than {RESIDUAL_MAX_ELEMS} values")
        q, hist = residual_quantize(x, base, delta)
        hist_h = hist.cpu().numpy().view(np.uint32)                                                     # the one read-back of the histogram
        choice, cost_q = residual_choice(hist_h, self.y_tables.host)
        ids = residual_table_ids(base, torch.from_numpy(choice).to(base.device))
        segments, lanes = residual_streams(H, W)
        payload, lens = rans_encode(q, ids, self.y_tables, segments, lanes)
        words = payload.cpu().numpy()
        ops.check_conv_status()
        self.last_residual = dict(max_error=delta, choice=choice, cost_q=cost_q, hist=hist_h,
                                  bits_predicted=cost_q / float(COST_UNIT) + 32.0 * segments * lanes)
        return pack_v8(ARITH[self.m._precision], delta, base_blob, segments, lanes, choice, lens) + words.tobytes()

    def add_residual(self, blob: bytes, x, max_error) -> bytes:
        """A v3 / v5 / v7 bitstream of this model and the images it was made from -> the v8 bitstream whose decoded pixels are
        within ``max_error`` (an int, 0 .. 127; 0: lossless) of x quantised to uint8, every one of them: the base file unchanged,
        then the coded residual q = sgn(r) ((|r| + max_error) div (2 max_error + 1)), r = x8 - the base's decoded pixel
        (csrc/residual_rules.h), under one of the model's 64 normal tables per (image, class), chosen by exact coded cost.
        ``split_residual(result)[0] == blob``.  A v8 ``blob`` is a ValueError.  ``last_residual``: max_error, choice, cost_q,
        bits_predicted per image, and hist, the histogram the choice was made from."""
        m = self.m
        delta = check_max_error(max_error)
        require_fp32(m._precision, "the residual layer")
        self._refuse_tiled([blob], "add_residual")
        self._refuse_layered([blob], "add_residual")
        x = self._layer_images(blob, x, "add_residual")
        with torch.cuda.device(m.device):
            return self._layer(bytes(blob), self.decompress(blob), x, delta)

    def _layer_images(self, blob, x, what):
        """``x`` of ``add_residual`` / ``residual_bits`` on the device, checked against the header of ``blob`` before any launch."""
        x = self.m._as_device_images(x)
        hd = self._parse(blob)
        shape = (hd["n"], hd["H"], hd["W"], RESIDUAL_CHANNELS)
        if tuple(x.shape) != shape or x.dtype != torch.float32:
            raise ValueError(f"{what}: float32 images {tuple(x.shape)} are not the {shape} the bitstream decodes to")
        if hd["H"] * hd["W"] * RESIDUAL_CHANNELS > RESIDUAL_MAX_ELEMS:
            raise ValueError(f"{what}: an image of more than {RESIDUAL_MAX_ELEMS} values")
        return x

    def residual_bits(self, x, blob: bytes, max_error):
        """What the residual layer of ``add_residual(blob, x, d)`` would pay per image, without coding anything: ``max_error`` an
        int -> float64 [n], a list of ints -> [n, len].  The exact coded cost of the chosen tables (``residual_choice``) / 65536 +
        32 bits per flushed lane state; the coder's renormalisation slack, the choice bytes and the length fields are not in it.
        One decode of the base, one quantisation launch per value, ONE read-back."""
        m = self.m
        many = not isinstance(max_error, (int, np.integer)) or isinstance(max_error, bool)
        deltas = [check_max_error(d) for d in (max_error if many else [max_error])]
        if not deltas:
            raise ValueError("residual_bits: no max_error")
        require_fp32(m._precision, "the residual layer")
        self._refuse_tiled([blob], "residual_bits")
        self._refuse_layered([blob], "residual_bits")
        x = m._as_device_images(x)
        with torch.cuda.device(m.device):
            base = self.decompress(blob)
            if tuple(x.shape) != tuple(base.shape) or x.dtype != torch.float32:
                raise ValueError(f"residual_bits: images {tuple(x.shape)} are not the {tuple(base.shape)} the bitstream decodes to")
            hists = torch.stack([residual_quantize(x, base, d)[1] for d in deltas]).cpu().numpy().view(np.uint32)      # the one read-back
        segments, lanes = residual_streams(base.shape[1], base.shape[2])
        bits = np.stack([residual_choice(h, self.y_tables.host)[1] / float(COST_UNIT) + 32.0 * segments * lanes for h in hists], axis=1)
        return bits if many else bits[:, 0]

    def transcode(self, blob: bytes, shift=None, target_bpp=None) -> bytes:
        """``transcode_many`` of one bitstream; ``shift`` / ``target_bpp``: a value or one per image.  ``last_report``: [its rows]."""
        return self.transcode_many([blob], None if shift is None else [shift], None if target_bpp is None else [target_bpp])[0]

    def transcode_many(self, blobs, shift=None, target_bpp=None):
        """Bitstreams of this model -> the bitstreams of a coarser step, without pixels: image i of a blob moves d_i >= 0 places
        up the scale ladder, every position from its index k0 to k1 = clip(k0 + d_i, STEP_MIN, STEP_MAX).  Per latent element
        (csrc/quant_step.hip, one rule): y_hat0 = step_value(s0, mu, step[k0]) is what ``decompress`` would feed the
        synthesis, s1 = step_round(step_diff(y_hat0, mu), inv_step[k1]) and t1 = step_table_id(base, k1) are coded.  The output is
        ``compress_latents(z_hat, y_hat0, (H, W))`` on the grid k1, byte for byte: wire format 3, 5 or 7 (``StepGrid.shifted``),
        the z streams and their header fields copied from the source.  The work is ``_decode_front``, which ``decompress_many``
        drives too -- z decoded side by side, the hyper-synthesis, y decoded with the source grid's tables, pipelined largest
        first -- then one requantisation launch and the y coder per blob; no analysis, no synthesis.
        Exactly one of ``shift`` / ``target_bpp``, each ONE value for every blob or a sequence with one entry per blob, an entry
        being a value or one per image of that blob (``check_shifts`` / ``check_budgets``).  ``target_bpp``: per image the SMALLEST
        d whose exact coded cost fits target_bpp H W -- ``select_steps`` over d = 0 .. STEP_MAX - min(k0) with the bits
        ``compress(target_bpp=)`` compares (``rans_cost`` of z, the requantised y priced by ``step_requant_ladder_cost``, the flushed
        lane states, 24 bits per run of a source map; header and length fields not counted), the top d and met = False where
        none fits.  ``last_report``: per blob the rows of ``select_steps`` (step_chosen = d).  One read-back more than ``shift=``.
        A corrupt source raises ``SntcError`` like ``decompress_many`` and yields no file."""
        m = self.m
        blobs = list(blobs)
        if (shift is None) == (target_bpp is None):
            raise ValueError("transcode: exactly one of shift and target_bpp")
        require_fp32(m._precision, "transcode")
        self._refuse_tiled(blobs, "transcode")
        self._refuse_layered(blobs, "transcode")
        if not blobs:
            return []
        heads = [self._parse(b) for b in blobs]

        def per_blob(value, check):
            values = list(value) if isinstance(value, (list, tuple, np.ndarray)) else [value] * len(heads)
            if len(values) != len(heads):
                raise ValueError(f"transcode: {len(values)} entries for {len(heads)} bitstreams")
            return [check(v, hd["n"]) for v, hd in zip(values, heads)]

        grids = [hd["grid"] for hd in heads]
        if shift is not None:
            shifts = per_blob(shift, check_shifts)
        else:
            budgets = [b * float(hd["H"] * hd["W"]) for b, hd in zip(per_blob(target_bpp, check_budgets), heads)]
        srcs = [g.indexes(hd["h"], hd["w"]) for g, hd in zip(grids, heads)]
        dev = m.device
        with torch.cuda.device(dev):
            lut = cached_step_lut(dev)
            # every blob's source map goes up here, before anything is enqueued (a map grid keeps its own copy)
            src_d = [g.on(dev)[0] if g.kind == "map" else torch.from_numpy(s).to(dev) for g, s in zip(grids, srcs)]
            f = self._decode_front(blobs, heads)
            main, lanes, syms, hypers, bases = f["main"], f["lanes"], f["syms"], f["hypers"], f["bases"]
            if shift is None:
                for k in f["order"]:
                    ops.join(main, lanes[k], made=(syms[k],))
                shifts = self._shift_control(heads, f["zis"], syms, hypers, bases, srcs, src_d, budgets, f["bad"])
            jobs = [None] * len(heads)
            for k in f["order"]:              # blob k requantised and coded while the later blobs' latents still decode
                hd = heads[k]
                if shift is not None:
                    ops.join(main, lanes[k], made=(syms[k],))
                out = grids[k].shifted(shifts[k])
                dst = torch.from_numpy(np.ascontiguousarray(out.indexes(hd["h"], hd["w"]))).to(dev)
                sym, tid = ops.step_requant_symbols(syms[k], hypers[k], bases[k], src_d[k], dst, lut)
                jobs[k] = dict(n=hd["n"], H=hd["H"], W=hd["W"], sz=hd["sz"], sy=hd["sy"], lz=hd["lz"], ly=hd["ly"], grid=out,
                               dims=tuple(hd[d] for d in ("c", "cz", "hz", "wz", "h", "w")),
                               copied=(hd["zl"], np.frombuffer(blobs[k], "<i2", hd["zw"], hd["pos"])),
                               groups=[rans_encode_launch(sym, tid, self.y_tables, hd["sy"], hd["ly"])])
            out = self._finish(jobs)
            _raise_if_bad(int(f["bad"].sum().item()), sum(hd["n"] * (hd["sz"] + hd["sy"]) for hd in heads))
            return out

    def _shift_control(self, heads, zis, syms, hypers, bases, srcs, src_d, budgets, bad):
        """The rate-control pass of ``transcode_many(target_bpp=...)``: every blob's shifts d = 0 .. STEP_MAX - min(k0) priced from
        its decoded symbols (launches of at most ``LADDER_MAX`` candidates), ONE read-back for all blobs (the bad-stream counters
        travel with it: a corrupt source raises here), then ``select_steps`` with the shifts as its steps -- the bits
        ``_rate_control`` compares.  Fills ``last_report``; -> per blob the chosen shifts."""
        dev = self.m.device
        cands = [list(range(0, STEP_MAX - int(s.min()) + 1)) for s in srcs]
        parts = [bad.to(torch.int64)]
        for k, hd in enumerate(heads):
            cost_z = rans_cost(zis[k], channel_table_ids(tuple(zis[k].shape), dev), self.z_tables)
            cost_y = step_requant_ladder_cost(syms[k], hypers[k], bases[k], src_d[k], cands[k], self.y_tables)
            parts += [cost_z, cost_y.reshape(-1)]
        host = torch.cat(parts).cpu().numpy()                                                                    # the one read-back
        _raise_if_bad(int(host[:len(bad)].sum()), sum(hd["n"] * (hd["sz"] + hd["sy"]) for hd in heads))
        self.last_report, shifts, o = [], [], len(bad)
        for k, hd in enumerate(heads):
            n, S = hd["n"], len(cands[k])
            cost_z, cost_y = host[o:o + n], host[o + n:o + n + n * S].reshape(n, S)
            o += n + n * S
            bits = (cost_z[:, None] + cost_y) / float(COST_UNIT) + float(self.flushed_bits(hd["H"], hd["W"]))
            map_bits = MAP_RECORD_BITS * count_runs(srcs[k]) if hd["grid"].kind == "map" else None
            report = select_steps(bits, budgets[k], cands[k], map_bits)
            for i, r in enumerate(report):    # where nothing fits select_steps names the ladder's top: here that is the last shift
                if not r["met"]:
                    r.update(step_chosen=cands[k][-1], bits_predicted=float(bits[i, -1]) + r.get("map_bits", 0.0))
            self.last_report.append(report)
            shifts.append([r["step_chosen"] for r in report])
        return shifts


# -- wire format v4: pure host functions (numbers in, numbers out; no device) ---------------------------------------------
HEAD_V4 = "<HHIIHHHHBB"                   # version | n | H | W | C | h | w | segments | lanes | 0
MAX_IMAGES, MAX_SIDE = Codec.MAX_IMAGES, Codec.MAX_SIDE


def pack_v4(arith, n, H, W, c, h, w, segments, lanes, len_words) -> bytes:
    """Everything of a v4 blob in front of the payload: magic, header, the streams' lengths in 16-bit words."""
    len_words = np.asarray(len_words, np.int64)
    if len(len_words) != n * segments:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "stream count does not match the image / segment counts")
    return MAGIC + struct.pack(HEAD_V4, VERSION_FACTORIZED | (arith << 8), n, H, W, c, h, w, segments, lanes, 0) + len_words.astype("<u4").tobytes()


def parse_v4(blob: bytes, arith, latent_shape):
    """Header and stream lengths of one v4 blob, checked against the decoding model: ``arith`` its arithmetic tag,
    ``latent_shape(H, W) -> (C, h, w)`` its latents for an H x W image.  Every dimension is recomputed from (H, W) and compared;
    segments and lanes are recomputed from the latent size: no header field sizes an allocation.
    -> dict(n, H, W, c, h, w, segments, lanes, lens int64[n * segments], pos = payload offset, words)."""
    if blob[:4] != MAGIC:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "not an SNTC bitstream")
    pos = 4 + struct.calcsize(HEAD_V4)
    if len(blob) < 6:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "bitstream truncated")
    (word,) = struct.unpack_from("<H", blob, 4)
    ver, tag = word & 0xff, word >> 8
    if ver != VERSION_FACTORIZED:
        raise capi.SntcError(capi.ERR_UNSUPPORTED, f"bitstream version {ver}: a factorized-prior model reads version {VERSION_FACTORIZED}")
    if tag != arith:
        names = {v: k for k, v in ARITH.items()}
        raise capi.SntcError(capi.ERR_UNSUPPORTED, f"bitstream was written by a {names.get(tag, tag)!r} model, this model computes "
                             f"in {names.get(arith, arith)!r}: the pixels would not be reproduced bit for bit")
    if len(blob) < pos:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "bitstream truncated")
    _, n, H, W, c, h, w, segments, lanes, zero = struct.unpack_from(HEAD_V4, blob, 4)
    if not (1 <= n <= MAX_IMAGES and 1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise capi.SntcError(capi.ERR_BAD_SHAPE, f"bitstream header: implausible batch / image size n={n} H={H} W={W}")
    want = tuple(int(v) for v in latent_shape(H, W))
    if (c, h, w) != want:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, f"bitstream header (C, h, w) = {(c, h, w)} does not match this model's latents "
                             f"for a {H} x {W} image: {want}")
    e = h * w * c
    if segments != _segments(e) or lanes != _lanes(-(-e // segments)) or zero != 0:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "bitstream header: segment / lane counts do not match the latent size")
    ns = n * segments
    if len(blob) < pos + 4 * ns:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "bitstream truncated")
    lens = np.frombuffer(blob, "<u4", ns, pos).astype(np.int64)
    pos += 4 * ns
    words = int(lens.sum())
    if len(blob) != pos + 2 * words:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "bitstream truncated")
    return dict(n=n, H=H, W=W, c=c, h=h, w=w, segments=segments, lanes=lanes, lens=lens, pos=pos, words=words)


class FactorizedCodec:
    """compress / decompress for a factorized-prior ``Model`` (factorized/models.py): wire format v4, one table per channel of
    y from the model's deep-factorized prior, coded by the channel-indexed kernels (csrc/rans_channels.hip) straight from the
    analysis output and straight into the synthesis input.  ``decompress(compress(x))`` equals
    ``model.decode(model.encode(x)[0], None, (H, W))`` bit for bit.

    Known limit, shared with ``Codec``: an escaped value travels in 16 bits, so |y_hat| > 32767 is clamped in the stream."""

    def __init__(self, model):
        self.m = model
        self.last_decompress_report = None
        dev = model.device
        nl = len(model._prior_num_filters) + 1
        with torch.cuda.device(dev):
            self.y_tables = DeviceTables(factorized_tables(model._prior_weights, nl), dev)

    def latent_shape(self, H, W):
        """(C, h, w) of this model's latents for an H x W image (pad to the downsample factor, then the analysis' own shape
        arithmetic)."""
        m = self.m
        f = m.downsample_factor
        h, w = m._analysis.out_hw(-(-H // f) * f, -(-W // f) * f)
        return (m._bottleneck_size, h, w)

    def _check_latents(self, y, image_hw):
        H, W = int(image_hw[0]), int(image_hw[1])
        c, h, w = self.latent_shape(H, W)
        n = y.shape[0]
        if tuple(y.shape) != (n, h, w, c):
            raise capi.SntcError(capi.ERR_BAD_SHAPE, f"latents {tuple(y.shape)} are not this model's for {n} images of {H} x {W}: {(n, h, w, c)}")
        return n, H, W

    def _launch_latents(self, y, image_hw):
        """The coder's launch(es) (``FUSED_CHANNEL_ENCODE``) on latents of images of ``image_hw``, on the current stream; no host
        synchronisation."""
        n, H, W = self._check_latents(y, image_hw)
        e = y[0].numel()
        segments = _segments(e)
        lanes = _lanes(-(-e // segments))
        if FUSED_CHANNEL_ENCODE:
            scratch, lens, _ = rans_encode_channels_launch(y, self.y_tables, segments, lanes)
        else:
            scratch, lens = rans_encode_launch(round_to_int(y), channel_table_ids(y.shape, y.device), self.y_tables, segments, lanes)
        return dict(n=n, H=H, W=W, dims=tuple(y.shape[1:]), segments=segments, lanes=lanes, groups=[(scratch, lens)])

    def _launch(self, x):
        """analysis -> ``_launch_latents``."""
        return self._launch_latents(self.m.infer_latent_rvs(x).uq[0].loc, x.shape[1:3])

    def _finish(self, jobs):
        """Launched jobs -> their blobs (``finish_streams``: two read-backs for all of them)."""
        out = []
        for j, ((lens_h, words),) in zip(jobs, finish_streams([j["groups"] for j in jobs])):
            h, w, c = j["dims"]
            out.append(pack_v4(ARITH[self.m._precision], j["n"], j["H"], j["W"], c, h, w, j["segments"], j["lanes"], lens_h) + words.tobytes())
        return out

    def compress_latents(self, y_loc, image_hw) -> bytes:
        """Latents of this model for images of ``image_hw`` = (H, W) -- the analysis', or ones refined by iterative inference --
        -> the bitstream ``decompress`` reads.  ``compress(x)`` is this on ``infer_latent_rvs(x)``."""
        with torch.cuda.device(self.m.device):
            return self._finish([self._launch_latents(y_loc.contiguous(), image_hw)])[0]

    def latents_cost(self, y_loc, x):
        """``Codec.latents_cost`` for the one latent: -> (None, cost_y int64 [n] in 2^-16 bit, uint8 pixels, integer SSE [n])."""
        n, H, W = self._check_latents(y_loc, x.shape[1:3])
        yi = round_to_int(y_loc.contiguous())
        cost_y = rans_cost(yi, channel_table_ids(yi.shape, yi.device), self.y_tables)
        px, sse = self.m.decode(int_to_float(yi), None, (H, W), reference=x, check=False)
        return None, cost_y, px, sse

    def compress(self, x) -> bytes:
        m = self.m
        x = m._as_device_images(x)
        with torch.cuda.device(m.device):
            return self._finish([self._launch(x)])[0]

    def compress_many(self, xs):
        """``compress`` for several batches -> their bitstreams, in order, byte for byte what one ``compress`` per batch returns.
        The batches' analyses and coder launches run side by side on the library's side streams; the stream lengths of ALL
        batches come back in one copy, the packed payloads in another (``Codec.compress_many``)."""
        return _compress_many(self, xs)

    def _parse(self, blob: bytes):
        """Header and stream lengths of one blob, checked against THIS model: nothing later trusts the header."""
        return parse_v4(blob, ARITH[self.m._precision], self.latent_shape)

    def decompress(self, blob: bytes):
        return self.decompress_many([blob])[0]

    def decompress_many(self, blobs):
        """Several bitstreams -> their pixel batches, in order.  ONE upload for every blob's words and stream offsets; the
        entropy-decoding launches of all blobs run side by side on streams of their own (lone waves whose time is a latency,
        ``Codec.decompress_many``); the syntheses run on the caller's stream, largest blob first, each as soon as its latents
        are there.  A synthesis that may run beside another blob's decoding waves takes the static schedules
        (``ops.static_schedules``: same bits); the last one, and a lone blob's, meet none and keep stream-K.  One read-back
        of the streams' termination counters, ``ops.check_conv_status()``, then the pixels are returned."""
        m = self.m
        if not blobs:
            return []
        heads = [self._parse(b) for b in blobs]
        dev = m.device
        with torch.cuda.device(dev):
            main, lanes = ops.lanes(len(blobs), dev)
            bad = torch.zeros((len(blobs),), dtype=torch.int32, device=dev)
            up, views = pack_upload([np.concatenate([[0], np.cumsum(hd["lens"])]).astype(np.int64) for hd in heads] +
                                    [np.frombuffer(b, "<i2", hd["words"], hd["pos"]) for b, hd in zip(blobs, heads)], dev)
            y_hats = []
            for k, (hd, st) in enumerate(zip(heads, lanes)):
                with ops.fork(main, st, reads=(up, bad)):
                    y_hats.append(rans_decode_channels(views[len(heads) + k], hd["lens"], (hd["n"], hd["h"], hd["w"], hd["c"]), self.y_tables,
                                                       hd["segments"], hd["lanes"], bad=bad[k:k + 1], offsets=views[k]))
            beside = len(set(lanes)) > 1                           # the blobs have streams of their own
            order = sorted(range(len(heads)), key=lambda k: -(heads[k]["n"] * heads[k]["h"] * heads[k]["w"]))
            out = [None] * len(heads)
            for i, k in enumerate(order):
                hd = heads[k]
                ops.join(main, lanes[k], made=(y_hats[k],))
                with ops.static_schedules(beside and i + 1 < len(order)):
                    out[k] = m.decode(y_hats[k], None, (hd["H"], hd["W"]), check=False)
            _raise_if_bad(int(bad.sum().item()), sum(hd["n"] * hd["segments"] for hd in heads))     # synchronises the stream
            ops.check_conv_status()       # wrong pixels never leave without an error
            return out
