"""The gather GEMM's vector loader (csrc/gather_gemm_kernel.h): tap offsets from per-tile (base, mask) state and a
scalar delta (csrc/gg_tap_rules.h), and the two staging register sets of the steady-state K loop.

Every case meets the float64 oracle at the bar of test_conv_family_fuzz (2e-5 * max(|ref|, 1)) on forced variants 1, 2, 3, 8, 9 --
register ring -- and on variant 2 with direct-to-LDS staging, and all of them give the same bits (torch.equal).  Variant 3
(128 x 96) keeps ONE staging set in every build and the direct-to-LDS instance has no staging registers at all: in a library built
with -DSNTC_GG_TWO_SETS=1 (csrc/sntc_internal.h; off in the shipped one, it measured slower) equality with them is the evidence that
the two-set loop of variants 1, 2, 8, 9 runs the same k-ordered fma chains.  The tests pass on both builds.

The shapes are the smallest at which the loader can go wrong:
  1. borders on all four sides, several images and padding rows inside one tile;
  2. 1 to 7 K stages per tile: every prologue / tail pattern of the two-set loop (it leaves its steady state on either parity);
  3. stream-K pieces and split-K ranges that start and end on odd and on even stages of a tile.
"""
import zlib

import numpy as np
import pytest
import torch

from oracle import ops_np as O

gpu = pytest.mark.gpu

TOL = 2e-5
REF = {"conv": O.conv2d, "convT": O.conv2d_transpose}
FORCED = [(1, False), (2, False), (3, False), (8, False), (9, False), (2, True)]     # (variant, direct-to-LDS)


def _dev_t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def _within(got, ref, what):
    got = got.cpu().numpy()
    assert got.shape == ref.shape, what
    err = np.abs(got.astype(np.float64) - ref).max()
    bar = TOL * max(np.abs(ref).max(), 1.0)
    print(f"{what}: max |got - f64| = {err:.3e}, bar {bar:.3e}")
    assert err <= bar, (what, err)


def _case(kind, k, s, cin, cout, n, h, w, dev):
    from shallow_ntc_amd import ops
    rng = np.random.default_rng(zlib.crc32(repr((kind, k, s, cin, cout, n, h, w)).encode()))
    wshape = (k, k, cout, cin) if kind == "convT" else (k, k, cin, cout)
    wk = (rng.standard_normal(wshape) / np.sqrt(max(k * k * cin / 4, 1))).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    x = rng.standard_normal((n, h, w, cin)).astype(np.float32)
    ref = REF[kind](x, wk, b, s)
    return ops.ConvPlan(kind, _dev_t(wk, dev), _dev_t(b, dev), s), _dev_t(x, dev), ref


class _state:
    """Restores the process-wide schedule state and the plan's forced choices; a timed-out stream-K hand-off fails the test."""

    def __init__(self, plan):
        self.plan = plan

    def __enter__(self):
        from shallow_ntc_amd import ops
        self.sk = ops.stream_k_enabled()
        ops.set_stream_k(True)
        return self

    def __exit__(self, *exc):
        from shallow_ntc_amd import ops
        try:
            self.plan.set_tile(0)
            self.plan.set_stream_k(True)
            self.plan.clear_tuning()
        finally:
            ops.set_stream_k(self.sk)
            if exc[0] is not None:
                ops.take_conv_status()
        if exc[0] is None:
            ops.check_conv_status()
        return False


def _forced_static(plan, x, ref, n, h, w, what):
    """The static schedule on every forced instance: the oracle's bar each, one set of bits."""
    bits = None
    for v, dma in FORCED:
        plan.set_tile(v)
        plan.set_stream_k(False, dma=dma)
        assert plan.launch_info(n, h, w)[0] == v
        y = plan(x).clone()
        _within(y, ref, f"{what} variant {v}{' dma' if dma else ''}")
        if bits is None:
            bits = y
        assert torch.equal(y, bits), (what, v, dma)
    return bits


BORDERS = [  # kind, k, s, cin, cout, n, h, w
    ("conv", 3, 1, 32, 64, 3, 5, 7),        # M = 105: three images and 23 padding rows in one 128-row tile
    ("conv", 5, 2, 32, 64, 2, 9, 11),       # 5x5 / 2 down: M = 60
    ("convT", 5, 2, 32, 48, 2, 4, 6),       # four phase groups, 3x3 ... 2x2 taps, tstep = -1
    ("convT", 13, 8, 16, 24, 1, 3, 4),      # 2x2 ... 1x1 taps per phase group, the macro grid one larger than the image
]


@gpu
@pytest.mark.parametrize("case", BORDERS, ids=lambda c: "-".join(map(str, c)))
def test_borders_images_and_padding_rows_in_one_tile(case, dev):
    kind, k, s, cin, cout, n, h, w = case
    plan, x, ref = _case(*case, dev)
    with _state(plan):
        _forced_static(plan, x, ref, n, h, w, "-".join(map(str, case)))


@gpu
@pytest.mark.parametrize("cin", [16, 32, 48, 64, 80, 96, 112])
def test_one_to_seven_stages_per_tile(cin, dev):
    """1x1, Cin = 16 s: s stages per tile -- n = 1 ... 5 and more of the two-set loop's prologue and tail."""
    n, h, w = 1, 8, 8
    plan, x, ref = _case("conv", 1, 1, cin, 40, n, h, w, dev)
    with _state(plan):
        _forced_static(plan, x, ref, n, h, w, f"1x1 cin {cin}")


PIECES = [  # n, h, w, does forced stream-K really cut this launch
    # schedule() in conv_plan.hip runs stream-K only with at least half of an instance's resident workgroups at work: these 8 ...
    # 16 tiles stay one workgroup per tile however hard stream-K is forced, and the static schedule runs the layer unsplit (the
    # split rule needs K >= 2048, this layer has K = 432; a plan has no switch that forces a split).  Kept: the forced calls
    # must still give the oracle's values and the same bits
    (4, 16, 16, False),
    # M = 60480: 473 tiles of 128 rows on 472 workers, 945 tiles of 64 rows on 944: equal shares of 27.06 stages, so the cuts
    # creep through every stage of a tile -- pieces that start and end on odd and on even stages, one- and two-stage pieces
    (4, 120, 126, True),
]


@gpu
@pytest.mark.parametrize("shape", PIECES, ids=lambda c: "-".join(map(str, c)))
def test_pieces_that_start_and_end_on_odd_and_even_stages(shape, dev):
    """3x3, 48 -> 64: 27 stages per tile.  Stream-K forced on variants 2, 8, 9 and the column-major twin of 9, after the static
    schedule on every forced instance."""
    n, h, w, cut = shape
    plan, x, ref = _case("conv", 3, 1, 48, 64, n, h, w, dev)
    with _state(plan):
        bits = _forced_static(plan, x, ref, n, h, w, "3x3 48->64 static")
        for v, colm in [(2, False), (8, False), (9, False), (9, True)]:
            plan.set_tile(v)
            plan.set_stream_k(False, dma=False)
            nb_static = plan.launch_info(n, h, w)[1]
            plan.set_stream_k(True, dma=False, force=True, colm=colm)
            v_sk, nb_sk = plan.launch_info(n, h, w)
            assert v_sk == v
            if cut:
                assert nb_sk < nb_static and nb_static % nb_sk != 0, (v, nb_sk, nb_static)     # shares are no whole tiles
                assert plan.launch_order(n, h, w) == colm, (v, colm)
            y = plan(x)
            _within(y, ref, f"3x3 48->64 stream-K variant {v}{' colm' if colm else ''} ({nb_sk} workgroups, {nb_static} tiles)")
            assert torch.equal(y, bits), (v, colm)


@gpu
def test_split_k_ranges_on_odd_and_even_stages(dev):
    """A real static split-K launch of the same 3x3 layer shape, at the smallest Cin the split rule takes: 3x3, 240 -> 64 is 135
    stages in eight K ranges that start at stages 16, 33, 50, 67, 84, 101 and 118."""
    from shallow_ntc_amd import _capi as capi
    case = ("conv", 3, 1, 240, 64, 2, 16, 16)
    kind, k, s, cin, cout, n, h, w = case
    plan, x, ref = _case(*case, dev)
    with _state(plan):
        plan.set_stream_k(False)
        assert int(capi.load().sntc_conv_workspace_bytes(plan._h, n, h, w)) > 0      # the split-K slabs: the launch is split
        _forced_static(plan, x, ref, n, h, w, "3x3 240->64 split-K")
