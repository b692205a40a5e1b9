"""The register-staged K loop of the gather GEMM with compile-time ring slots (csrc/gather_gemm_kernel.h, SLOTS3):
three stages per loop iteration in slots 0, 1, 2, then up to five tail steps, one copy per position.

Every case meets the float64 oracle at the bar of test_hip_gemm_loader (2e-5 * max(|ref|, 1)) on forced variants 1, 2, 3, 4, 5, 8, 9
and on the column-major twin of 9, and all of them give the bits of variant 2 with direct-to-LDS staging (torch.equal): that
instance has a loop of its own, which this change does not touch, so it is the bit reference.

The shapes are the smallest at which the loop can go wrong:
  1. 1 to 10 K stages per tile: every remainder of the triple loop with zero, one and two trips through it, pieces shorter than
     the ring included;
  2. stream-K shares of 27.06 stages: the cuts creep through every stage of a tile, so pieces start (at ring slot 0) on every
     residue of the stage number mod 3 and have every length;
  3. static split-K ranges of 16 and 17 stages;
  4. four phase groups with different tap grids in one launch.
"""
import zlib

import numpy as np
import pytest
import torch

from oracle import ops_np as O

gpu = pytest.mark.gpu

TOL = 2e-5
REF = {"conv": O.conv2d, "convT": O.conv2d_transpose}
BIT_REFERENCE = (2, True)                                    # (variant, direct-to-LDS)
RING = [1, 2, 3, 4, 5, 8, 9]                                 # register-staged variants


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


def _forced(plan, x, ref, n, h, w, what):
    """The direct-to-LDS reference first, then the static schedule on every register-staged variant and the column-major twin of
    variant 9 (a stream-K instance: forced, it runs whole tiles where the launch is too small to cut): the oracle's bar each, the
    reference's bits."""
    v, dma = BIT_REFERENCE
    plan.set_tile(v)
    plan.set_stream_k(False, dma=dma)
    assert plan.launch_info(n, h, w)[0] == v
    bits = plan(x).clone()
    _within(bits, ref, f"{what} variant {v} dma")
    for v in RING:
        plan.set_tile(v)
        plan.set_stream_k(False, dma=False)
        assert plan.launch_info(n, h, w)[0] == v
        y = plan(x)
        _within(y, ref, f"{what} variant {v}")
        assert torch.equal(y, bits), (what, v)
    plan.set_tile(9)
    plan.set_stream_k(True, dma=False, force=True, colm=True)
    assert plan.launch_info(n, h, w)[0] == 9
    y = plan(x)
    _within(y, ref, f"{what} variant 9 colm")
    assert torch.equal(y, bits), (what, "9 colm")
    return bits


@gpu
@pytest.mark.parametrize("stages", range(1, 11))
def test_every_remainder_of_the_triple_loop(stages, dev):
    """1x1, Cin = 16 s at 1 x 8 x 8 -> 40 channels: s stages per tile.  s <= 5 runs in the tail alone (s <= 2: shorter than the
    ring), 6 ... 8 take the loop once and leave 3 ... 5, 9 and 10 take it twice and leave 3 and 4."""
    n, h, w = 1, 8, 8
    plan, x, ref = _case("conv", 1, 1, 16 * stages, 40, n, h, w, dev)
    with _state(plan):
        _forced(plan, x, ref, n, h, w, f"1x1 cin {16 * stages}")


@gpu
def test_stream_k_pieces_of_every_length_and_start(dev):
    """3x3, 48 -> 64 at (4, 120, 126): 27 stages per tile, M = 60480 -- 473 tiles of 128 rows on 472 workers, 945 tiles of 64
    rows on 944: equal shares of 27.06 stages."""
    n, h, w = 4, 120, 126
    plan, x, ref = _case("conv", 3, 1, 48, 64, n, h, w, dev)
    with _state(plan):
        bits = _forced(plan, x, ref, n, h, w, "3x3 48->64 static")
        for v, colm in [(v, False) for v in RING] + [(9, True)]:
            plan.set_tile(v)
            plan.set_stream_k(False, dma=False)
            nb_static = plan.launch_info(n, h, w)[1]
            plan.set_stream_k(True, dma=False, force=True, colm=colm)
            v_sk, nb_sk = plan.launch_info(n, h, w)
            assert v_sk == v
            if v in (2, 8, 9):      # the 64-column tiles fit the layer: one tile column, shares that are no whole tiles
                assert nb_sk < nb_static and nb_static % nb_sk != 0, (v, nb_sk, nb_static)
                assert plan.launch_order(n, h, w) == colm, (v, colm)
            y = plan(x)
            _within(y, ref, f"3x3 48->64 stream-K variant {v}{' colm' if colm else ''} ({nb_sk} workgroups, {nb_static} tiles)")
            assert torch.equal(y, bits), (v, colm)


@gpu
def test_split_k_ranges(dev):
    """3x3, 240 -> 64 at 2 x 16 x 16: 135 stages in eight K ranges of 16 and 17 stages (remainders 4 and 5 after four triples)."""
    from shallow_ntc_amd import _capi as capi
    case = ("conv", 3, 1, 240, 64, 2, 16, 16)
    kind, k, s, cin, cout, n, h, w = case
    plan, x, ref = _case(*case, dev)
    with _state(plan):
        plan.set_stream_k(False)
        assert int(capi.load().sntc_conv_workspace_bytes(plan._h, n, h, w)) > 0      # the split-K slabs: the launch is split
        _forced(plan, x, ref, n, h, w, "3x3 240->64 split-K")


@gpu
def test_phase_groups(dev):
    """convT 5x5 / 2, 32 -> 48 at 2 x 4 x 6: four phase groups, 3x3 ... 2x2 taps (18, 12, 12 and 8 stages), tstep = -1."""
    case = ("convT", 5, 2, 32, 48, 2, 4, 6)
    kind, k, s, cin, cout, n, h, w = case
    plan, x, ref = _case(*case, dev)
    with _state(plan):
        _forced(plan, x, ref, n, h, w, "-".join(map(str, case)))
